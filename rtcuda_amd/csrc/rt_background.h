// rt_background.h -- the pixel rectangle outside which no camera ray of a pinhole frame can hit the scene (host only; shared
// by render_shard_impl, which hands it to k_paths / k_paths<PathsChunked> in AdvanceParams, and by rt_host_check.cpp, which exports
// it for the tests as rt_background_rect).
//
// Guarantee.  For every pixel (px, py) outside [x0, x1) x [y0, y1) and every jitter (jx, jy) in [0, 1)^2, the ray gen_core
// makes -- camera_get_ray(cam, (px + jx) / width, (py + jy) / height) -- misses every triangle of the scene, under the
// product's walk of its padded records and under the reference's literal walk.
//
// The chain.
//   (1) Every box either walk tests, and every triangle, lies inside B = [lo - m, hi + m], with lo / hi the bounds of the
//       builder's records (the root's children: they contain everything below them) and, per axis a,
//           m_a = 1e-4 (hi_a - lo_a)                    slack for the triangle test's own rounding
//               + 2^-22 R_a + 2^-20 max(|lo_a|, |hi_a|) the records' padding: 2^-23 R_a (pad_quads_for_origins, R = the
//                                                       origin radius the scene is padded for) and 2 + 1 + 1 ulps
//               + 2^-17 D                               a box test that accepts a ray passing outside the box: the exit
//                                                       distance widened by 1.000001 and the fp32 slab arithmetic (~1e-6 of
//                                                       the distance travelled), the reference's 1 / d clamped to FLT_EPSILON
//                                                       (1.2e-7 of it); D bounds the distance from lookfrom to any point of B.
//                                                       (kCullTmaxWiden widens the far limit of a ray, FLT_MAX for a camera
//                                                       ray: it adds nothing here.)
//       A walk reaches a triangle only through a box that holds it, so a ray that passes B by more than rounding hits nothing.
//   (2) The exact ray through the plane point P(u, v) = upper_left + u horizontal + v vertical meets B only if (u, v) is the
//       central projection, from lookfrom, of a point of B.  With all 8 corners of B strictly in front of the camera (depth
//       a > 0 along horizontal x vertical, oriented towards upper_left - lookfrom) the projection of B is the convex hull of
//       the projected corners, which lies inside the bounding interval [u0, u1] x [v0, v1] of the eight (u, v).  The corner
//       Q - lookfrom = a (upper_left - lookfrom) + b horizontal + c vertical projects to (b / a, c / a): solved in the basis
//       as given, which need not be orthogonal.
//   (3) A pixel outside x0' = floor(u0 width), x1' = ceil(u1 width) (exclusive) has (px + jx) / width <= u0 or >= u1 for
//       every jitter, in exact arithmetic; likewise the rows.  The fp32 ray differs from the exact one: (px + jx) / width,
//       the sum upper_left + x horizontal + y vertical - lookfrom and unit() are rounded, together below 2^-20 (|upper_left|
//       + |horizontal| + |vertical| + |lookfrom|) in the plane -- the frame is given up (whole-frame rectangle) unless that
//       is under a quarter of a pixel step, |horizontal| / width and |vertical| / height -- and the walks' remaining
//       rounding is in m.  The rectangle is x0' - 1 .. x1' + 1, y0' - 1 .. y1' + 1: one whole pixel (5e-4 of a 1920-wide
//       frame) for errors of about 1e-6.
// Whole frame (nothing is skipped): a corner not strictly in front (unless all eight are strictly behind), a degenerate
// basis, anything non-finite, a frame whose pixel step does not dominate the rounding.  A scene wholly off screen, wholly
// behind the camera (a camera ray only reaches positive depths) or without a box gives the empty rectangle {0, 0, 0, 0}.
#pragma once

#include <cmath>

namespace rtbg {

struct Rect {
    int x0, y0, x1, y1;  // pixels [x0, x1) x [y0, y1); x0 == x1: empty
};

// cam12: lookfrom, upper_left, horizontal, vertical (rt_camera's floats, in order).  radius3: the origin radius the scene's
// records are padded for, or null (then the one a render would ask for: twice 1.001 x the largest coordinate, with room).
inline Rect background_rect(const float cam12[12], int width, int height, const float lo3[3], const float hi3[3],
                            const float *radius3 = nullptr) {
    const Rect whole{0, 0, width, height}, empty{0, 0, 0, 0};
    if (width <= 0 || height <= 0) return empty;
    double lf[3], w0[3], hz[3], vt[3];
    for (int a = 0; a < 3; a++) {
        lf[a] = cam12[a];
        w0[a] = (double)cam12[3 + a] - (double)cam12[a];
        hz[a] = cam12[6 + a];
        vt[a] = cam12[9 + a];
    }
    for (int k = 0; k < 12; k++)
        if (!std::isfinite(cam12[k])) return whole;
    bool any_box = true;
    for (int a = 0; a < 3; a++) {
        if (std::isnan(lo3[a]) || std::isnan(hi3[a])) return whole;
        if (!(lo3[a] <= hi3[a])) any_box = false;  // (an empty scene: lo = +FLT_MAX, hi = -FLT_MAX)
    }
    if (!any_box) return empty;
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(lo3[a]) || !std::isfinite(hi3[a])) return whole;
    // the basis: n = horizontal x vertical, towards upper_left - lookfrom
    double n[3] = {hz[1] * vt[2] - hz[2] * vt[1], hz[2] * vt[0] - hz[0] * vt[2], hz[0] * vt[1] - hz[1] * vt[0]};
    const double hh = hz[0] * hz[0] + hz[1] * hz[1] + hz[2] * hz[2], vv = vt[0] * vt[0] + vt[1] * vt[1] + vt[2] * vt[2];
    const double hv = hz[0] * vt[0] + hz[1] * vt[1] + hz[2] * vt[2];
    const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const double wn = w0[0] * n[0] + w0[1] * n[1] + w0[2] * n[2];
    const double ww = w0[0] * w0[0] + w0[1] * w0[1] + w0[2] * w0[2];
    if (!(hh > 0.0) || !(vv > 0.0) || !std::isfinite(hh * vv) || !std::isfinite(nn) || !std::isfinite(wn)) return whole;
    if (!(nn > 1e-12 * hh * vv)) return whole;            // horizontal and vertical (nearly) parallel
    if (!(wn * wn > 1e-12 * nn * ww)) return whole;       // lookfrom (nearly) in the image plane
    // the rounding of the fp32 ray against the pixel step (step 3 of the chain)
    {
        double mag = 0.0;
        for (int k = 0; k < 12; k++) mag = std::fmax(mag, std::fabs((double)cam12[k]));
        const double err = std::ldexp(4.0 * mag, -20);
        if (!(err < 0.25 * std::sqrt(hh) / width) || !(err < 0.25 * std::sqrt(vv) / height)) return whole;
    }
    // B: the inflated bounds (step 1)
    double dist = 0.0;
    for (int a = 0; a < 3; a++) dist += std::fmax(std::fabs(lo3[a]), std::fabs(hi3[a])) + std::fabs(lf[a]);
    double blo[3], bhi[3];
    for (int a = 0; a < 3; a++) {
        const double big = std::fmax(std::fabs((double)lo3[a]), std::fabs((double)hi3[a]));
        double rad = 4.0 * std::fmax(big, std::fabs(lf[a]));
        if (radius3 && std::isfinite(radius3[a])) rad = std::fmax(rad, std::fabs((double)radius3[a]));
        const double m = 1e-4 * ((double)hi3[a] - (double)lo3[a]) + std::ldexp(rad, -22) + std::ldexp(big, -20) + std::ldexp(2.0 * dist, -17);
        blo[a] = (double)lo3[a] - m;
        bhi[a] = (double)hi3[a] + m;
    }
    // the corners' projections (step 2): Q - lookfrom = a w0 + b horizontal + c vertical
    double u0 = INFINITY, u1 = -INFINITY, v0 = INFINITY, v1 = -INFINITY;
    int behind = 0;
    for (int k = 0; k < 8; k++) {
        double q[3];
        for (int a = 0; a < 3; a++) q[a] = (((k >> a) & 1) ? bhi[a] : blo[a]) - lf[a];
        const double depth = (q[0] * n[0] + q[1] * n[1] + q[2] * n[2]) / wn;
        const double qq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
        // strictly on one side: by more than the solve's own rounding (relative to the corner's distance)
        behind += (depth < 0.0 && depth * depth * ww > 1e-12 * qq) ? 1 : 0;
    }
    // (every point of a camera ray has positive depth: a scene wholly behind the camera is never reached)
    if (behind == 8) return empty;
    for (int k = 0; k < 8; k++) {
        double q[3];
        for (int a = 0; a < 3; a++) q[a] = (((k >> a) & 1) ? bhi[a] : blo[a]) - lf[a];
        const double depth = (q[0] * n[0] + q[1] * n[1] + q[2] * n[2]) / wn;  // a
        const double qq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
        if (!(depth > 0.0) || !(depth * depth * ww > 1e-12 * qq)) return whole;
        double r[3];
        for (int a = 0; a < 3; a++) r[a] = q[a] - depth * w0[a];  // = b horizontal + c vertical (in the plane of the basis)
        const double rh = r[0] * hz[0] + r[1] * hz[1] + r[2] * hz[2], rv = r[0] * vt[0] + r[1] * vt[1] + r[2] * vt[2];
        const double b = (rh * vv - rv * hv) / nn, c = (rv * hh - rh * hv) / nn;  // (Gram determinant = |h x v|^2)
        const double u = b / depth, v = c / depth;
        if (!std::isfinite(u) || !std::isfinite(v)) return whole;
        u0 = std::fmin(u0, u);
        u1 = std::fmax(u1, u);
        v0 = std::fmin(v0, v);
        v1 = std::fmax(v1, v);
    }
    // pixels, rounded outward, one whole pixel wider on every side (step 3); clamped before the conversion to int
    auto lo_px = [](double t, int size) { return (int)std::fmin(std::fmax(std::floor(t * size) - 1.0, 0.0), (double)size); };
    auto hi_px = [](double t, int size) { return (int)std::fmin(std::fmax(std::ceil(t * size) + 1.0, 0.0), (double)size); };
    const Rect r{lo_px(u0, width), lo_px(v0, height), hi_px(u1, width), hi_px(v1, height)};
    if (r.x0 >= r.x1 || r.y0 >= r.y1) return empty;
    return r;
}

// the bounds of the builder's 4-wide records: the root's children (a record: two boxes lo xyz / hi xyz and two links; `absent`:
// the link of a child that is not there).  Returns false if the root has no child: lo > hi then.
template <class PAIR>
inline bool root_bounds(const PAIR *root2, int absent, float lo3[3], float hi3[3]) {
    bool any = false;
    for (int a = 0; a < 3; a++) {
        lo3[a] = INFINITY;
        hi3[a] = -INFINITY;
    }
    for (int k = 0; k < 4; k++) {
        const PAIR &p = root2[k >> 1];
        if (((k & 1) ? p.rlink : p.llink) == absent) continue;
        const float *b = (k & 1) ? p.rbox : p.lbox;
        any = true;
        for (int a = 0; a < 3; a++) {
            lo3[a] = std::fmin(lo3[a], b[a]);
            hi3[a] = std::fmax(hi3[a], b[3 + a]);
        }
    }
    return any;
}

}  // namespace rtbg
