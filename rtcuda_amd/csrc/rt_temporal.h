// rt_temporal.h -- the per-pixel arithmetic of rt_render_motion and rt_temporal_accumulate_fixed (include/rtcuda_amd.h, DESIGN.md
// section 2.9), as a fixed sequence of individually rounded fp32 operations (no FMA: every translation unit that includes it is
// compiled with -ffp-contract=off).  The kernels (k_motion: rt_stream_kernels.inc; k_temporal_accumulate: rt_temporal_kernels.inc)
// and the CPU twins (hc_motion_records, hc_temporal_accumulate: rt_host_check.cpp) call these functions and differ only in who
// walks the pixels.
//
// Plain C subset; usable from g++ (host) and hipcc (device).
#ifndef RT_TEMPORAL_H
#define RT_TEMPORAL_H

#include <math.h>
#include <stdint.h>

#include "rt_denoise.h"  // dn_fixed_to_float, the DN_* channel offsets of the AOV sums

// dot as everywhere in the library: (x * x + y * y) + z * z
RT_HD float tm_dot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the kernels' to_fixed: magnitudes clamped to 2^31, NaN to 0, units of 2^-30, round to nearest even (x * 2^30 is exact; a
// product of 2^23 or more is an integer already)
RT_HD int64_t tm_to_fixed(float x) {
    const float m = x < 0.f ? -x : x;
    if (!(m <= 2147483648.f)) x = (x == x) ? (x < 0.f ? -2147483648.f : 2147483648.f) : 0.f;
    return (int64_t)rintf(x * 1073741824.f);
}

// ---- rt_render_motion
// What of the previous camera does not depend on the pixel, formed once per call (on the host) by the operations of step 5:
// A = upper_left' - lookfrom', m = cross(horizontal', vertical') (rt_device.h's cross), dot(A, m), dot(h', h'), dot(v', v').
typedef struct TmCamera {
    float lookfrom[3], A[3], m[3], h[3], v[3];
    float Am, hh, vv;
    float fw, fh;  // float(width), float(height)
} TmCamera;

RT_HD void tm_camera(const float *cam12 /* rt_camera: lookfrom, upper_left, horizontal, vertical */, int width, int height, TmCamera *c) {
    const float *lf = cam12, *ul = cam12 + 3, *h = cam12 + 6, *v = cam12 + 9;
    for (int k = 0; k < 3; k++) {
        c->lookfrom[k] = lf[k];
        c->A[k] = ul[k] - lf[k];
        c->h[k] = h[k];
        c->v[k] = v[k];
    }
    c->m[0] = h[1] * v[2] - h[2] * v[1];
    c->m[1] = h[2] * v[0] - h[0] * v[2];
    c->m[2] = h[0] * v[1] - h[1] * v[0];
    c->Am = tm_dot(c->A, c->m);
    c->hh = tm_dot(h, h);
    c->vv = tm_dot(v, v);
    c->fw = (float)width;
    c->fh = (float)height;
}

// Step 4: tri_point on a stored record {q0, e1, e2}, and on the three vertices of a caller's row (e1 = q0 - q1, e2 = q2 - q0).
RT_HD void tm_point(const float *q0, const float *e1, const float *e2, float u, float v, float *P) {
    for (int k = 0; k < 3; k++) P[k] = (q0[k] - e1[k] * u) + e2[k] * v;
}
RT_HD void tm_point_of_vertices(const float *q9, float u, float v, float *P) {
    float e1[3], e2[3];
    for (int k = 0; k < 3; k++) {
        e1[k] = q9[k] - q9[3 + k];
        e2[k] = q9[6 + k] - q9[k];
    }
    tm_point(q9, e1, e2, u, v, P);
}

// Steps 5 and 6: where P lay on the previous camera's image plane, in continuous pixel coordinates, and how far from its pinhole.
// rec = {sx, sy, dist}; {-1, -1, dist} when P is behind or beside the pinhole (lam not positive and finite).
RT_HD void tm_project(const TmCamera *c, const float *P, float *rec3) {
    float a[3], r[3];
    for (int k = 0; k < 3; k++) a[k] = P[k] - c->lookfrom[k];
    const float lam = c->Am / tm_dot(a, c->m);
    for (int k = 0; k < 3; k++) r[k] = a[k] * lam - c->A[k];
    const float sx = (tm_dot(r, c->h) / c->hh) * c->fw;
    const float sy = (tm_dot(r, c->v) / c->vv) * c->fh;
    const bool valid = lam > 0.f && lam <= 3.402823466e+38f;
    rec3[0] = valid ? sx : -1.f;
    rec3[1] = valid ? sy : -1.f;
    rec3[2] = sqrtf(tm_dot(a, a));
}

// ---- rt_temporal_accumulate_fixed
// the mean normal, the mean depth over the hits and the hit count of a pixel's AOV sums, exactly as rt_aov_resolve forms them
RT_HD int64_t tm_features(const int64_t *aov11, float inv_aov, float *n3, float *z) {
    const int64_t hits = aov11[DN_HITS];
    for (int k = 0; k < 3; k++) n3[k] = dn_fixed_to_float(aov11[DN_NORMAL + k]) * inv_aov;
    *z = hits > 0 ? dn_fixed_to_float(aov11[DN_DEPTH]) / (float)hits : 0.f;
    return hits;
}

// Step 3, the stops of one tap that lies inside the image: its history length, the previous frame's hit count, depth and normal.
RT_HD bool tm_tap_accept(int32_t len_q, const int64_t *prev_aov11, float inv_prev_aov, const float *n_p, float dist, float depth_tolerance,
                         float normal_cos_min) {
    if (len_q < 1) return false;
    float n_q[3], z_q;
    if (tm_features(prev_aov11, inv_prev_aov, n_q, &z_q) <= 0) return false;
    const float dz = z_q - dist;
    if (!((dz < 0.f ? -dz : dz) <= depth_tolerance * dist)) return false;
    return tm_dot(n_p, n_q) >= normal_cos_min;
}

// Step 4: N, alpha and the blend of one channel.
RT_HD int32_t tm_history_length(int32_t n_prev, int32_t max_history) { return n_prev >= max_history ? max_history : n_prev + 1; }
RT_HD float tm_alpha(int32_t n, float alpha_min) {
    const float alpha = 1.f / (float)n;
    return alpha > alpha_min ? alpha : alpha_min;
}
RT_HD float tm_blend(float c, float hbar, float alpha) { return (c - hbar) * alpha + hbar; }

// One pixel (x, y), both colour buffers in one pass over the taps.  sum_b, hist_b_in and out_b are null together; hist_a_in null:
// the first frame.  mo: the pixel's motion record.  Writes out_a[3 p ..], out_b[3 p ..] and len_out[p].
RT_HD void tm_accumulate_pixel(int x, int y, int width, int height, const int64_t *sum_a, float inv_a, const int64_t *sum_b, float inv_b,
                               const int64_t *aov, float inv_aov, const float *mo, const int64_t *hist_a_in, const int64_t *hist_b_in,
                               const int32_t *len_in, const int64_t *prev_aov, float inv_prev_aov, int32_t max_history, float alpha_min,
                               float depth_tolerance, float normal_cos_min, int64_t *out_a, int64_t *out_b, int32_t *len_out) {
    const long long p = (long long)y * width + x;
    float ca[3], cb[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; k++) {
        ca[k] = dn_fixed_to_float(sum_a[3 * p + k]) * inv_a;
        if (sum_b) cb[k] = dn_fixed_to_float(sum_b[3 * p + k]) * inv_b;
    }
    float sw = 0.f, sa[3] = {0.f, 0.f, 0.f}, sb[3] = {0.f, 0.f, 0.f};
    int32_t n_prev = 0x7fffffff;
    int32_t tri;
    {
        union { float f; int32_t i; } bits;  // (the triangle id rides in the record's fourth float)
        bits.f = mo[3];
        tri = bits.i;
    }
    if (hist_a_in && tri >= 0) {
        const float fx = mo[0] - 0.5f, fy = mo[1] - 0.5f, dist = mo[2];
        if (fx >= -1.f && fx < (float)width && fy >= -1.f && fy < (float)height) {  // (false for a NaN)
            float n_p[3], z_p;
            (void)tm_features(aov + DN_AOV_CHANNELS * p, inv_aov, n_p, &z_p);
            const float flx = floorf(fx), fly = floorf(fy);
            const int x0 = (int)flx, y0 = (int)fly;
            const float ax = fx - flx, ay = fy - fly;
            for (int j = 0; j < 2; j++) {
                const int yy = y0 + j;
                if (yy < 0 || yy >= height) continue;
                for (int i = 0; i < 2; i++) {
                    const int xx = x0 + i;
                    if (xx < 0 || xx >= width) continue;
                    const long long q = (long long)yy * width + xx;
                    const int32_t len_q = len_in[q];
                    if (!tm_tap_accept(len_q, prev_aov + DN_AOV_CHANNELS * q, inv_prev_aov, n_p, dist, depth_tolerance, normal_cos_min)) continue;
                    const float b = (i ? ax : 1.f - ax) * (j ? ay : 1.f - ay);
                    sw = sw + b;
                    for (int k = 0; k < 3; k++) {
                        sa[k] = sa[k] + b * dn_fixed_to_float(hist_a_in[3 * q + k]);
                        if (sum_b) sb[k] = sb[k] + b * dn_fixed_to_float(hist_b_in[3 * q + k]);
                    }
                    n_prev = len_q < n_prev ? len_q : n_prev;
                }
            }
        }
    }
    if (sw > 0.f) {
        const int32_t n = tm_history_length(n_prev, max_history);
        const float alpha = tm_alpha(n, alpha_min);
        for (int k = 0; k < 3; k++) {
            out_a[3 * p + k] = tm_to_fixed(tm_blend(ca[k], sa[k] / sw, alpha));
            if (sum_b) out_b[3 * p + k] = tm_to_fixed(tm_blend(cb[k], sb[k] / sw, alpha));
        }
        len_out[p] = n;
    } else {
        for (int k = 0; k < 3; k++) {
            out_a[3 * p + k] = tm_to_fixed(ca[k]);
            if (sum_b) out_b[3 * p + k] = tm_to_fixed(cb[k]);
        }
        len_out[p] = 1;
    }
}

#endif  // RT_TEMPORAL_H
