// rt_temporal.h -- the per-pixel arithmetic of rt_render_motion and of the temporal accumulator (rt_temporal_accumulate_moments_fixed,
// and rt_temporal_accumulate_fixed, which is the same call with the newer features off: include/rtcuda_amd.h, DESIGN.md sections
// 2.9 and 2.10), as a fixed sequence of individually rounded fp32 operations (no FMA: every translation unit that includes it is
// compiled with -ffp-contract=off).  The kernels (k_motion: rt_stream_kernels.inc; k_temporal_accumulate_moments:
// rt_temporal_kernels.inc) and the CPU twins (hc_motion_records, hc_temporal_accumulate_moments: rt_host_check.cpp) call these
// functions and differ only in who walks the pixels.
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

// ---- the temporal accumulator (both entry points)
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

// The accumulator: the four taps with the depth and normal stops, and optionally an emission stop (use_emission), a triangle stop
// (prev_motion given), temporally accumulated first and second moments of demodulated radiance and the variance of the mean they
// give (moments_out given).  What one call is handed, the kernel's parameter block and the twin's alike (host or device pointers;
// the optional ones null).
typedef struct TmMoments {
    const int64_t *sum_a, *sum_b, *aov, *hist_a_in, *hist_b_in, *prev_aov;
    const float *motion, *prev_motion, *moments_in;
    const int32_t *len_in;
    int64_t *out_a, *out_b;
    int32_t *len_out;
    float *moments_out, *variance_out;
    int width, height, tiles_x;
    int32_t max_history, variance_min_history;
    int use_emission;  // emission_tolerance < +inf: the previous frame's emission sums are read at all
    float inv_a, inv_b, inv_n, inv_aov, inv_prev_aov, alpha_min, depth_tolerance, normal_cos_min, emission_tolerance;
} TmMoments;

// The whole block from an entry point's arguments (rt_temporal_accumulate_moments_fixed's, in its order; checked by the caller).
// tiles_x: the kernel's tiles per row (the twin walks rows: 0).
RT_HD void tm_moments_fill(TmMoments *t, const int64_t *sum_a, int samples_a, const int64_t *sum_b, int samples_b, const int64_t *aov,
                           int aov_samples, const float *motion, const int64_t *hist_a_in, const int64_t *hist_b_in, const int32_t *len_in,
                           const int64_t *prev_aov, int prev_aov_samples, const float *prev_motion, const float *moments_in, int width,
                           int height, int tiles_x, int32_t max_history, float alpha_min, float depth_tolerance, float normal_cos_min,
                           float emission_tolerance, int32_t variance_min_history, int64_t *out_a, int64_t *out_b, int32_t *len_out,
                           float *moments_out, float *variance_out) {
    const bool two = sum_b != 0, moments = moments_out != 0;
    t->sum_a = sum_a, t->sum_b = sum_b, t->aov = aov, t->hist_a_in = hist_a_in, t->hist_b_in = hist_b_in, t->prev_aov = prev_aov;
    t->motion = motion, t->prev_motion = prev_motion, t->moments_in = moments_in, t->len_in = len_in;
    t->out_a = out_a, t->out_b = out_b, t->len_out = len_out, t->moments_out = moments_out, t->variance_out = variance_out;
    t->width = width, t->height = height, t->tiles_x = tiles_x;
    t->max_history = max_history, t->variance_min_history = variance_min_history;
    t->use_emission = emission_tolerance <= 3.402823466e+38f;
    t->inv_a = 1.f / (float)samples_a;
    t->inv_b = two ? 1.f / (float)samples_b : 0.f;
    t->inv_n = 1.f / (float)(two && moments ? samples_a + samples_b : samples_a);
    t->inv_aov = 1.f / (float)aov_samples;
    t->inv_prev_aov = hist_a_in ? 1.f / (float)prev_aov_samples : 0.f;
    t->alpha_min = alpha_min, t->depth_tolerance = depth_tolerance, t->normal_cos_min = normal_cos_min;
    t->emission_tolerance = emission_tolerance;
}

// a moments record is one 16-byte access on the device (the entry point checks the alignment; the twin's host buffers need none)
#ifdef __HIP_DEVICE_COMPILE__
#define TM_RECORD(p) __builtin_assume_aligned(p, 16)
#else
#define TM_RECORD(p) (p)
#endif

// the triangle id rides in a motion record's fourth float
RT_HD int32_t tm_tri_of(float w) {
    union { float f; int32_t i; } bits;
    bits.f = w;
    return bits.i;
}

RT_HD void tm_emission(const int64_t *aov11, float inv_aov, float *e3) {
    for (int k = 0; k < 3; k++) e3[k] = dn_fixed_to_float(aov11[DN_EMISSION + k]) * inv_aov;
}

// the emission stop: the largest channel difference, by comparison and selection from channel 0, against the tolerance
RT_HD bool tm_emission_accept(const float *e_p, const int64_t *prev_aov11, float inv_prev_aov, float emission_tolerance) {
    float e_q[3];
    tm_emission(prev_aov11, inv_prev_aov, e_q);
    float de = 0.f;
    for (int k = 0; k < 3; k++) {
        const float d = e_p[k] - e_q[k];
        const float ad = d < 0.f ? -d : d;
        de = k == 0 ? ad : (ad > de ? ad : de);
    }
    return de <= emission_tolerance;
}

// The frame's moments of pixel q: u is the dual denoiser's step-1 demodulated radiance of the (wrapped) sum of the supplied
// buffers, f = {u.x, u.y, u.z, dot(u, u)}.  Also the features the spatial estimate's stops need (dn_prepare forms n and z as
// tm_features does).  Returns the hit count.
RT_HD int64_t tm_frame_moments(const TmMoments *t, long long q, float *f4, float *n3, float *z) {
    int64_t s[3];
    for (int k = 0; k < 3; k++) s[k] = t->sum_b ? (int64_t)((uint64_t)t->sum_a[3 * q + k] + (uint64_t)t->sum_b[3 * q + k]) : t->sum_a[3 * q + k];
    DnPixel px;
    dn_prepare(s, t->aov + DN_AOV_CHANNELS * q, t->inv_n, t->inv_aov, &px);
    for (int k = 0; k < 3; k++) f4[k] = px.u[k], n3[k] = px.n[k];
    f4[3] = tm_dot(px.u, px.u);
    *z = px.z;
    return t->aov[DN_AOV_CHANNELS * q + DN_HITS];
}

RT_HD float tm_variance_of(const float *m4, int32_t n) {
    const float t = m4[3] - tm_dot(m4, m4);
    return (t > 0.f ? t : 0.f) / (float)n;
}

// The spatial estimate of this frame at (x, y): the moments' mean over the 5 x 5 window's taps that pass the depth and normal
// stops against the centre (which always counts).  tap(dx, dy, q, f_q, n_q, &z_q) hands back the moments and features of the
// neighbour (dx, dy), which is pixel q of the frame, and whether it has hits: from global memory (tm_spatial_variance) or from a
// staged tile (k_temporal_accumulate_moments) -- with the front's one bool the use of C++ in this header.
template <typename Tap>
RT_HD float tm_spatial_variance_of(const TmMoments *t, int x, int y, const float *f_p, const float *n_p, float z_p, int32_t n, Tap tap) {
    float cnt = 0.f, s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int dy = -2; dy <= 2; dy++) {
        const int yy = y + dy;
        if (yy < 0 || yy >= t->height) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int xx = x + dx;
            if (xx < 0 || xx >= t->width) continue;
            float f_q[4] = {f_p[0], f_p[1], f_p[2], f_p[3]};
            if (dx != 0 || dy != 0) {
                float n_q[3], z_q;
                if (!tap(dx, dy, (long long)yy * t->width + xx, f_q, n_q, &z_q)) continue;
                const float dz = z_q - z_p;
                if (!((dz < 0.f ? -dz : dz) <= t->depth_tolerance * z_p)) continue;
                if (!(tm_dot(n_p, n_q) >= t->normal_cos_min)) continue;
            }
            cnt = cnt + 1.f;
            for (int j = 0; j < 4; j++) s[j] = s[j] + f_q[j];
        }
    }
    float m[4];
    for (int j = 0; j < 4; j++) m[j] = s[j] / cnt;
    return tm_variance_of(m, n);
}
// the CPU twin's: a tap is the neighbour's beauty and AOV sums, demodulated here
RT_HD float tm_spatial_variance(const TmMoments *t, int x, int y, const float *f_p, const float *n_p, float z_p, int32_t n) {
    return tm_spatial_variance_of(t, x, y, f_p, n_p, z_p, n, [t](int, int, long long q, float *f_q, float *n_q, float *z_q) {
        return tm_frame_moments(t, q, f_q, n_q, z_q) > 0;
    });
}

// One pixel (x, y), both colour buffers in one pass over the taps (sum_b, hist_b_in and out_b are null together; hist_a_in null: the
// first frame; mo: the pixel's motion record), with the emission stop (use_emission), the triangle stop (prev_motion given) and,
// with moments_out given, the moments through the same taps and weights and the variance of the mean -- all but the spatial estimate:
// returns true where that is still owed (variance_out[p] not written), with what it needs: the frame's moments f, n_p, z_p and N.
// FEATURES false: the three are compiled out whatever t says (k_temporal_accumulate's instantiation), and the answer is false.
template <bool FEATURES>
RT_HD bool tm_accumulate_moments_front(const TmMoments *t, int x, int y, const float *mo, float *f, float *n_p, float *z_p_out, int32_t *n_out) {
    const int width = t->width, height = t->height;
    const long long p = (long long)y * width + x;
    const bool two = t->sum_b != 0, moments = FEATURES && t->moments_out != 0;
    float ca[3], cb[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; k++) {
        ca[k] = dn_fixed_to_float(t->sum_a[3 * p + k]) * t->inv_a;
        if (two) cb[k] = dn_fixed_to_float(t->sum_b[3 * p + k]) * t->inv_b;
    }
    float z_p = 0.f;
    for (int k = 0; k < 4; k++) f[k] = 0.f;
    for (int k = 0; k < 3; k++) n_p[k] = 0.f;
    if (moments) (void)tm_frame_moments(t, p, f, n_p, &z_p);
    float sw = 0.f, sa[3] = {0.f, 0.f, 0.f}, sb[3] = {0.f, 0.f, 0.f}, sm[4] = {0.f, 0.f, 0.f, 0.f};
    int32_t n_prev = 0x7fffffff;
    const int32_t tri = tm_tri_of(mo[3]);
    if (t->hist_a_in && tri >= 0) {
        const float fx = mo[0] - 0.5f, fy = mo[1] - 0.5f, dist = mo[2];
        if (fx >= -1.f && fx < (float)width && fy >= -1.f && fy < (float)height) {  // (false for a NaN)
            float e_p[3] = {0.f, 0.f, 0.f};
            if (!moments) (void)tm_features(t->aov + DN_AOV_CHANNELS * p, t->inv_aov, n_p, &z_p);
            if (FEATURES && t->use_emission) tm_emission(t->aov + DN_AOV_CHANNELS * p, t->inv_aov, e_p);
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
                    const int32_t len_q = t->len_in[q];
                    const int64_t *aov_q = t->prev_aov + DN_AOV_CHANNELS * q;
                    if (!tm_tap_accept(len_q, aov_q, t->inv_prev_aov, n_p, dist, t->depth_tolerance, t->normal_cos_min)) continue;
                    if (FEATURES && t->use_emission && !tm_emission_accept(e_p, aov_q, t->inv_prev_aov, t->emission_tolerance)) continue;
                    if (FEATURES && t->prev_motion && tm_tri_of(t->prev_motion[4 * q + 3]) != tri) continue;
                    const float b = (i ? ax : 1.f - ax) * (j ? ay : 1.f - ay);
                    sw = sw + b;
                    for (int k = 0; k < 3; k++) {
                        sa[k] = sa[k] + b * dn_fixed_to_float(t->hist_a_in[3 * q + k]);
                        if (two) sb[k] = sb[k] + b * dn_fixed_to_float(t->hist_b_in[3 * q + k]);
                    }
                    if (moments && t->moments_in) {
                        const float *m_q = (const float *)TM_RECORD(t->moments_in) + 4 * q;
                        for (int k = 0; k < 4; k++) sm[k] = sm[k] + b * m_q[k];
                    }
                    n_prev = len_q < n_prev ? len_q : n_prev;
                }
            }
        }
    }
    int32_t n = 1;
    float m[4] = {f[0], f[1], f[2], f[3]};
    if (sw > 0.f) {
        n = tm_history_length(n_prev, t->max_history);
        const float alpha = tm_alpha(n, t->alpha_min);
        for (int k = 0; k < 3; k++) {
            t->out_a[3 * p + k] = tm_to_fixed(tm_blend(ca[k], sa[k] / sw, alpha));
            if (two) t->out_b[3 * p + k] = tm_to_fixed(tm_blend(cb[k], sb[k] / sw, alpha));
        }
        if (moments && t->moments_in)
            for (int k = 0; k < 4; k++) m[k] = tm_blend(f[k], sm[k] / sw, alpha);
    } else {
        for (int k = 0; k < 3; k++) {
            t->out_a[3 * p + k] = tm_to_fixed(ca[k]);
            if (two) t->out_b[3 * p + k] = tm_to_fixed(cb[k]);
        }
    }
    t->len_out[p] = n;
    *z_p_out = z_p;
    *n_out = n;
    if (!moments) return false;
    float *m_out = (float *)TM_RECORD(t->moments_out) + 4 * p;
    for (int k = 0; k < 4; k++) m_out[k] = m[k];
    if (n < t->variance_min_history) return true;
    t->variance_out[p] = tm_variance_of(m, n);
    return false;
}
RT_HD void tm_accumulate_moments_pixel(const TmMoments *t, int x, int y, const float *mo) {
    float f[4], n_p[3], z_p;
    int32_t n;
    if (tm_accumulate_moments_front<true>(t, x, y, mo, f, n_p, &z_p, &n))
        t->variance_out[(long long)y * t->width + x] = tm_spatial_variance(t, x, y, f, n_p, z_p, n);
}

#endif  // RT_TEMPORAL_H
