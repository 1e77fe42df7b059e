// rt_denoise.h -- the per-pixel and per-tap arithmetic of rt_denoise_fixed (include/rtcuda_amd.h), as a
// fixed sequence of individually rounded fp32 operations (no FMA: every translation unit that includes it is compiled with
// -ffp-contract=off).  The kernels (rt_denoise_kernels.inc) and the CPU twin (hc_denoise, rt_host_check.cpp) both call these
// three functions and differ only in who walks the pixels.  rt_denoise_dual_fixed's additions follow them.
//
// Plain C subset; usable from g++ (host) and hipcc (device).
#ifndef RT_DENOISE_H
#define RT_DENOISE_H

#include <stdint.h>

#include "rt_pinned_math.h"

#define DN_MAX_PASSES 8
#define DN_MAX_NORMAL_POWER_LOG2 8
#define DN_AOV_CHANNELS 11  // RT_AOV_CHANNELS and the RT_AOV_* offsets, restated for the translation units without the C-ABI header
#define DN_ALBEDO 0
#define DN_NORMAL 3
#define DN_EMISSION 6
#define DN_DEPTH 9
#define DN_HITS 10

// What a pixel carries: u = demodulated radiance (the one thing the passes change), z = mean depth over the hits,
// n = mean first-hit normal (not renormalised), d = the albedo the radiance was divided by, e = first-hit emission.
typedef struct DnPixel {
    float u[3], z, n[3], d[3], e[3];
} DnPixel;

// the à-trous kernel {1/16, 1/4, 3/8, 1/4, 1/16}: every product of two of them is exact
RT_HD float dn_kernel(int t /* -2 .. 2 */) {
    const int a = t < 0 ? -t : t;
    return a == 0 ? 0.375f : (a == 1 ? 0.25f : 0.0625f);
}

RT_HD float dn_fixed_to_float(int64_t sum) { return (float)((double)sum * (1.0 / 1073741824.0)); }

// Steps 1 and 2: the pixel of its beauty sums (3) and AOV sums (11).  inv_spp = 1.f / num_samples, inv_aov = 1.f / aov_samples.
RT_HD void dn_prepare(const int64_t *sum3, const int64_t *aov11, float inv_spp, float inv_aov, DnPixel *px) {
    const int64_t hits = aov11[DN_HITS];
    px->z = hits > 0 ? dn_fixed_to_float(aov11[DN_DEPTH]) / (float)hits : 0.f;
    for (int k = 0; k < 3; k++) {
        const float c = dn_fixed_to_float(sum3[k]) * inv_spp;
        const float a = dn_fixed_to_float(aov11[DN_ALBEDO + k]) * inv_aov;
        px->n[k] = dn_fixed_to_float(aov11[DN_NORMAL + k]) * inv_aov;
        px->e[k] = dn_fixed_to_float(aov11[DN_EMISSION + k]) * inv_aov;
        px->d[k] = a > 0.0009765625f ? a : 0.0009765625f;
        const float t = c - px->e[k];
        px->u[k] = (t > 0.f ? t : 0.f) / px->d[k];
    }
}

// Step 3, one tap that is not the centre: w = (h * rt_expnegf(-(x_c + x_z))) * w_n.
RT_HD float dn_tap_weight(float h, const float *up, float zp, const float *np, const float *uq, float zq, const float *nq, float kc,
                          float kz, int normal_power_log2) {
    const float dx = uq[0] - up[0], dy = uq[1] - up[1], dz = uq[2] - up[2];
    const float xc = ((dx * dx + dy * dy) + dz * dz) * kc;
    const float dd = zq - zp;
    const float xz = (dd * dd) * kz;
    const float ex = rt_expnegf(-(xc + xz));
    const float dot = (np[0] * nq[0] + np[1] * nq[1]) + np[2] * nq[2];
    float wn = dot > 0.f ? (dot < 1.f ? dot : 1.f) : 0.f;  // (at most 1: no weight exceeds h, nothing overflows, no NaN can arise)
    for (int k = 0; k < normal_power_log2; k++) wn = wn * wn;
    return (h * ex) * wn;
}

// Step 4: out = u * d + e, two operations per channel.
RT_HD void dn_finish(const float *u, const float *d, const float *e, float *out3) {
    for (int k = 0; k < 3; k++) out3[k] = u[k] * d[k] + e[k];
}

// ---- rt_denoise_dual_fixed (include/rtcuda_amd.h): two half frames, a variance channel v next to u, a colour stop measured in
// standard deviations of the local estimate.  Shared by the kernels k_*_dual / k_atrous_var* and the CPU twin hc_denoise_dual.
// Both keep {u.x, u.y, u.z, v} as four consecutive floats per pixel, which is what dn_var_blur indexes.
#define DN_VAR_EPS 1.4901161193847656e-08f  // 2^-26

// Steps 1 and 2: the pixel of the wrapped sum S = A + B (exactly dn_prepare's for (S, n)) and the variance of the mean, from
// u_a and u_b formed like u with the same d and e.  inv_a = 1.f / samples_a, inv_b = 1.f / samples_b, inv_n = 1.f / n.
RT_HD float dn_prepare_dual(const int64_t *sum_a3, const int64_t *sum_b3, const int64_t *aov11, float inv_a, float inv_b, float inv_n,
                            float inv_aov, float kv, DnPixel *px) {
    int64_t s[3];
    for (int k = 0; k < 3; k++) s[k] = (int64_t)((uint64_t)sum_a3[k] + (uint64_t)sum_b3[k]);
    dn_prepare(s, aov11, inv_n, inv_aov, px);
    float sq[3];
    for (int k = 0; k < 3; k++) {
        const float ta = dn_fixed_to_float(sum_a3[k]) * inv_a - px->e[k];
        const float tb = dn_fixed_to_float(sum_b3[k]) * inv_b - px->e[k];
        const float ua = (ta > 0.f ? ta : 0.f) / px->d[k];
        const float ub = (tb > 0.f ? tb : 0.f) / px->d[k];
        const float df = ua - ub;
        sq[k] = df * df;
    }
    return ((sq[0] + sq[1]) + sq[2]) * kv;
}

// the 3 x 3 prefilter's kernel {1/4, 1/2, 1/4}: every product of two of them is exact
RT_HD float dn_var_blur_weight(int dx /* -1 .. 1 */, int dy) { return (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f); }

// Step 3, the prefilter: g of pixel (x, y) from the pass's input, taps at stride 1 whatever the pass's stride.
RT_HD float dn_var_blur(const float *uv /* 4 floats per pixel, v the fourth */, long long x, long long y, int width, int height) {
    float sg = 0.f, sk = 0.f;
    for (int dy = -1; dy <= 1; dy++) {
        const long long yy = y + dy;
        if (yy < 0 || yy >= height) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const long long xx = x + dx;
            if (xx < 0 || xx >= width) continue;
            const float k = dn_var_blur_weight(dx, dy);
            sg = sg + k * uv[4 * (yy * width + xx) + 3];
            sk = sk + k;
        }
    }
    return sg / sk;
}

// r = 1.f / (ks * g + 2^-26): what a pixel's colour distances are multiplied by.  One division per pixel.
RT_HD float dn_var_rcp(float ks, float g) { return 1.f / (ks * g + DN_VAR_EPS); }

// One tap that is not the centre is dn_tap_weight with the pixel's r in the place of the pass's kc -- x_v = (|du|^2) * r is the
// same three operations as x_c.

// ---- rt_denoise_variance_fixed (include/rtcuda_amd.h): rt_denoise_dual_fixed's passes on ONE frame and a variance the caller
// brings.  Shared by k_dn_prepare_var and the CPU twin hc_denoise_variance.
#define DN_VAR_MAX 154742504910672534362390528.f  // 2^87: above every v that dn_prepare_dual can form

// Steps 1 and 2: dn_prepare's pixel of (sum, n), and the caller's x made a legal v: a NaN or a negative x gives 0, the top is 2^87.
RT_HD float dn_prepare_var(const int64_t *sum3, const int64_t *aov11, float x, float inv_spp, float inv_aov, DnPixel *px) {
    dn_prepare(sum3, aov11, inv_spp, inv_aov, px);
    return x > 0.f ? (x < DN_VAR_MAX ? x : DN_VAR_MAX) : 0.f;
}

#endif  // RT_DENOISE_H
