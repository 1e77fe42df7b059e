// rt_upsample.h -- the per-pixel arithmetic of rt_upsample_fixed / rt_upsample_rgb (include/rtcuda_amd.h, DESIGN.md section
// 2.13), as a fixed sequence of individually rounded fp32 operations (no FMA: every translation unit that includes it is compiled
// with -ffp-contract=off).  The kernel (k_upsample: rt_upsample_kernels.inc) and the CPU twin (hc_upsample, rt_host_check.cpp)
// both call up_low_pixel for a low-resolution pixel and up_full_pixel for a full-resolution one, and differ only in who walks
// the pixels and where the low pixels' records live (`low` below: LDS there, an array here).
//
// Usable from g++ (host) and hipcc (device).
#ifndef RT_UPSAMPLE_H
#define RT_UPSAMPLE_H

#include <stdint.h>

#include "rt_denoise.h"   // dn_prepare, dn_tap_weight, dn_finish: the denoiser's text, used as it stands
#include "rt_temporal.h"  // tm_to_fixed

#define UP_MIN_FACTOR 2
#define UP_MAX_FACTOR 4
#define UP_LOW_FLOATS 7  // what a tap reads of a low pixel: u (3), z, n (3)

// which form a full pixel took (hc_upsample reports it; the kernel has no use for it)
#define UP_GUIDED 0    // step 5's first form: su / sw
#define UP_TENT 1      // step 5's second form: sb / sh, no low tap shares the pixel's features
#define UP_SHORTCUT 2  // step 2's shortcut: no sample hit the pixel

typedef struct UpLow {
    float u[3], z, n[3];
} UpLow;

// Step 1 for rt_upsample_rgb: a c that is NaN or infinite is 0.f (m <= FLT_MAX is false for both)
RT_HD float up_finite_or_zero(float c) {
    const float m = c < 0.f ? -c : c;
    return m <= 3.402823466e+38f ? c : 0.f;
}

// Step 1 for rt_upsample_fixed: low pixel q of its fixed-point sums -- dn_prepare itself
RT_HD void up_low_of_sums(const int64_t *sum3, const int64_t *aov11, float inv_spp, float inv_aov, UpLow *q) {
    DnPixel px;
    dn_prepare(sum3, aov11, inv_spp, inv_aov, &px);
    q->z = px.z;
    for (int k = 0; k < 3; k++) q->u[k] = px.u[k], q->n[k] = px.n[k];
}
// Step 1 for rt_upsample_rgb: c is the given float, made finite; everything after c is dn_prepare's text
RT_HD void up_low_of_rgb(const float *rgb3, const int64_t *aov11, float inv_aov, UpLow *q) {
    const int64_t hits = aov11[DN_HITS];
    q->z = hits > 0 ? dn_fixed_to_float(aov11[DN_DEPTH]) / (float)hits : 0.f;
    for (int k = 0; k < 3; k++) {
        const float c = up_finite_or_zero(rgb3[k]);
        const float a = dn_fixed_to_float(aov11[DN_ALBEDO + k]) * inv_aov;
        q->n[k] = dn_fixed_to_float(aov11[DN_NORMAL + k]) * inv_aov;
        const float e = dn_fixed_to_float(aov11[DN_EMISSION + k]) * inv_aov;
        const float d = a > 0.0009765625f ? a : 0.0009765625f;
        const float t = c - e;
        q->u[k] = (t > 0.f ? t : 0.f) / d;
    }
}

// Step 3, one axis: full coordinate x -> the low coordinate i0 of tap j = 0 and the fraction f in [0, 1).
// a = 2x + 1 - factor >= 1 - factor > -2 * factor, so the floor of a / (2 * factor) is -1 for every negative a.
RT_HD void up_position(int x, int factor, int *i0, float *f) {
    const int a = 2 * x + 1 - factor, m = 2 * factor;
    *i0 = a < 0 ? -1 : a / m;
    const int r = a - m * *i0;
    *f = (float)r / (float)m;
}

// Step 4, one axis: the tent of radius 2 at tap j = -1 .. 2
RT_HD float up_tent(int j, float f) {
    const float t = (float)j - f;
    return 1.f - 0.5f * (t < 0.f ? -t : t);
}

// Steps 2 to 6 for full pixel (x, y).  low(qx, qy, &q) hands back the record of low pixel (qx, qy), which is inside the low
// image.  Writes the three floats of out3; returns UP_GUIDED, UP_TENT or UP_SHORTCUT.
template <typename Low>
RT_HD int up_full_pixel(int x, int y, int factor, int low_width, int low_height, const int64_t *aov_hi11, float inv_aov_hi, float kz,
                        int normal_power_log2, Low low, float *out3) {
    const int64_t no_sum[3] = {0, 0, 0};
    DnPixel px;  // z, n, d, e of the full pixel (its u is not used: the pixel has no radiance of its own)
    dn_prepare(no_sum, aov_hi11, 1.f, inv_aov_hi, &px);
    float u[3] = {0.f, 0.f, 0.f};
    int form = UP_SHORTCUT;
    if (aov_hi11[DN_HITS] > 0) {
        int x0, y0;
        float fx, fy;
        up_position(x, factor, &x0, &fx);
        up_position(y, factor, &y0, &fy);
        float sw = 0.f, sh = 0.f, su[3] = {0.f, 0.f, 0.f}, sb[3] = {0.f, 0.f, 0.f};
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
        for (int jy = -1; jy <= 2; jy++) {
            const int qy = y0 + jy;
            if (qy < 0 || qy >= low_height) continue;
            const float ky = up_tent(jy, fy);
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
            for (int jx = -1; jx <= 2; jx++) {
                const int qx = x0 + jx;
                if (qx < 0 || qx >= low_width) continue;
                const float h = ky * up_tent(jx, fx);
                UpLow q;
                low(qx, qy, &q);
                const float w = dn_tap_weight(h, q.u, px.z, px.n, q.u, q.z, q.n, 0.f, kz, normal_power_log2);
                sw = sw + w;
                for (int k = 0; k < 3; k++) su[k] = su[k] + w * q.u[k];
                sh = sh + h;
                for (int k = 0; k < 3; k++) sb[k] = sb[k] + h * q.u[k];
            }
        }
        form = sw > 0.f ? UP_GUIDED : UP_TENT;
        for (int k = 0; k < 3; k++) u[k] = sw > 0.f ? su[k] / sw : sb[k] / sh;
    }
    dn_finish(u, px.d, px.e, out3);
    return form;
}

#endif  // RT_UPSAMPLE_H
