// ---- rt_denoise_fixed: argument checks, the constants of the passes, the launches (kernels: rt_denoise_kernels.inc)
constexpr int kDnRecordBytes = 16, kDnRecords = 3;  // per pixel: {u, z} twice, {n} once
constexpr long long kDnMaxPixels = 0x7fffffff / 3;  // the pixel limit of the AOV entry points

rt_denoise_params denoise_defaults() {
    rt_denoise_params p{};
    p.passes = 2;  // (the sweep of tools/denoise_quality.py: profiles/denoise_quality.json)
    p.sigma_color = 0.125f;
    p.sigma_depth = 0.5f;
    p.normal_power_log2 = 1;
    p.flags = 0u;
    return p;
}

long long denoise_scratch_bytes(int width, int height) {
    if (width < 1 || height < 1 || (long long)width * height > kDnMaxPixels) return -1;
    return (long long)width * height * (kDnRecordBytes * kDnRecords);
}

// One pass.  form: 1 = k_atrous (direct), 2 = k_atrous_lds.  The grids are one-dimensional; a HIP launch holds fewer than 2^32
// threads, so a pass has at most kDnMaxBlocks workgroups: dn_pass_blocks says how many a form needs (frames of a few pixels'
// width or height are the ones that can exceed it: their tiles are mostly empty).
constexpr long long kDnMaxBlocks = (1ll << 24) - 1;
long long dn_pass_blocks(int width, int height, int stride, int form) {
    if (form == 1) return (long long)((width + kDnTileW - 1) / kDnTileW) * ((height + kDnTileH - 1) / kDnTileH);
    const long long n_res = (long long)std::min(stride, width) * std::min(stride, height);
    const long long sub_w = (width + stride - 1) / stride, sub_h = (height + stride - 1) / stride;
    return n_res * ((sub_w + kDnTileW - 1) / kDnTileW) * ((sub_h + kDnTileH - 1) / kDnTileH);
}
// Which form wins at a stride (profiles/denoise_time.json, `pass_kernel_ms`, 1920 x 1080 on an MI355X); the other form where the
// winner's grid would be too large.  RT_DENOISE_FORM = 1 / 2 (an experiment knob: RTCUDA_EXPERIMENTAL=1) forces a form wherever
// its grid fits -- how the tests run every form at every stride.
bool dn_lds_wins(int stride) { return stride <= 4; }
int dn_pass_form(int width, int height, int stride, bool lds_wins) {
    int want = lds_wins ? 2 : 1;
    if (const char *k = knob("RT_DENOISE_FORM")) want = atoi(k) == 2 ? 2 : atoi(k) == 1 ? 1 : want;
    if (dn_pass_blocks(width, height, stride, want) <= kDnMaxBlocks) return want;
    return dn_pass_blocks(width, height, stride, 3 - want) <= kDnMaxBlocks ? 3 - want : 0;
}
// Which form and which placement of the variance prefilter win at a stride (profiles/denoise_dual_time.json, `pass_kernel_ms`,
// 1920 x 1080 on an MI355X; the prepass placement is timed with its k_dn_var_blur launch).  In the pass wherever its nine loads
// are cheap -- the direct form, and the LDS form at stride 1, where the staging has just touched the same lines; the LDS form at stride 2 runs
// after k_dn_var_blur and still beats the direct form; from stride 4 on the direct form wins.  RT_DENOISE_FORM = 1 / 2 forces
// the form as it does for rt_denoise_fixed, RT_DENOISE_DUAL_G = 1 (in the pass) / 2 (k_dn_var_blur before it) the placement.
bool dn_dual_lds_wins(int stride) { return stride <= 2; }
bool dn_dual_inline_g_wins(int form, int stride) { return form == 1 || stride == 1; }
int dn_dual_pass_g(int form, int stride) {
    if (const char *k = knob("RT_DENOISE_DUAL_G"))
        if (atoi(k) == 1 || atoi(k) == 2) return atoi(k);
    return dn_dual_inline_g_wins(form, stride) ? 1 : 2;
}
// One pass of either filter.  g: 0 = rt_denoise_fixed (k is the pass's kc, no r_buf), 1 / 2 = rt_denoise_dual_fixed (k is ks) with
// r formed in the pass / by k_dn_var_blur before it.
void dn_launch_pass(int form, int g, const float4 *src, const float4 *nrm, float *r_buf, float4 *dst, int width, int height, int stride,
                    float k, float kz, int normal_power_log2, hipStream_t stream) {
    const dim3 grid((unsigned)dn_pass_blocks(width, height, stride, form)), block(kBlock);
    const float *r_in = r_buf;
    if (g == 2) {
        const long long n = (long long)width * height;
        hipLaunchKernelGGL(k_dn_var_blur, dim3((unsigned)((n + kBlock - 1) / kBlock)), block, 0, stream, src, r_buf, width, height, n, k);
    }
    if (form == 1) {
        const int tiles_x = (width + kDnTileW - 1) / kDnTileW;
        if (g == 0)
            hipLaunchKernelGGL(k_atrous, grid, block, 0, stream, src, nrm, dst, width, height, tiles_x, stride, k, kz, normal_power_log2);
        else
            hipLaunchKernelGGL(g == 1 ? k_atrous_var<true> : k_atrous_var<false>, grid, block, 0, stream, src, nrm, r_in, dst, width, height,
                               tiles_x, stride, k, kz, normal_power_log2);
    } else {
        const int n_rx = std::min(stride, width), n_res = n_rx * std::min(stride, height);
        const int lat_tiles_x = ((width + stride - 1) / stride + kDnTileW - 1) / kDnTileW;
        if (g == 0)
            hipLaunchKernelGGL(k_atrous_lds, grid, block, 0, stream, src, nrm, dst, width, height, stride, n_rx, n_res, lat_tiles_x, k, kz,
                               normal_power_log2);
        else
            hipLaunchKernelGGL(g == 1 ? k_atrous_var_lds<true> : k_atrous_var_lds<false>, grid, block, 0, stream, src, nrm, r_in, dst, width,
                               height, stride, n_rx, n_res, lat_tiles_x, k, kz, normal_power_log2);
    }
}

// The argument checks both entry points make, in the order they fire.  me: the entry point's prefix; null_arg, samples_fault:
// what the caller found wrong with its own pointers and sample counts (null: nothing); sigma_name, sigma: its colour stop.
int dn_check(const std::string &me, const char *null_arg, int width, int height, const char *samples_fault, const void *d_scratch,
             unsigned flags, int passes, int normal_power_log2, const char *sigma_name, float sigma, float sigma_depth) {
    if (null_arg) return fail(me + "null " + null_arg);
    if (width < 1 || height < 1) return fail(me + "width and height must be at least 1");
    if ((long long)width * height > kDnMaxPixels) return fail(me + "more than 715827882 pixels");
    if (samples_fault) return fail(me + samples_fault);
    if ((uintptr_t)d_scratch % kDnRecordBytes) return fail(me + "d_scratch must be 16-byte aligned");
    if (flags) return fail(me + "flags must be 0");
    if (passes < 0 || passes > DN_MAX_PASSES) return fail(me + "passes must be 0 .. 8, it is " + std::to_string(passes));
    if (normal_power_log2 < 0 || normal_power_log2 > DN_MAX_NORMAL_POWER_LOG2)
        return fail(me + "normal_power_log2 must be 0 .. 8, it is " + std::to_string(normal_power_log2));
    if (!(std::isfinite(sigma) && sigma > 0.f)) return fail(me + sigma_name + " must be finite and positive");
    if (!(std::isfinite(sigma_depth) && sigma_depth > 0.f)) return fail(me + "sigma_depth must be finite and positive");
    return 0;
}

// prepare -> passes -> finish -> synchronise, for both filters.  var: the scratch has the r array behind its three record arrays
// and the passes carry v.  k[i]: pass i's kc, or ks.  kz = 1.f / (sigma_depth * sigma_depth), two rounded fp32 operations.
// prepare(blocks, n, first record array, third record array) and finish(blocks, n, the array the last pass wrote) launch the
// caller's own kernels over the n pixels.
template <typename Prepare, typename Finish>
int dn_run(const std::string &me, bool var, int width, int height, int passes, const float *k, float sigma_depth, int normal_power_log2,
           void *d_scratch, hipStream_t stream, Prepare prepare, Finish finish) {
    const float sd2 = sigma_depth * sigma_depth;
    const float kz = 1.f / sd2;
    if (!(std::isfinite(kz) && kz > 0.f)) return fail(me + "sigma_depth gives a depth constant that is not finite and positive");
    int form[DN_MAX_PASSES];
    for (int i = 0; i < passes; i++)
        if (!(form[i] = dn_pass_form(width, height, 1 << i, var ? dn_dual_lds_wins(1 << i) : dn_lds_wins(1 << i))))
            return fail(me + "a " + std::to_string(width) + " x " + std::to_string(height) + " frame needs more than 16777215 workgroups in the pass of stride " +
                        std::to_string(1 << i) + " (a frame this narrow or this flat is not served)");

    const long long n = (long long)width * height;
    float4 *buf[2] = {(float4 *)d_scratch, (float4 *)d_scratch + n};
    float4 *nrm = (float4 *)d_scratch + 2 * n;
    float *r_buf = var ? (float *)((float4 *)d_scratch + 3 * n) : nullptr;
    const unsigned flat_blocks = (unsigned)((n + kBlock - 1) / kBlock);
    prepare(flat_blocks, n, buf[0], nrm);
    HIP_TRY(hipGetLastError());
    int at = 0;
    for (int i = 0; i < passes; i++, at ^= 1) {
        dn_launch_pass(form[i], var ? dn_dual_pass_g(form[i], 1 << i) : 0, buf[at], nrm, r_buf, buf[at ^ 1], width, height, 1 << i, k[i], kz,
                       normal_power_log2, stream);
        HIP_TRY(hipGetLastError());
    }
    finish(flat_blocks, n, buf[at]);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

int denoise_impl(const int64_t *d_sum_fixed, int num_samples, const int64_t *d_aov_fixed, int aov_samples, int width, int height,
                 const rt_denoise_params *params, void *d_scratch, float *d_rgb_out, hipStream_t stream) {
    const std::string me = "rt_denoise_fixed: ";
    const rt_denoise_params prm = params ? *params : denoise_defaults();
    if (dn_check(me, !d_sum_fixed ? "d_sum_fixed" : !d_aov_fixed ? "d_aov_fixed" : !d_scratch ? "d_scratch" : !d_rgb_out ? "d_rgb_out" : nullptr,
                 width, height, num_samples < 1 || aov_samples < 1 ? "num_samples and aov_samples must be at least 1" : nullptr, d_scratch,
                 prm.flags, prm.passes, prm.normal_power_log2, "sigma_color", prm.sigma_color, prm.sigma_depth))
        return 1;
    // the colour constants of the passes, each one rounded fp32 operation: kc_i = float(4^i) / (sigma_color * sigma_color)
    const float sc2 = prm.sigma_color * prm.sigma_color;
    float kc[DN_MAX_PASSES];
    for (int i = 0; i < prm.passes; i++) {
        kc[i] = (float)(1 << (2 * i)) / sc2;
        if (!(std::isfinite(kc[i]) && kc[i] > 0.f))
            return fail(me + "sigma_color gives a colour constant that is not finite and positive in pass " + std::to_string(i));
    }
    const float inv_spp = 1.f / (float)num_samples, inv_aov = 1.f / (float)aov_samples;
    return dn_run(
        me, false, width, height, prm.passes, kc, prm.sigma_depth, prm.normal_power_log2, d_scratch, stream,
        [&](unsigned blocks, long long n, float4 *uz, float4 *nrm) {
            hipLaunchKernelGGL(k_dn_prepare, dim3(blocks), dim3(kBlock), 0, stream, (const long long *)d_sum_fixed,
                               (const long long *)d_aov_fixed, n, inv_spp, inv_aov, uz, nrm);
        },
        [&](unsigned blocks, long long n, const float4 *uz) {
            hipLaunchKernelGGL(k_dn_finish, dim3(blocks), dim3(kBlock), 0, stream, uz, (const long long *)d_sum_fixed,
                               (const long long *)d_aov_fixed, n, inv_spp, inv_aov, d_rgb_out);
        });
}

// ---- rt_denoise_dual_fixed: the same checks, grids and forms; per pass one more choice, where r comes from
constexpr int kDnDualBytesPerPixel = 3 * kDnRecordBytes + 4;  // {u, v} twice, {n, z} once, r once

rt_denoise_dual_params denoise_dual_defaults() {
    rt_denoise_dual_params p{};
    p.passes = 3;  // (the sweep of tools/denoise_dual_quality.py: profiles/denoise_dual_quality.json)
    p.sigma_variance = 4.f;
    p.sigma_depth = 0.03125f;
    p.normal_power_log2 = 5;
    p.flags = 0u;
    return p;
}

long long denoise_dual_scratch_bytes(int width, int height) {
    if (width < 1 || height < 1 || (long long)width * height > kDnMaxPixels) return -1;
    return (long long)width * height * kDnDualBytesPerPixel;
}

int denoise_dual_impl(const int64_t *d_sum_a, int samples_a, const int64_t *d_sum_b, int samples_b, const int64_t *d_aov_fixed,
                      int aov_samples, int width, int height, const rt_denoise_dual_params *params, void *d_scratch, float *d_rgb_out,
                      hipStream_t stream) {
    const std::string me = "rt_denoise_dual_fixed: ";
    const rt_denoise_dual_params prm = params ? *params : denoise_dual_defaults();
    if (dn_check(me, !d_sum_a ? "d_sum_a" : !d_sum_b ? "d_sum_b" : !d_aov_fixed ? "d_aov_fixed" : !d_scratch ? "d_scratch" : !d_rgb_out ? "d_rgb_out" : nullptr,
                 width, height,
                 samples_a < 1 || samples_b < 1 || aov_samples < 1 ? "samples_a, samples_b and aov_samples must be at least 1"
                 : (long long)samples_a + samples_b > 0x7fffffffll ? "samples_a + samples_b must fit an int32"
                                                                   : nullptr,
                 d_scratch, prm.flags, prm.passes, prm.normal_power_log2, "sigma_variance", prm.sigma_variance, prm.sigma_depth))
        return 1;
    // the constants, each one rounded fp32 operation: ks = sigma_variance * sigma_variance;
    // kv = float(double(samples_a) * samples_b / (double(n) * n))
    const float ks = prm.sigma_variance * prm.sigma_variance;
    if (!(std::isfinite(ks) && ks > 0.f)) return fail(me + "sigma_variance gives a variance constant that is not finite and positive");
    const float k[DN_MAX_PASSES] = {ks, ks, ks, ks, ks, ks, ks, ks};
    const int n_samples = samples_a + samples_b;
    const float kv = (float)((double)samples_a * (double)samples_b / ((double)n_samples * (double)n_samples));
    const float inv_a = 1.f / (float)samples_a, inv_b = 1.f / (float)samples_b, inv_n = 1.f / (float)n_samples, inv_aov = 1.f / (float)aov_samples;
    return dn_run(
        me, true, width, height, prm.passes, k, prm.sigma_depth, prm.normal_power_log2, d_scratch, stream,
        [&](unsigned blocks, long long n, float4 *uv, float4 *nz) {
            hipLaunchKernelGGL(k_dn_prepare_dual, dim3(blocks), dim3(kBlock), 0, stream, (const long long *)d_sum_a, (const long long *)d_sum_b,
                               (const long long *)d_aov_fixed, n, inv_a, inv_b, inv_n, inv_aov, kv, uv, nz);
        },
        [&](unsigned blocks, long long n, const float4 *uv) {
            hipLaunchKernelGGL(k_dn_finish_dual, dim3(blocks), dim3(kBlock), 0, stream, uv, (const long long *)d_sum_a,
                               (const long long *)d_sum_b, (const long long *)d_aov_fixed, n, inv_n, inv_aov, d_rgb_out);
        });
}

// ---- rt_denoise_variance_fixed: the dual filter's checks, scratch, forms and passes on one frame; v comes from the caller
int denoise_variance_impl(const int64_t *d_sum_fixed, int num_samples, const float *d_variance, const int64_t *d_aov_fixed, int aov_samples,
                          int width, int height, const rt_denoise_dual_params *params, void *d_scratch, float *d_rgb_out, hipStream_t stream) {
    const std::string me = "rt_denoise_variance_fixed: ";
    const rt_denoise_dual_params prm = params ? *params : denoise_dual_defaults();
    if (dn_check(me, !d_sum_fixed ? "d_sum_fixed" : !d_variance ? "d_variance" : !d_aov_fixed ? "d_aov_fixed" : !d_scratch ? "d_scratch" : !d_rgb_out ? "d_rgb_out" : nullptr,
                 width, height, num_samples < 1 || aov_samples < 1 ? "num_samples and aov_samples must be at least 1" : nullptr, d_scratch,
                 prm.flags, prm.passes, prm.normal_power_log2, "sigma_variance", prm.sigma_variance, prm.sigma_depth))
        return 1;
    const float ks = prm.sigma_variance * prm.sigma_variance;
    if (!(std::isfinite(ks) && ks > 0.f)) return fail(me + "sigma_variance gives a variance constant that is not finite and positive");
    const float k[DN_MAX_PASSES] = {ks, ks, ks, ks, ks, ks, ks, ks};
    const float inv_spp = 1.f / (float)num_samples, inv_aov = 1.f / (float)aov_samples;
    return dn_run(
        me, true, width, height, prm.passes, k, prm.sigma_depth, prm.normal_power_log2, d_scratch, stream,
        [&](unsigned blocks, long long n, float4 *uv, float4 *nz) {
            hipLaunchKernelGGL(k_dn_prepare_var, dim3(blocks), dim3(kBlock), 0, stream, (const long long *)d_sum_fixed, d_variance,
                               (const long long *)d_aov_fixed, n, inv_spp, inv_aov, uv, nz);
        },
        [&](unsigned blocks, long long n, const float4 *uv) {
            hipLaunchKernelGGL(k_dn_finish, dim3(blocks), dim3(kBlock), 0, stream, uv, (const long long *)d_sum_fixed,
                               (const long long *)d_aov_fixed, n, inv_spp, inv_aov, d_rgb_out);
        });
}

// ---- rt_upsample_fixed / rt_upsample_rgb: dn_check's checks, no scratch, no passes, one launch (kernel: rt_upsample_kernels.inc)
rt_upsample_params upsample_defaults() {
    rt_upsample_params p{};
    p.sigma_depth = 0.03125f;  // (the sweep of tools/upsample_quality.py: profiles/upsample_quality.json)
    p.normal_power_log2 = 5;
    p.flags = 0u;
    return p;
}

// low: d_sum_lo (rgb = false, num_samples its samples) or d_rgb_lo (rgb = true).  What of the sizes dn_check does not know --
// the factor, the low size, the full frame's pixel count -- is found first and handed to it in the place of the sample fault, so
// the order is: pointers, factor, sizes, samples, flags, normal_power_log2, sigma_depth.
int upsample_impl(const std::string &me, bool rgb, const void *low, const char *low_name, int num_samples, const int64_t *d_aov_lo,
                  int aov_samples_lo, int low_width, int low_height, int factor, const int64_t *d_aov_hi, int aov_samples_hi,
                  const rt_upsample_params *params, float *d_rgb_out, int64_t *d_out_fixed, hipStream_t stream) {
    const rt_upsample_params prm = params ? *params : upsample_defaults();
    const bool factor_ok = factor >= UP_MIN_FACTOR && factor <= UP_MAX_FACTOR, size_ok = low_width >= 1 && low_height >= 1;
    const char *fault = !factor_ok ? "factor must be 2, 3 or 4"
                        : !size_ok ? "low_width and low_height must be at least 1"
                        : (long long)low_width * low_height > kDnMaxPixels / ((long long)factor * factor) ? "more than 715827882 pixels in the full frame"
                        : num_samples < 1 || aov_samples_lo < 1 || aov_samples_hi < 1 ? (rgb ? "aov_samples_lo and aov_samples_hi must be at least 1"
                                                                                             : "num_samples, aov_samples_lo and aov_samples_hi must be at least 1")
                                                                                      : nullptr;
    if (dn_check(me, !low ? low_name : !d_aov_lo ? "d_aov_lo" : !d_aov_hi ? "d_aov_hi" : !d_rgb_out && !d_out_fixed ? "d_rgb_out and null d_out_fixed" : nullptr,
                 1, 1, fault, nullptr, prm.flags, 0, prm.normal_power_log2, "sigma_depth", prm.sigma_depth, prm.sigma_depth))
        return 1;
    const float sd2 = prm.sigma_depth * prm.sigma_depth;
    const float kz = 1.f / sd2;
    if (!(std::isfinite(kz) && kz > 0.f)) return fail(me + "sigma_depth gives a depth constant that is not finite and positive");
    const int width = factor * low_width, height = factor * low_height;
    const int tiles_x = (width + kDnTileW - 1) / kDnTileW;
    const long long blocks = dn_pass_blocks(width, height, 1, 1);
    if (blocks > kDnMaxBlocks)
        return fail(me + "a " + std::to_string(width) + " x " + std::to_string(height) +
                    " frame needs more than 16777215 workgroups (a frame this narrow or this flat is not served)");
    const float inv_spp = 1.f / (float)num_samples, inv_lo = 1.f / (float)aov_samples_lo, inv_hi = 1.f / (float)aov_samples_hi;
    using Kernel = void (*)(const void *, const long long *, const long long *, int, int, int, float, float, float, float, int, float *, long long *);
    static const Kernel kernels[2][UP_MAX_FACTOR - UP_MIN_FACTOR + 1] = {{k_upsample<2, false>, k_upsample<3, false>, k_upsample<4, false>},
                                                                          {k_upsample<2, true>, k_upsample<3, true>, k_upsample<4, true>}};
    hipLaunchKernelGGL(kernels[rgb][factor - UP_MIN_FACTOR], dim3((unsigned)blocks), dim3(kBlock), 0, stream, low, (const long long *)d_aov_lo,
                       (const long long *)d_aov_hi, low_width, low_height, tiles_x, inv_spp, inv_lo, inv_hi, kz, prm.normal_power_log2, d_rgb_out,
                       (long long *)d_out_fixed);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}
