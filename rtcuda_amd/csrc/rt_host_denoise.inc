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
int dn_pass_form(int width, int height, int stride) {
    int want = dn_lds_wins(stride) ? 2 : 1;
    if (const char *k = knob("RT_DENOISE_FORM")) want = atoi(k) == 2 ? 2 : atoi(k) == 1 ? 1 : want;
    if (dn_pass_blocks(width, height, stride, want) <= kDnMaxBlocks) return want;
    return dn_pass_blocks(width, height, stride, 3 - want) <= kDnMaxBlocks ? 3 - want : 0;
}
void dn_launch_pass(int form, const float4 *src, const float4 *nrm, float4 *dst, int width, int height, int stride, float kc, float kz,
                    int normal_power_log2, hipStream_t stream) {
    const unsigned blocks = (unsigned)dn_pass_blocks(width, height, stride, form);
    if (form == 1) {
        hipLaunchKernelGGL(k_atrous, dim3(blocks), dim3(kBlock), 0, stream, src, nrm, dst, width, height, (width + kDnTileW - 1) / kDnTileW,
                           stride, kc, kz, normal_power_log2);
    } else {
        const int n_rx = std::min(stride, width), n_res = n_rx * std::min(stride, height);
        const int sub_w = (width + stride - 1) / stride;
        hipLaunchKernelGGL(k_atrous_lds, dim3(blocks), dim3(kBlock), 0, stream, src, nrm, dst, width, height, stride, n_rx, n_res,
                           (sub_w + kDnTileW - 1) / kDnTileW, kc, kz, normal_power_log2);
    }
}

int denoise_impl(const int64_t *d_sum_fixed, int num_samples, const int64_t *d_aov_fixed, int aov_samples, int width, int height,
                 const rt_denoise_params *params, void *d_scratch, float *d_rgb_out, hipStream_t stream) {
    const char *null_arg = !d_sum_fixed ? "d_sum_fixed" : !d_aov_fixed ? "d_aov_fixed" : !d_scratch ? "d_scratch" : !d_rgb_out ? "d_rgb_out" : nullptr;
    if (null_arg) return fail(std::string("rt_denoise_fixed: null ") + null_arg);
    if (width < 1 || height < 1) return fail("rt_denoise_fixed: width and height must be at least 1");
    if ((long long)width * height > kDnMaxPixels) return fail("rt_denoise_fixed: more than 715827882 pixels");
    if (num_samples < 1 || aov_samples < 1) return fail("rt_denoise_fixed: num_samples and aov_samples must be at least 1");
    if ((uintptr_t)d_scratch % kDnRecordBytes) return fail("rt_denoise_fixed: d_scratch must be 16-byte aligned");
    const rt_denoise_params prm = params ? *params : denoise_defaults();
    if (prm.flags) return fail("rt_denoise_fixed: flags must be 0");
    if (prm.passes < 0 || prm.passes > DN_MAX_PASSES) return fail("rt_denoise_fixed: passes must be 0 .. 8, it is " + std::to_string(prm.passes));
    if (prm.normal_power_log2 < 0 || prm.normal_power_log2 > DN_MAX_NORMAL_POWER_LOG2)
        return fail("rt_denoise_fixed: normal_power_log2 must be 0 .. 8, it is " + std::to_string(prm.normal_power_log2));
    if (!(std::isfinite(prm.sigma_color) && prm.sigma_color > 0.f)) return fail("rt_denoise_fixed: sigma_color must be finite and positive");
    if (!(std::isfinite(prm.sigma_depth) && prm.sigma_depth > 0.f)) return fail("rt_denoise_fixed: sigma_depth must be finite and positive");
    // the constants of the passes, each one rounded fp32 operation: kc_i = float(4^i) / (sigma_color * sigma_color),
    // kz = 1.f / (sigma_depth * sigma_depth)
    const float sc2 = prm.sigma_color * prm.sigma_color, sd2 = prm.sigma_depth * prm.sigma_depth;
    const float kz = 1.f / sd2;
    float kc[DN_MAX_PASSES];
    for (int i = 0; i < prm.passes; i++) {
        kc[i] = (float)(1 << (2 * i)) / sc2;
        if (!(std::isfinite(kc[i]) && kc[i] > 0.f))
            return fail("rt_denoise_fixed: sigma_color gives a colour constant that is not finite and positive in pass " + std::to_string(i));
    }
    if (!(std::isfinite(kz) && kz > 0.f)) return fail("rt_denoise_fixed: sigma_depth gives a depth constant that is not finite and positive");

    int form[DN_MAX_PASSES];
    for (int i = 0; i < prm.passes; i++)
        if (!(form[i] = dn_pass_form(width, height, 1 << i)))
            return fail("rt_denoise_fixed: a " + std::to_string(width) + " x " + std::to_string(height) + " frame needs more than 16777215 workgroups in the pass of stride " +
                        std::to_string(1 << i) + " (a frame this narrow or this flat is not served)");

    const long long n = (long long)width * height;
    float4 *buf[2] = {(float4 *)d_scratch, (float4 *)d_scratch + n};
    float4 *nrm = (float4 *)d_scratch + 2 * n;
    const float inv_spp = 1.f / (float)num_samples, inv_aov = 1.f / (float)aov_samples;
    const unsigned flat_blocks = (unsigned)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_dn_prepare, dim3(flat_blocks), dim3(kBlock), 0, stream, (const long long *)d_sum_fixed,
                       (const long long *)d_aov_fixed, n, inv_spp, inv_aov, buf[0], nrm);
    HIP_TRY(hipGetLastError());
    int at = 0;
    for (int i = 0; i < prm.passes; i++, at ^= 1) {
        dn_launch_pass(form[i], buf[at], nrm, buf[at ^ 1], width, height, 1 << i, kc[i], kz, prm.normal_power_log2, stream);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_dn_finish, dim3(flat_blocks), dim3(kBlock), 0, stream, buf[at], (const long long *)d_sum_fixed,
                       (const long long *)d_aov_fixed, n, inv_spp, inv_aov, d_rgb_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
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

// Which form and which placement of the variance prefilter win at a stride (profiles/denoise_dual_time.json, `pass_kernel_ms`,
// 1920 x 1080 on an MI355X; the prepass placement is timed with its k_dn_var_blur launch).  In the pass wherever its nine loads
// are cheap -- the direct form, and the LDS form at stride 1, where the staging has just touched the same lines; the LDS form at stride 2 runs
// after k_dn_var_blur and still beats the direct form; from stride 4 on the direct form wins.  RT_DENOISE_FORM = 1 / 2 forces
// the form as it does for rt_denoise_fixed, RT_DENOISE_DUAL_G = 1 (in the pass) / 2 (k_dn_var_blur before it) the placement.
bool dn_dual_lds_wins(int stride) { return stride <= 2; }
bool dn_dual_inline_g_wins(int form, int stride) { return form == 1 || stride == 1; }
int dn_dual_pass_form(int width, int height, int stride) {
    int want = dn_dual_lds_wins(stride) ? 2 : 1;
    if (const char *k = knob("RT_DENOISE_FORM")) want = atoi(k) == 2 ? 2 : atoi(k) == 1 ? 1 : want;
    if (dn_pass_blocks(width, height, stride, want) <= kDnMaxBlocks) return want;
    return dn_pass_blocks(width, height, stride, 3 - want) <= kDnMaxBlocks ? 3 - want : 0;
}
bool dn_dual_pass_inline_g(int form, int stride) {
    if (const char *k = knob("RT_DENOISE_DUAL_G"))
        if (atoi(k) == 1 || atoi(k) == 2) return atoi(k) == 1;
    return dn_dual_inline_g_wins(form, stride);
}
void dn_launch_dual_pass(int form, bool inline_g, const float4 *src, const float4 *nz, float *r_buf, float4 *dst, int width, int height,
                         int stride, float ks, float kz, int normal_power_log2, hipStream_t stream) {
    const unsigned blocks = (unsigned)dn_pass_blocks(width, height, stride, form);
    const long long n = (long long)width * height;
    if (!inline_g)
        hipLaunchKernelGGL(k_dn_var_blur, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, src, r_buf, width, height, n, ks);
    if (form == 1) {
        const int tiles_x = (width + kDnTileW - 1) / kDnTileW;
        if (inline_g)
            hipLaunchKernelGGL(k_atrous_var<true>, dim3(blocks), dim3(kBlock), 0, stream, src, nz, (const float *)r_buf, dst, width, height,
                               tiles_x, stride, ks, kz, normal_power_log2);
        else
            hipLaunchKernelGGL(k_atrous_var<false>, dim3(blocks), dim3(kBlock), 0, stream, src, nz, (const float *)r_buf, dst, width, height,
                               tiles_x, stride, ks, kz, normal_power_log2);
    } else {
        const int n_rx = std::min(stride, width), n_res = n_rx * std::min(stride, height);
        const int lat_tiles_x = ((width + stride - 1) / stride + kDnTileW - 1) / kDnTileW;
        if (inline_g)
            hipLaunchKernelGGL(k_atrous_var_lds<true>, dim3(blocks), dim3(kBlock), 0, stream, src, nz, (const float *)r_buf, dst, width,
                               height, stride, n_rx, n_res, lat_tiles_x, ks, kz, normal_power_log2);
        else
            hipLaunchKernelGGL(k_atrous_var_lds<false>, dim3(blocks), dim3(kBlock), 0, stream, src, nz, (const float *)r_buf, dst, width,
                               height, stride, n_rx, n_res, lat_tiles_x, ks, kz, normal_power_log2);
    }
}

int denoise_dual_impl(const int64_t *d_sum_a, int samples_a, const int64_t *d_sum_b, int samples_b, const int64_t *d_aov_fixed,
                      int aov_samples, int width, int height, const rt_denoise_dual_params *params, void *d_scratch, float *d_rgb_out,
                      hipStream_t stream) {
    const std::string me = "rt_denoise_dual_fixed: ";
    const char *null_arg = !d_sum_a ? "d_sum_a" : !d_sum_b ? "d_sum_b" : !d_aov_fixed ? "d_aov_fixed" : !d_scratch ? "d_scratch" : !d_rgb_out ? "d_rgb_out" : nullptr;
    if (null_arg) return fail(me + "null " + null_arg);
    if (width < 1 || height < 1) return fail(me + "width and height must be at least 1");
    if ((long long)width * height > kDnMaxPixels) return fail(me + "more than 715827882 pixels");
    if (samples_a < 1 || samples_b < 1 || aov_samples < 1) return fail(me + "samples_a, samples_b and aov_samples must be at least 1");
    if ((long long)samples_a + samples_b > 0x7fffffffll) return fail(me + "samples_a + samples_b must fit an int32");
    if ((uintptr_t)d_scratch % kDnRecordBytes) return fail(me + "d_scratch must be 16-byte aligned");
    const rt_denoise_dual_params prm = params ? *params : denoise_dual_defaults();
    if (prm.flags) return fail(me + "flags must be 0");
    if (prm.passes < 0 || prm.passes > DN_MAX_PASSES) return fail(me + "passes must be 0 .. 8, it is " + std::to_string(prm.passes));
    if (prm.normal_power_log2 < 0 || prm.normal_power_log2 > DN_MAX_NORMAL_POWER_LOG2)
        return fail(me + "normal_power_log2 must be 0 .. 8, it is " + std::to_string(prm.normal_power_log2));
    if (!(std::isfinite(prm.sigma_variance) && prm.sigma_variance > 0.f)) return fail(me + "sigma_variance must be finite and positive");
    if (!(std::isfinite(prm.sigma_depth) && prm.sigma_depth > 0.f)) return fail(me + "sigma_depth must be finite and positive");
    // the constants, each one rounded fp32 operation: ks = sigma_variance * sigma_variance, kz = 1.f / (sigma_depth * sigma_depth);
    // kv = float(double(samples_a) * samples_b / (double(n) * n))
    const float ks = prm.sigma_variance * prm.sigma_variance, sd2 = prm.sigma_depth * prm.sigma_depth;
    const float kz = 1.f / sd2;
    if (!(std::isfinite(ks) && ks > 0.f)) return fail(me + "sigma_variance gives a variance constant that is not finite and positive");
    if (!(std::isfinite(kz) && kz > 0.f)) return fail(me + "sigma_depth gives a depth constant that is not finite and positive");
    const int n_samples = samples_a + samples_b;
    const float kv = (float)((double)samples_a * (double)samples_b / ((double)n_samples * (double)n_samples));

    int form[DN_MAX_PASSES];
    for (int i = 0; i < prm.passes; i++)
        if (!(form[i] = dn_dual_pass_form(width, height, 1 << i)))
            return fail(me + "a " + std::to_string(width) + " x " + std::to_string(height) + " frame needs more than 16777215 workgroups in the pass of stride " +
                        std::to_string(1 << i) + " (a frame this narrow or this flat is not served)");

    const long long n = (long long)width * height;
    float4 *buf[2] = {(float4 *)d_scratch, (float4 *)d_scratch + n};
    float4 *nz = (float4 *)d_scratch + 2 * n;
    float *r_buf = (float *)((float4 *)d_scratch + 3 * n);
    const float inv_a = 1.f / (float)samples_a, inv_b = 1.f / (float)samples_b, inv_n = 1.f / (float)n_samples, inv_aov = 1.f / (float)aov_samples;
    const unsigned flat_blocks = (unsigned)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_dn_prepare_dual, dim3(flat_blocks), dim3(kBlock), 0, stream, (const long long *)d_sum_a, (const long long *)d_sum_b,
                       (const long long *)d_aov_fixed, n, inv_a, inv_b, inv_n, inv_aov, kv, buf[0], nz);
    HIP_TRY(hipGetLastError());
    int at = 0;
    for (int i = 0; i < prm.passes; i++, at ^= 1) {
        dn_launch_dual_pass(form[i], dn_dual_pass_inline_g(form[i], 1 << i), buf[at], nz, r_buf, buf[at ^ 1], width, height, 1 << i, ks, kz,
                            prm.normal_power_log2, stream);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_dn_finish_dual, dim3(flat_blocks), dim3(kBlock), 0, stream, buf[at], (const long long *)d_sum_a,
                       (const long long *)d_sum_b, (const long long *)d_aov_fixed, n, inv_n, inv_aov, d_rgb_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}
