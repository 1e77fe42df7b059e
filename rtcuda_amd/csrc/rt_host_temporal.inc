// ---- the temporal accumulator: two sets of defaults (two sweeps), one set of argument checks, one launch (kernels:
// rt_temporal_kernels.inc).  rt_temporal_accumulate_fixed is temporal_run with the newer features off (rtcuda_amd.hip).
rt_temporal_params temporal_defaults() {
    rt_temporal_params p{};
    p.max_history = 4;  // (the sweep of tools/temporal_quality.py: profiles/temporal_quality.json)
    p.alpha_min = 0.03125f;
    p.depth_tolerance = 0.03125f;
    p.normal_cos_min = 0.5f;
    p.flags = 0u;
    return p;
}

rt_temporal_moments_params temporal_moments_defaults() {
    rt_temporal_moments_params p{};
    p.max_history = 4;  // (the sweep of tools/temporal_moments_quality.py: profiles/temporal_moments_quality.json)
    p.alpha_min = 0.03125f;
    p.depth_tolerance = 0.03125f;
    p.normal_cos_min = 0.5f;
    p.emission_tolerance = 0.0625f;
    p.variance_min_history = 1;
    p.flags = 0u;
    return p;
}

// me: the entry point's name, the head of every message; kernel: its instantiation of the pixel body
int temporal_run(const std::string &me, void (*kernel)(TmMoments), const int64_t *d_sum_a, int samples_a, const int64_t *d_sum_b, int samples_b, const int64_t *d_aov,
                 int aov_samples, const float *d_motion, const int64_t *d_hist_a_in, const int64_t *d_hist_b_in, const int32_t *d_len_in,
                 const int64_t *d_prev_aov, int prev_aov_samples, const float *d_prev_motion, const float *d_moments_in, int width, int height,
                 const rt_temporal_moments_params *params, int64_t *d_hist_a_out, int64_t *d_hist_b_out, int32_t *d_len_out,
                 float *d_moments_out, float *d_variance_out, hipStream_t stream) {
    const rt_temporal_moments_params prm = params ? *params : temporal_moments_defaults();
    const char *null_arg = !d_sum_a ? "d_sum_a" : !d_aov ? "d_aov_fixed" : !d_motion ? "d_motion" : !d_hist_a_out ? "d_hist_a_out" : !d_len_out ? "d_len_out" : nullptr;
    if (null_arg) return fail(me + "null " + null_arg);
    if (width < 1 || height < 1) return fail(me + "width and height must be at least 1");
    if ((long long)width * height > kDnMaxPixels) return fail(me + "more than 715827882 pixels");
    const bool two = d_sum_b != nullptr, history = d_hist_a_in != nullptr, moments = d_moments_out != nullptr;
    if (samples_a < 1 || aov_samples < 1 || (two && samples_b < 1)) return fail(me + "samples_a, samples_b (with d_sum_b) and aov_samples must be at least 1");
    if (two != (d_hist_b_out != nullptr)) return fail(me + "d_sum_b and d_hist_b_out must be null together");
    if (!history && (d_hist_b_in || d_len_in || d_prev_aov)) return fail(me + "the history pointers (d_hist_a_in, d_len_in, d_prev_aov_fixed, and d_hist_b_in with d_sum_b) must be all null or all set");
    if (history && (!d_len_in || !d_prev_aov)) return fail(me + "the history pointers (d_hist_a_in, d_len_in, d_prev_aov_fixed, and d_hist_b_in with d_sum_b) must be all null or all set");
    if (history && two != (d_hist_b_in != nullptr)) return fail(me + "d_sum_b and d_hist_b_in must be null together when history is given");
    if (history && prev_aov_samples < 1) return fail(me + "prev_aov_samples must be at least 1");
    if (!history && (d_moments_in || d_prev_motion)) return fail(me + "d_moments_in and d_prev_motion may be set only when history is given");
    if (moments != (d_variance_out != nullptr)) return fail(me + "d_moments_out and d_variance_out must be null together");
    if (d_moments_in && !moments) return fail(me + "d_moments_in needs d_moments_out");
    if (moments && two && (long long)samples_a + samples_b > 0x7fffffffll) return fail(me + "samples_a + samples_b must fit an int32");
    if ((uintptr_t)d_motion % 16) return fail(me + "d_motion must be 16-byte aligned");
    if ((uintptr_t)d_prev_motion % 16) return fail(me + "d_prev_motion must be 16-byte aligned");
    if ((uintptr_t)d_moments_in % 16) return fail(me + "d_moments_in must be 16-byte aligned");
    if ((uintptr_t)d_moments_out % 16) return fail(me + "d_moments_out must be 16-byte aligned");
    if (prm.flags) return fail(me + "flags must be 0");
    if (prm.max_history < 1) return fail(me + "max_history must be at least 1, it is " + std::to_string(prm.max_history));
    if (!(prm.alpha_min > 0.f && prm.alpha_min <= 1.f)) return fail(me + "alpha_min must be in (0, 1]");
    if (!(std::isfinite(prm.depth_tolerance) && prm.depth_tolerance > 0.f)) return fail(me + "depth_tolerance must be finite and positive");
    if (!(prm.normal_cos_min >= -1.f && prm.normal_cos_min <= 1.f)) return fail(me + "normal_cos_min must be in [-1, 1]");
    if (!(prm.emission_tolerance >= 0.f)) return fail(me + "emission_tolerance must be at least 0 (+inf passes every tap)");
    if (prm.variance_min_history < 1) return fail(me + "variance_min_history must be at least 1, it is " + std::to_string(prm.variance_min_history));
    const long long blocks = dn_pass_blocks(width, height, 1, 1);
    if (blocks > kDnMaxBlocks)
        return fail(me + "a " + std::to_string(width) + " x " + std::to_string(height) + " frame needs more than 16777215 workgroups (a frame this narrow or this flat is not served)");
    // no output range may touch an input range (or another output): the caller ping-pongs
    const long long n = (long long)width * height;
    struct Range {
        const char *name;
        uintptr_t lo, hi;
    };
    auto range = [&](const char *name, const void *p, long long bytes) { return Range{name, (uintptr_t)p, p ? (uintptr_t)p + (uintptr_t)bytes : (uintptr_t)p}; };
    constexpr int kOuts = 5, kIns = 10;
    const Range outs[kOuts] = {range("d_hist_a_out", d_hist_a_out, 24 * n), range("d_hist_b_out", d_hist_b_out, 24 * n), range("d_len_out", d_len_out, 4 * n),
                               range("d_moments_out", d_moments_out, 16 * n), range("d_variance_out", d_variance_out, 4 * n)};
    const Range ins[kIns] = {range("d_sum_a", d_sum_a, 24 * n), range("d_sum_b", d_sum_b, 24 * n), range("d_aov_fixed", d_aov, 8 * RT_AOV_CHANNELS * n),
                             range("d_motion", d_motion, 16 * n), range("d_hist_a_in", d_hist_a_in, 24 * n), range("d_hist_b_in", d_hist_b_in, 24 * n),
                             range("d_len_in", d_len_in, 4 * n), range("d_prev_aov_fixed", d_prev_aov, 8 * RT_AOV_CHANNELS * n),
                             range("d_prev_motion", d_prev_motion, 16 * n), range("d_moments_in", d_moments_in, 16 * n)};
    for (int o = 0; o < kOuts; o++) {
        if (outs[o].lo == outs[o].hi) continue;
        for (int i = 0; i < kIns; i++)
            if (ins[i].lo < outs[o].hi && outs[o].lo < ins[i].hi) return fail(me + outs[o].name + " overlaps " + ins[i].name);
        for (int i = o + 1; i < kOuts; i++)
            if (outs[i].lo < outs[o].hi && outs[o].lo < outs[i].hi) return fail(me + outs[o].name + " overlaps " + outs[i].name);
    }

    TmMoments tm{};
    tm_moments_fill(&tm, d_sum_a, samples_a, d_sum_b, samples_b, d_aov, aov_samples, d_motion, d_hist_a_in, d_hist_b_in, d_len_in, d_prev_aov,
                    prev_aov_samples, d_prev_motion, d_moments_in, width, height, (width + kDnTileW - 1) / kDnTileW, prm.max_history,
                    prm.alpha_min, prm.depth_tolerance, prm.normal_cos_min, prm.emission_tolerance, prm.variance_min_history, d_hist_a_out,
                    d_hist_b_out, d_len_out, d_moments_out, d_variance_out);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, tm);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}
