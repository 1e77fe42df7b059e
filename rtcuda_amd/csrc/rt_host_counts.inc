// What a counted frame (rt_render_counts_fixed, rt_host_render.inc) is used with: the per-pixel divisor (rt_normalize_counts_fixed,
// rt_post_process_counts_fixed) and the budgeted allocator from a weight map to counts (rt_sample_allocate).  All three work on the
// current device, on the caller's stream.  The two that read a result back keep their two device words in a cached buffer of the
// device (out_buffer, slot kCountsWordsSlot, under g_dev_busy): nothing is allocated after a device's first call.
constexpr int kCountsWordsSlot = 1000;

// The device's two words, zeroed on `st`.  The caller holds g_dev_busy[*dev].
static int counts_words(const std::string &w, int dev, hipStream_t st, unsigned long long **words) {
    *words = (unsigned long long *)out_buffer(dev, kCountsWordsSlot, sizeof(unsigned long long) * 2);
    if (!*words) return fail(w + ": out of device memory");
    HIP_TRY(hipMemsetAsync(*words, 0, sizeof(unsigned long long) * 2, st));
    return 0;
}
static int counts_device(const std::string &w, int *dev) {
    HIP_TRY(hipGetDevice(dev));
    if (*dev < 0 || *dev >= kMaxDevices) return fail(w + ": device ordinal out of range");
    return 0;
}

static int normalize_counts_impl(const int64_t *d_sum_fixed, const int32_t *d_samples, int num_pixels, int64_t *d_out_fixed, hipStream_t st) {
    const std::string w("rt_normalize_counts_fixed");
    if (!d_sum_fixed || !d_samples || !d_out_fixed) return fail(w + ": null " + (!d_sum_fixed ? "d_sum_fixed" : !d_samples ? "d_samples" : "d_out_fixed"));
    if (num_pixels < 1) return fail(w + ": num_pixels must be at least 1");
    if (num_pixels > 0x7fffffff / 3) return fail(w + ": more than 715827882 pixels");
    int dev = 0;
    if (counts_device(w, &dev)) return 1;
    unsigned long long h[2] = {0, 0};
    {
        std::lock_guard<std::mutex> lock(g_dev_busy[dev]);
        unsigned long long *words = nullptr;
        if (counts_words(w, dev, st, &words)) return 1;
        hipLaunchKernelGGL(k_counts_negative, dim3((num_pixels + 255) / 256), dim3(256), 0, st, d_samples, num_pixels, words);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, words, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (h[0]) return fail(w + ": " + std::to_string(h[0]) + " pixel(s) with a negative sample count");
    const int nv = num_pixels * 3;
    hipLaunchKernelGGL(k_normalize_counts, dim3((nv + 255) / 256), dim3(256), 0, st, (const long long *)d_sum_fixed, d_samples, nv, (long long *)d_out_fixed);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int post_process_counts_impl(const int64_t *d_sum_fixed, const int32_t *d_samples, int num_pixels, float *d_rgb_out, hipStream_t st) {
    const std::string w("rt_post_process_counts_fixed");
    if (!d_sum_fixed || !d_samples || !d_rgb_out) return fail(w + ": null " + (!d_sum_fixed ? "d_sum_fixed" : !d_samples ? "d_samples" : "d_rgb_out"));
    if (num_pixels < 1) return fail(w + ": num_pixels must be at least 1");
    if (num_pixels > 0x7fffffff / 3) return fail(w + ": more than 715827882 pixels");
    const int nv = num_pixels * 3;
    hipLaunchKernelGGL(k_post_process_counts, dim3((nv + 255) / 256), dim3(256), 0, st, (const long long *)d_sum_fixed, d_samples, d_rgb_out, nv);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int sample_allocate_impl(const float *d_weight, int num_pixels, int min_count, int max_count, int64_t budget, int32_t *d_count_out,
                                int64_t *total_out, hipStream_t st) {
    const std::string w("rt_sample_allocate");
    if (!d_weight || !d_count_out || !total_out) return fail(w + ": null " + (!d_weight ? "d_weight" : !d_count_out ? "d_count_out" : "total_out"));
    if (num_pixels < 1) return fail(w + ": num_pixels must be at least 1");
    if (min_count < 0) return fail(w + ": min_count = " + std::to_string(min_count) + " is negative");
    if (max_count < min_count) return fail(w + ": max_count = " + std::to_string(max_count) + " is below min_count = " + std::to_string(min_count));
    const long long floor_total = (long long)num_pixels * min_count;  // (below 2^62)
    if (budget < floor_total) return fail(w + ": budget = " + std::to_string(budget) + " is below num_pixels * min_count = " + std::to_string(floor_total));
    const long long extra = budget - floor_total;
    if (extra >= (1LL << 31)) return fail(w + ": budget - num_pixels * min_count = " + std::to_string(extra) + " exceeds 2147483647");
    int dev = 0;
    if (counts_device(w, &dev)) return 1;
    unsigned long long h[2] = {0, 0};
    std::lock_guard<std::mutex> lock(g_dev_busy[dev]);
    unsigned long long *words = nullptr;
    if (counts_words(w, dev, st, &words)) return 1;
    const dim3 grid((num_pixels + 255) / 256), block(256);
    hipLaunchKernelGGL(k_allocate_total, grid, block, 0, st, d_weight, num_pixels, words);
    hipLaunchKernelGGL(k_allocate_counts, grid, block, 0, st, d_weight, num_pixels, min_count, max_count, (unsigned long long)extra, words, d_count_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, words, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *total_out = (int64_t)h[1];
    return 0;
}
