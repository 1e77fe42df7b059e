// ---- whole frames: shards side by side on host threads of their own (RT_SPLIT, rt_render_multi), their stats merged
// (rt_stats_merge.h), their sums finished into an image on the host (rt_render, rt_render_multi)

// What every shard of a frame is rendered with
struct FrameArgs {
    const rt_camera *camera;
    int width, height, spp, max_bounces;
    uint64_t seed;
    uint32_t flags;  // (kFlagFixedFb: the sums are int64)
};
// One shard, rendered by a host thread of its own on a stream of its own
struct ShardJob {
    int device;             // made current on the thread
    const rt_scene *scene;  // as it exists on `device` (scene_on_device)
    int shard_index, shard_count;
    float *d_sum;           // the shard's raw sums, on `device`
    bool zero_sums;         // the thread zeroes d_sum first; otherwise the caller has, and several jobs add into the one buffer
    void *d_peer;           // non-null: d_sum is copied there, on `peer_device`, when the shard is done
    int peer_device;
    int lane;               // the context lane (get_context): jobs that run side by side on one device never share one
};

// Runs the jobs side by side, one host thread each (render.cuh's render() is one thread on one device: this is its form for
// several shards); sub[k] = job k's stats.  Fails with the first failed job's error; `who` names the entry point in what the
// thread itself reports.
int run_shard_jobs(const char *who, const FrameArgs &f, const std::vector<ShardJob> &jobs, std::vector<rt_stats> &sub) {
    const size_t n = jobs.size();
    const size_t sum_bytes = 3 * (size_t)f.width * (size_t)f.height * ((f.flags & kFlagFixedFb) ? sizeof(long long) : sizeof(float));
    sub.assign(n, rt_stats{});
    std::vector<int> rc(n, 0);
    std::vector<std::string> err(n);
    std::vector<std::thread> th;
    for (size_t k = 0; k < n; k++)
        th.emplace_back([&, k] {
            const ShardJob &j = jobs[k];
            auto bail = [&](const std::string &what) { rc[k] = 1; err[k] = std::string(who) + ": " + what + " (device " + std::to_string(j.device) + ")"; };
            if (hipSetDevice(j.device) != hipSuccess) return bail("hipSetDevice failed");
            hipStream_t st;
            if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return bail("stream create failed");
            if (j.zero_sums && hipMemsetAsync(j.d_sum, 0, sum_bytes, st) != hipSuccess) {
                bail("memset failed");
            } else {
                rc[k] = render_shard_impl(j.scene, f.camera, f.width, f.height, f.spp, f.max_bounces, f.seed, j.shard_index, j.shard_count,
                                          f.flags, j.d_sum, st, &sub[k], j.lane);
                if (rc[k]) err[k] = g_last_error;
                else if (j.d_peer) {
                    const hipError_t pe = hipMemcpyPeerAsync(j.d_peer, j.peer_device, j.d_sum, j.device, sum_bytes, st);
                    if (pe != hipSuccess) bail(std::string("peer copy of the shard's sums failed: ") + hipGetErrorString(pe));
                }
            }
            if (hipStreamSynchronize(st) != hipSuccess && rc[k] == 0) bail("stream synchronise failed");
            (void)hipStreamDestroy(st);
        });
    for (auto &t : th) t.join();
    for (size_t k = 0; k < n; k++)
        if (rc[k]) return fail(err[k]);
    return 0;
}

// rt_render_shard[_fixed], and rt_render's one shard.  A shard may be rendered as `split` interleaved sub-shards (RT_SPLIT) on
// separate HIP streams: slot sets are independent, so the sub-shards only meet in the framebuffer atomics, and the tail of
// one sub-shard's persistent trace kernel overlaps the head of the other's.  Without RT_SPLIT: on the calling thread, on `st`.
int render_overlapped(const rt_scene *scene, const rt_camera *camera, int width, int height, int spp,
                      int max_bounces, uint64_t seed, int shard_index, int shard_count, uint32_t flags,
                      float *d_sum, hipStream_t st, rt_stats *stats) {
    int split = 1;
    if (const char *e = knob("RT_SPLIT")) split = std::max(1, std::min(8, atoi(e)));
    while (split > 1 && (shard_count <= 0 || kW % (shard_count * split) != 0 || kW / (shard_count * split) < 4096)) split >>= 1;
    if (split <= 1)
        return render_shard_impl(scene, camera, width, height, spp, max_bounces, seed, shard_index, shard_count, flags,
                                 d_sum, st, stats);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipStreamSynchronize(st));  // the caller zeroed d_sum on its stream
    std::vector<ShardJob> jobs;
    for (int k = 0; k < split; k++)  // (lane 0 is the unsplit shard's)
        jobs.push_back({dev, scene, shard_index * split + k, shard_count * split, d_sum, false, nullptr, 0, k + 1});
    std::vector<rt_stats> sub;
    if (run_shard_jobs("rt_render_shard", {camera, width, height, spp, max_bounces, seed, flags}, jobs, sub)) return 1;
    if (stats) *stats = merge_shard_stats(sub.data(), split, /* sub_shards: */ true);
    return 0;
}

// post_process_framebuffer (render.cuh:330-338) on `st`: from fixed-point sums into d_rgb, or (d_sum_fixed null) in place on
// the float sums in d_rgb.  rt_post_process[_fixed] have checked the arguments.
int post_process_impl(const long long *d_sum_fixed, float *d_rgb, int num_pixels, int num_samples, hipStream_t st) {
    const int nv = num_pixels * 3;
    const float inv = 1.f / (float)num_samples;
    if (d_sum_fixed) hipLaunchKernelGGL(k_post_process_fixed, dim3((nv + 255) / 256), dim3(256), 0, st, d_sum_fixed, d_rgb, nv, inv);
    else hipLaunchKernelGGL(k_post_process, dim3((nv + 255) / 256), dim3(256), 0, st, d_rgb, nv, inv);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Raw sums on the current device -> the image on the host, on the null stream: the other shards' sums (already on this device)
// are added in shard order -- a fixed order: the result does not depend on which shard finished first --, then the
// post-process into d_image (float sums: d_image is d_sum, in place), then the copy out.
int finish_frame(bool fixed, void *d_sum, const std::vector<void *> &d_others, float *d_image, int width, int height, int spp,
                 float *out_rgb) {
    const int nv = 3 * width * height;
    for (void *d_other : d_others) {
        if (fixed) hipLaunchKernelGGL(k_accumulate_i64, dim3((nv + 255) / 256), dim3(256), 0, nullptr, (long long *)d_sum, (const long long *)d_other, nv);
        else hipLaunchKernelGGL(k_accumulate_f32, dim3((nv + 255) / 256), dim3(256), 0, nullptr, (float *)d_sum, (const float *)d_other, nv);
    }
    if (!d_others.empty()) HIP_TRY(hipGetLastError());
    if (int rc = post_process_impl(fixed ? (const long long *)d_sum : nullptr, d_image, width * height, spp, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out_rgb, d_image, sizeof(float) * (size_t)nv, hipMemcpyDeviceToHost));
    return 0;
}

// rt_render: one shard on the current device, the calling thread and the null stream (RT_SPLIT aside); cached buffers 0 (the
// image; float sums in place) and 1 (fixed-point sums)
int render_impl(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples, int max_bounces, uint64_t seed,
                uint32_t flags, float *out_rgb, rt_stats *stats) {
    if (!out_rgb) return fail("rt_render: out_rgb is null");
    if (width <= 0 || height <= 0) return fail("rt_render: bad dimensions");
    if ((long long)width * height > (long long)(0x7fffffff / 3)) return fail("rt_render: width*height exceeds 715827882 pixels");
    const bool fixed = (flags & RT_FLAG_DETERMINISTIC) != 0;
    const size_t n_values = 3 * (size_t)width * height;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) return fail("rt_render: device ordinal out of range");
    std::lock_guard<std::mutex> out_lock(g_dev_busy[dev]);  // (this device's cached buffers serve one host-output call at a time)
    float *d_fb = (float *)out_buffer(dev, 0, sizeof(float) * n_values);
    long long *d_fixed = fixed ? (long long *)out_buffer(dev, 1, sizeof(long long) * n_values) : nullptr;
    if (!d_fb || (fixed && !d_fixed)) return fail("rt_render: out of device memory");
    void *d_sum = fixed ? (void *)d_fixed : (void *)d_fb;
    HIP_TRY(hipMemsetAsync(d_sum, 0, n_values * (fixed ? sizeof(long long) : sizeof(float)), nullptr));
    if (int rc = render_overlapped(scene, camera, width, height, num_samples, max_bounces, seed, 0, 1,
                                   (flags & ~kFlagFixedFb) | (fixed ? kFlagFixedFb : 0u), (float *)d_sum, nullptr, stats))
        return rc;
    return finish_frame(fixed, d_sum, {}, d_fb, width, height, num_samples, out_rgb);
}

// Peer access between dev0 and every other listed device, once per pair and process: with it the shards' sums travel over xGMI
// straight into dev0's memory; without it hipMemcpyPeerAsync still works, staged through host memory by the runtime.  Leaves
// some listed device current.  (Nothing of this has run on two PHYSICAL devices yet -- one-GPU boxes list a device twice; the
// first multi-GPU run is the driver's scaling run, where bench.py's probe records what happened here: `peer_access`.)
void ensure_peer_access(int dev0, const int *devices, int n_devices) {
    static std::mutex peer_mutex;
    static std::vector<std::pair<int, int>> peer_done;
    std::lock_guard<std::mutex> peer_lock(peer_mutex);
    for (int k = 1; k < n_devices; k++) {
        const int dk = devices[k];
        if (dk == dev0 || std::find(peer_done.begin(), peer_done.end(), std::make_pair(dev0, dk)) != peer_done.end()) continue;
        peer_done.push_back({dev0, dk});
        int can01 = 0, can10 = 0;
        std::string why;
        if (hipDeviceCanAccessPeer(&can01, dev0, dk) != hipSuccess || hipDeviceCanAccessPeer(&can10, dk, dev0) != hipSuccess) why = "hipDeviceCanAccessPeer failed";
        else if (!can01 || !can10) why = "the devices report no peer access";
        else {
            hipError_t e1 = hipSetDevice(dev0) == hipSuccess ? hipDeviceEnablePeerAccess(dk, 0) : hipErrorInvalidDevice;
            hipError_t e2 = hipSetDevice(dk) == hipSuccess ? hipDeviceEnablePeerAccess(dev0, 0) : hipErrorInvalidDevice;
            if (e1 == hipErrorPeerAccessAlreadyEnabled) e1 = hipSuccess;  // (PyTorch, or an earlier library in the process, got there first)
            if (e2 == hipErrorPeerAccessAlreadyEnabled) e2 = hipSuccess;
            (void)hipGetLastError();
            if (e1 != hipSuccess || e2 != hipSuccess) why = std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2);
        }
        g_peer_log += "devices " + std::to_string(dev0) + " <-> " + std::to_string(dk) + ": " + (why.empty() ? "peer access enabled" : "NO peer access (" + why + "): copies go through host memory") + "; ";
        if (!why.empty())
            fprintf(stderr, "rtcuda_amd: rt_render_multi: no peer access between devices %d and %d (%s): the shard's sums are copied through host memory\n", dev0, dk, why.c_str());
    }
}

// rt_render_multi: device shard k of n on devices[k] -- its replica of the scene, a host thread, context lane 8 + k --, the
// sums brought to devices[0] and finished there.  Cached buffers, per (device, slot) like rt_render's: 2 + 2k = shard k's sums
// on its device, 3 + 2k = its staging copy on devices[0], 1 = the post-processed image (fixed-point mode).
int render_multi_impl(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples, int max_bounces,
                      uint64_t seed, uint32_t flags, const int *devices, int n_devices, float *out_rgb, rt_stats *stats) {
    if (!scene || !camera || !out_rgb) return fail("rt_render_multi: null argument");
    if (!devices || n_devices < 1) return fail("rt_render_multi: empty device list");
    if (width <= 0 || height <= 0) return fail("rt_render_multi: bad dimensions");
    if ((long long)width * height > (long long)(0x7fffffff / 3)) return fail("rt_render_multi: width*height exceeds 715827882 pixels");
    if (kW % n_devices != 0) return fail("rt_render_multi: the number of devices must divide 1048576 (1, 2, 4, 8, ...)");
    int n_visible = 0;
    HIP_TRY(hipGetDeviceCount(&n_visible));
    for (int k = 0; k < n_devices; k++)
        if (devices[k] < 0 || devices[k] >= n_visible)
            return fail("rt_render_multi: devices[" + std::to_string(k) + "] = " + std::to_string(devices[k]) + " but " +
                        std::to_string(n_visible) + " device(s) are visible");
    const bool fixed = (flags & RT_FLAG_DETERMINISTIC) != 0;
    const size_t n_values = 3 * (size_t)width * height;
    const size_t sum_bytes = n_values * (fixed ? sizeof(long long) : sizeof(float));
    const int dev0 = devices[0];
    DeviceGuard home;  // (the calling thread's device is restored on every return path)
    if (home.enter(dev0)) return 1;
    // every device's copy of the scene, before any thread starts (replicas are created under the scene's lock)
    std::vector<const rt_scene *> on_dev(n_devices, nullptr);
    for (int k = 0; k < n_devices; k++) {
        on_dev[k] = scene_on_device(scene, devices[k]);
        if (!on_dev[k]) return 1;
    }
    std::vector<int> distinct(devices, devices + n_devices);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    if (distinct.back() >= kMaxDevices) return fail("rt_render_multi: device ordinal out of range");
    std::vector<std::unique_lock<std::mutex>> out_locks;  // (ascending device order: two concurrent calls cannot deadlock)
    for (int d : distinct) out_locks.emplace_back(g_dev_busy[d]);
    ensure_peer_access(dev0, devices, n_devices);
    auto alloc = [&](int device, int slot, size_t bytes) { return home.select(device) ? nullptr : out_buffer(device, slot, bytes); };
    // shard k renders into its own raw-sum buffer on ITS device; shards 1.. land in a staging buffer on devices[0]
    std::vector<ShardJob> jobs;
    std::vector<void *> d_staged;  // shards 1..: where their sums are on devices[0]
    for (int k = 0; k < n_devices; k++) {
        void *d_sum = alloc(devices[k], 2 + 2 * k, sum_bytes), *d_peer = nullptr;
        if (!d_sum) return fail("rt_render_multi: out of device memory on device " + std::to_string(devices[k]));
        if (k > 0 && devices[k] != dev0) {  // (same device: the buffer is its own staging)
            d_peer = alloc(dev0, 3 + 2 * k, sum_bytes);
            if (!d_peer) return fail("rt_render_multi: out of device memory on device " + std::to_string(dev0));
        }
        if (k > 0) d_staged.push_back(d_peer ? d_peer : d_sum);
        jobs.push_back({devices[k], on_dev[k], k, n_devices, (float *)d_sum, true, d_peer, dev0, 8 + k});
    }
    float *d_image = fixed ? (float *)alloc(dev0, 1, n_values * sizeof(float)) : jobs[0].d_sum;
    if (!d_image) return fail("rt_render_multi: out of device memory");
    std::vector<rt_stats> sub;
    if (run_shard_jobs("rt_render_multi", {camera, width, height, num_samples, max_bounces, seed, (flags & ~kFlagFixedFb) | (fixed ? kFlagFixedFb : 0u)},
                       jobs, sub))
        return 1;
    if (home.select(dev0)) return 1;
    if (int rc = finish_frame(fixed, jobs[0].d_sum, d_staged, d_image, width, height, num_samples, out_rgb)) return rc;
    if (stats) *stats = merge_shard_stats(sub.data(), n_devices, /* sub_shards: */ false);
    return 0;
}
