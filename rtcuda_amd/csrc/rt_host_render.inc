// ---- per-device render context: pools are allocated once per (device, n) and reused
struct Context {
    int device = -1;
    int n = 0;
    int lane = 0;  // concurrent sub-shards of one render use separate contexts (and streams)
    DPools pools{};
    std::vector<void *> allocs;
    DCounters *d_ctr = nullptr;
    DCounters *h_ctr = nullptr;  // pinned ring of snapshots
    DWaveRow *d_rows = nullptr;  // one row per wave of the stage grid
    int n_rows = 0;
    uint32_t *d_jump = nullptr;
    hipEvent_t ev_ring[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_c = nullptr;
    // RNG states are a pure function of (seed, slot range): keep them cached across renders
    uint64_t rng_seed = 0;
    int rng_lo = -1;
    bool rng_valid = false;
    uint32_t *rng_backup = nullptr;  // 6 x n words
    std::vector<hipEvent_t> timing_events;
    unsigned int *d_lock = nullptr;  // mat() events per lockstep round of the final generation (lock_cap words, grown on demand)
    int lock_cap = 0;
    int *d_over = nullptr;  // overflow part of the traversal stacks of this context's grids (ensure_overflow)
    int over_levels = 0;
    // a counted frame's prepass (counts_prepass): the prefix sum of the count map, pixels + 1 words, and the tiles' words; grown
    // once per image size
    uint32_t *d_counts_offset = nullptr;
    unsigned long long *d_counts_words = nullptr;
    size_t counts_pixels = 0;
    std::mutex busy;  // a context (pools, counters, events) serves one render at a time
    Context() = default;
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    ~Context() {  // (rt_shutdown, or a context that failed half-way through get_context): on the device it lives on
        int saved = 0;
        const bool hop = device >= 0 && hipGetDevice(&saved) == hipSuccess && saved != device && hipSetDevice(device) == hipSuccess;
        for (void *q : allocs) (void)hipFree(q);
        (void)hipFree(d_lock);
        (void)hipFree(d_over);
        (void)hipFree(d_counts_offset);
        (void)hipFree(d_counts_words);
        if (h_ctr) (void)hipHostFree(h_ctr);
        for (hipEvent_t e : ev_ring) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : {ev_a, ev_b, ev_c}) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : timing_events) (void)hipEventDestroy(e);
        if (hop) (void)hipSetDevice(saved);
    }
};
std::mutex g_ctx_mutex;
std::vector<std::unique_ptr<Context>> g_contexts;

// Device buffers of the calls that take HOST output (rt_render, rt_render_multi): raw sums, staging, the post-processed image.
// Kept per (device, slot) and reused from call to call -- a hipMalloc / hipFree pair per frame cost ~0.3 ms and a device
// synchronisation each (round 4 allocated them per call); released by rt_shutdown.  The buffers of ONE device serve one call at
// a time (g_dev_busy[device]); calls on different devices -- one host thread per GPU -- do not wait for each other.
struct OutBuffer {
    int device = -1, slot = 0;
    void *ptr = nullptr;
    size_t bytes = 0;
};
constexpr int kMaxDevices = 64;
std::mutex g_dev_busy[kMaxDevices];
std::mutex g_out_mutex;  // the list below
std::vector<OutBuffer> g_out_buffers;
// (caller holds g_dev_busy[device]; the current device must be `device`)
void *out_buffer(int device, int slot, size_t bytes) {
    std::lock_guard<std::mutex> list_lock(g_out_mutex);
    for (OutBuffer &b : g_out_buffers)
        if (b.device == device && b.slot == slot) {
            if (b.bytes >= bytes) return b.ptr;
            (void)hipFree(b.ptr);
            b.ptr = nullptr;
            b.bytes = 0;
            if (hipMalloc(&b.ptr, bytes) != hipSuccess) return nullptr;
            b.bytes = bytes;
            return b.ptr;
        }
    OutBuffer b;
    b.device = device;
    b.slot = slot;
    if (hipMalloc(&b.ptr, bytes) != hipSuccess) return nullptr;
    b.bytes = bytes;
    g_out_buffers.push_back(b);
    return b.ptr;
}

// rt_shutdown: releases every device allocation the library holds behind the scenes -- the per-device render contexts (path
// pools, RNG states, counters, overflow stacks, events) and the cached output buffers of rt_render / rt_render_multi.  Scenes are
// the caller's (rt_scene_destroy).  No render may be in flight.  The library works again afterwards (everything is re-created
// on demand).  (The reference frees nothing at all: render.cuh:374-391, bvh.cuh:211-217.)
void shutdown_impl() {
    int saved = 0;
    const bool have = hipGetDevice(&saved) == hipSuccess;
    {
        std::lock_guard<std::mutex> lock(g_ctx_mutex);
        g_contexts.clear();  // (~Context frees on the context's own device)
    }
    {
        std::lock_guard<std::mutex> list_lock(g_out_mutex);
        for (OutBuffer &b : g_out_buffers) {
            if (hipSetDevice(b.device) == hipSuccess) (void)hipFree(b.ptr);
        }
        g_out_buffers.clear();
    }
    if (have) (void)hipSetDevice(saved);
}

template <typename T>
int dev_alloc(Context &c, T *&ptr, size_t count) {
    void *raw = nullptr;
    HIP_TRY(hipMalloc(&raw, count * sizeof(T)));
    c.allocs.push_back(raw);
    ptr = (T *)raw;
    return 0;
}

int get_context(int n, int lane, Context **out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    for (auto &c : g_contexts)
        if (c->device == dev && c->n == n && c->lane == lane) {
            *out = c.get();
            return 0;
        }
    auto c = std::make_unique<Context>();
    c->device = dev;
    c->n = n;
    c->lane = lane;
    DPools &p = c->pools;
    p.n = n;
    if (dev_alloc(*c, p.base, (size_t)A_COUNT * n)) return 1;
    if (dev_alloc(*c, c->rng_backup, (size_t)6 * n)) return 1;
    if (dev_alloc(*c, c->d_ctr, 1)) return 1;
    // one counter row per wave of the largest grid this context launches: k_advance's (n / 64 waves)
    c->n_rows = ((n + kBlock - 1) / kBlock) * (kBlock / 64);
    if (dev_alloc(*c, c->d_rows, (size_t)c->n_rows)) return 1;
    if (dev_alloc(*c, c->d_jump, (size_t)20 * 800)) return 1;
    HIP_TRY(hipMemcpy(c->d_jump, jump_powers().data(), sizeof(uint32_t) * 20 * 800, hipMemcpyHostToDevice));
    HIP_TRY(hipHostMalloc((void **)&c->h_ctr, sizeof(DCounters) * 4, hipHostMallocDefault));
    for (auto &e : c->ev_ring) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventCreate(&c->ev_a));
    HIP_TRY(hipEventCreate(&c->ev_b));
    HIP_TRY(hipEventCreate(&c->ev_c));
    *out = c.get();
    g_contexts.push_back(std::move(c));
    return 0;
}

int grid_for(int n) { return (n + kBlock - 1) / kBlock; }

// Entries of a lane's traversal stack kept in LDS (the rest of scene->stack_bound goes to the global overflow column).
// RT_STACK_CAP lowers it: a test knob that drives every traversal through the overflow path.
static int lds_stack_cap(const rt_scene *scene, int limit) {
    int cap = std::min(limit, std::max(1, scene->stack_bound));
    if (const char *e = knob("RT_STACK_CAP")) cap = std::max(1, std::min(cap, atoi(e)));
    return cap;
}

// Kernel selection: the builds of a kernel template that share a source of camera rays have the same signature, so the flags pick a
// function pointer and the caller launches (and sizes the grid with) that pointer.
template <class SRC>
using AdvanceKernel = decltype(&k_advance<SRC, false>);
using TraceKernel = decltype(&k_trace<false>);
template <class SRC>
using PathsKernel = void (*)(DScene, DPools, SRC, AdvanceParams, float *, DWaveRow *, int, int *, int, int, unsigned long long *, int, int, int, int, int, int,
                             unsigned int *, unsigned long long *);

// (Camera and RayTable: the sources whose frames can run on the round pipeline)
template <class SRC>
static AdvanceKernel<SRC> advance_kernel(bool lds_tables) { return lds_tables ? k_advance<SRC, true> : k_advance<SRC, false>; }

// k_trace: with RT_FLAG_REFERENCE_WALK the build that walks the reference's tree (the node format does not matter
// then); `verify`: the default build -- the product's walk with the reference's decisions (ref_visible); neither:
// RT_FLAG_WATERTIGHT.  Otherwise the node format is a property of the scene.
static TraceKernel trace_kernel(bool literal, bool verify, bool wide) {
    if (literal) return k_trace<false, true>;
    if (verify) return wide ? k_trace<true, false, true> : k_trace<false, false, true>;
    return wide ? k_trace<true> : k_trace<false>;
}

// k_paths<BUILD, ...>: the instances of a build tag (rtcuda_amd.hip) that a frame can select, and which of them.
// MIN_WAVES = 4 waves per SIMD (at most 128 VGPRs) when the grid fills the chip, 2 (up to 256 VGPRs) when the shard is so small
// that only 2 workgroups per CU exist anyway (8-GPU runs).  RT_FLAG_REFERENCE_WALK: the build whose node block is the reference's
// own walk (full pool: the 4-wave build although it spills 53 VGPRs -- measured 1 082 ms for C2's frame against 1 412 ms for the
// spill-free 2-wave build at half the occupancy).  Per-sample streams on the full pool: the build in which the waves draw their
// camera rays (rows, ids) from the frame's counter; on few blocks they are tied to slots and gen() stays inside ADV.
//   PathsCamera, PathsBg          all of the above, on either node format
//   PathsChunked, PathsChunkedBg  the 4-waves-per-SIMD reference-mode instances only (the caller asks for nothing else)
//   PathsRays                     4-wide tree only (a 2-wide scene runs such a frame on the round pipeline); no reference walk
//   PathsKeyed, PathsCounts       4-wide tree, the triangle-list definition of a hit, per-sample streams: one instance per pool size
struct PathsPick {
    bool few_blocks, per_sample, literal, verify;
};
template <class BUILD, bool LDS_TABLES, bool WIDE>
static PathsKernel<typename BUILD::Src> paths_kernel_of(const PathsPick &f) {
    constexpr bool kCamera = std::is_same<typename BUILD::Src, Camera>::value;  // (the tags that have a reference-walk build)
    constexpr bool kStreams = std::is_same<BUILD, PathsKeyed>::value || std::is_same<BUILD, PathsCounts>::value;
    if constexpr (kStreams) {
        if (f.few_blocks) return k_paths<BUILD, LDS_TABLES, WIDE, 2, false, false, false>;
        return k_paths<BUILD, LDS_TABLES, WIDE, 4, true, false, false>;
    } else {
        if constexpr (kCamera) {
            if (f.literal) {
                if constexpr (!BUILD::kChunks) {
                    if (f.few_blocks) return k_paths<BUILD, LDS_TABLES, false, 2, false, true, false>;
                }
                return k_paths<BUILD, LDS_TABLES, false, 4, false, true, false>;
            }
        }
        if constexpr (kCamera && !BUILD::kChunks) {
            if (f.per_sample && !f.few_blocks) return k_paths<BUILD, LDS_TABLES, WIDE, 4, true, false, false>;
        }
        if constexpr (!BUILD::kChunks) {
            if (f.few_blocks) return f.verify ? k_paths<BUILD, LDS_TABLES, WIDE, 2, false, false, true> : k_paths<BUILD, LDS_TABLES, WIDE, 2, false, false, false>;
        }
        return f.verify ? k_paths<BUILD, LDS_TABLES, WIDE, 4, false, false, true> : k_paths<BUILD, LDS_TABLES, WIDE, 4, false, false, false>;
    }
}
// (tables, keyed tables and counted frames walk 4-wide nodes only: their 2-wide instances do not exist)
template <class BUILD>
static PathsKernel<typename BUILD::Src> paths_kernel(bool lds_tables, bool wide, const PathsPick &f) {
    if constexpr (std::is_same<typename BUILD::Src, Camera>::value) {
        if (!wide) return lds_tables ? paths_kernel_of<BUILD, true, false>(f) : paths_kernel_of<BUILD, false, false>(f);
    }
    return lds_tables ? paths_kernel_of<BUILD, true, true>(f) : paths_kernel_of<BUILD, false, true>(f);
}

// Global overflow part of the traversal stacks: `levels` entries for each of kOverStride lanes.  Every OWNER of
// concurrently running grids has its own buffer -- a render context (one render at a time: Context::busy), or a
// scene's query state (queries, trace hooks and AOVs of one scene take turns: QueryState::mutex) -- because a lane
// indexes its column by its position in ITS grid only: two grids in flight on one device (RT_SPLIT sub-shards, host
// threads rendering different shard sizes) would otherwise push to and pop from the same columns.  Grown on demand under the owner's lock, never shrunk.
int ensure_overflow(int *&ptr, int &have_levels, int levels) {
    levels = std::max(levels, 1);
    if (ptr && have_levels >= levels) return 0;
    if (ptr) {
        HIP_TRY(hipDeviceSynchronize());  // (the owner is idle; this only guards against a caller's stray stream)
        (void)hipFree(ptr);
        ptr = nullptr;
        have_levels = 0;
    }
    HIP_TRY(hipMalloc((void **)&ptr, sizeof(int) * (size_t)levels * kOverStride));
    have_levels = levels;
    return 0;
}

int ensure_rng(Context &c, uint64_t seed, int slot_lo, hipStream_t st, double *seconds) {
    const size_t bytes = sizeof(uint32_t) * (size_t)c.n;
    uint32_t *parts[6];
    for (int k = 0; k < 6; k++) parts[k] = (uint32_t *)c.pools.array(A_RD + k);
    *seconds = 0.0;
    if (!(c.rng_valid && c.rng_seed == seed && c.rng_lo == slot_lo)) {
        HIP_TRY(hipEventRecord(c.ev_a, st));
        hipLaunchKernelGGL(k_rng_init, dim3(grid_for(c.n)), dim3(kBlock), 0, st, c.pools, c.n, slot_lo,
                           xorwow_seed(seed), c.d_jump);
        HIP_TRY(hipGetLastError());
        for (int k = 0; k < 6; k++)
            HIP_TRY(hipMemcpyAsync(c.rng_backup + (size_t)k * c.n, parts[k], bytes, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipEventRecord(c.ev_b, st));
        HIP_TRY(hipEventSynchronize(c.ev_b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c.ev_a, c.ev_b));
        *seconds = ms * 1e-3;
        c.rng_valid = true;
        c.rng_seed = seed;
        c.rng_lo = slot_lo;
    } else {
        for (int k = 0; k < 6; k++)
            HIP_TRY(hipMemcpyAsync(parts[k], c.rng_backup + (size_t)k * c.n, bytes, hipMemcpyDeviceToDevice, st));
    }
    return 0;
}

// One frame of one shard.  `rays` null: the camera's frame (rt_render_shard*).  `rays` set (rt_render_rays_*, which has
// validated the table on the device; `camera` is not looked at): camera ray c is row c of the table, the frame is
// rays->n_rays camera rays over width * height = n_pixels x 1 pixels, and `spp` is the rays_per_pixel of the c / spp rule.
// Everything else is one body: render_shard_impl checks and sets up a FrameRun, whose phases run and read the frame back.
// `keyed` (rt_render_rays_keyed_*; the caller sets RT_FLAG_RNG_PER_SAMPLE): `keyed_table` instead of `table`, k_paths<PathsKeyed>.
struct RayFrame {
    RayTable table;
    long long n_rays;
    bool keyed = false;
    KeyedRayTable keyed_table{};
};
// A counted frame (rt_render_counts_fixed): the camera's frame in the per-sample mode, `spp` the sample stride, and of it the
// samples first[p] .. first[p] + count[p] - 1 of every pixel.  render_shard_impl runs the prepass (counts_prepass) once it holds
// the context, whose scratch the prefix sum lives in; the frame's camera rays are the sum of the counts.
struct CountsFrame {
    const int32_t *d_first, *d_count;
    int32_t *d_samples;
};
// What the phases of one frame share: the context, the kernels' arguments, the round pipeline's launch (k_advance +
// k_trace: RT_PERSISTENT=0 frames and the lockstep final generation) and what the stats are made from.
struct FrameRun {
    Context &c;
    const rt_scene *scene;
    const RayFrame *rays;
    hipStream_t st;
    float *d_sum;
    uint32_t flags;
    bool per_sample;
    HitMode mode;
    bool lds_tables = false, persistent = true, finished = false, ran_lockstep = false;
    int cus = 0, stack_cap = 0, top_records_in_lds = 0, slot_chunk = 0, slot_head = 0, lock_enqueued = 0;
    bool ran_bg = false;  // the persistent launch was k_paths<PathsBg> / k_paths<PathsChunkedBg> (a rectangle smaller than the frame)
    bool counted = false;  // a counted frame: k_paths<PathsCounts> on counts_src (its camera is `cam`)
    CountsCamera counts_src{};
    DScene sc{};
    Camera cam{};
    AdvanceParams ap{};
    TraceParams tpp{};
    size_t lds_bytes = 0, ev_used = 0;  // (ev_used: of c.timing_events)
    dim3 grid_trace;
    TraceKernel trace = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;  // the frame's own pair: destroyed on every return path
    long long rounds = 0;
    float ms_paths = 0.f;
    double rng_seconds = 0.0, ref_tree_seconds = 0.0;
    ~FrameRun() {
        if (ev_start) (void)hipEventDestroy(ev_start);
        if (ev_stop) (void)hipEventDestroy(ev_stop);
    }
    void launch_advance() {
        const dim3 grid(grid_for(ap.n)), block(kBlock);
        if (rays) hipLaunchKernelGGL(advance_kernel<RayTable>(lds_tables), grid, block, 0, st, sc, c.pools, rays->table, ap, d_sum, c.d_ctr, c.d_rows, c.d_lock);
        else hipLaunchKernelGGL(advance_kernel<Camera>(lds_tables), grid, block, 0, st, sc, c.pools, cam, ap, d_sum, c.d_ctr, c.d_rows, c.d_lock);
    }
    void launch_trace() { hipLaunchKernelGGL(trace, grid_trace, dim3(kBlock), lds_bytes, st, sc, c.pools, tpp, stack_cap, c.d_over); }
    int run_persistent(), run_rounds(), run_lockstep(), frame_stats(rt_stats *stats);  // the phases, in this order
    int next_event(hipEvent_t *out) {
        if (ev_used == c.timing_events.size()) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            c.timing_events.push_back(e);
        }
        *out = c.timing_events[ev_used++];
        return 0;
    }
};

#ifdef RT_TRACE_PROFILE
static int report_paths_profile(unsigned long long *paths_prof, int paths_blocks) {
    unsigned long long h[kProfHead];
    HIP_TRY(hipMemcpy(h, paths_prof, sizeof(h), hipMemcpyDeviceToHost));
    fprintf(stderr, "k_paths cycles: ADV %.1f%% (%.0f / block) node %.1f%% (%.0f) tri %.1f%% (%.0f) rest %.1f%%\n",
            100.0 * h[8] / h[11], h[0] ? (double)h[8] / h[0] : 0.0, 100.0 * h[9] / h[11], h[2] ? (double)h[9] / h[2] : 0.0,
            100.0 * h[10] / h[11], h[4] ? (double)h[10] / h[4] : 0.0, 100.0 * (double)(h[11] - h[8] - h[9] - h[10]) / h[11]);
    fprintf(stderr, "k_paths GEN blocks: %llu avg lanes %.1f, %.1f %% of wave time (%.0f cycles / block; inside `rest` above)\n", h[12],
            h[12] ? (double)h[15] / h[12] : 0.0, 100.0 * h[16] / h[11], h[12] ? (double)h[16] / h[12] : 0.0);
    fprintf(stderr, "k_paths GEN cycles per wave %.0f; chunked deal: %.2f hand-overs per lane, made in %.2f %% of the GEN blocks\n", h[14] ? (double)h[16] / h[14] : 0.0,
            h[14] ? (double)h[22] / (64.0 * h[14]) : 0.0, h[12] ? 100.0 * h[23] / h[12] : 0.0);
    fprintf(stderr, "k_paths waves: %llu, mean lifetime %.0f cycles, longest %.0f cycles (x%.3f)\n", h[14], (double)h[11] / h[14], (double)h[13],
            (double)h[13] * h[14] / h[11]);
    // lane-idle tail: per wave, the lane-cycles between each lane's last work and the wave's exit -- whole-wave blocks issued
    // for lanes that have run out of slots -- as a share of wave time x 64; and the wave's longest such tail (from its first
    // lane going idle for good to its exit)
    fprintf(stderr, "k_paths lane-idle tail: %.2f %% of wave time x 64 lanes; a wave's first lane is idle for good %.2f %% of the wave's time before its exit\n",
            100.0 * h[20] / (64.0 * h[11]), 100.0 * h[21] / h[11]);
    fprintf(stderr, "k_paths fin section: %.1f %% of wave time, entered in %llu iterations (avg %.1f finished lanes), %.0f cycles each\n",
            100.0 * h[17] / h[11], h[19], h[19] ? (double)h[18] / h[19] : 0.0, h[19] ? (double)h[17] / h[19] : 0.0);
    fprintf(stderr, "k_paths profile: ADV blocks %llu avg lanes %.1f | node steps %llu avg lanes %.1f (ADV-waiting %.1f) | tri steps %llu avg lanes %.1f (ADV-waiting %.1f)\n",
            h[0], h[0] ? (double)h[1] / h[0] : 0.0, h[2], h[2] ? (double)h[3] / h[2] : 0.0, h[2] ? (double)h[6] / h[2] : 0.0, h[4],
            h[4] ? (double)h[5] / h[4] : 0.0, h[4] ? (double)h[7] / h[4] : 0.0);
    fprintf(stderr, "k_paths Russian-roulette chain: %.2f turns per ADV block (the longest lane's rolls), %.1f %% of the ADV blocks went round at all (%.2f turns each)\n",
            h[0] ? (double)h[24] / h[0] : 0.0, h[0] ? 100.0 * h[25] / h[0] : 0.0, h[25] ? (double)h[24] / h[25] : 0.0);
    if (const char *dump = knob("RT_PROF_DUMP")) {  // per-wave records: hw_id xcc_id cycles blocks idle_lane_cycles longest_lane_tail
        std::vector<unsigned long long> recs(kProfRec * (size_t)paths_blocks * (kBlock / 64));
        HIP_TRY(hipMemcpy(recs.data(), paths_prof + kProfHead, recs.size() * 8, hipMemcpyDeviceToHost));
        if (FILE *f = fopen(dump, "w")) {
            for (size_t k = 0; k < recs.size(); k += kProfRec)
                fprintf(f, "%zu %llu %llu %llu %llu %llu %llu\n", k / kProfRec, recs[k], recs[k + 1], recs[k + 2], recs[k + 3], recs[k + 4], recs[k + 5]);
            fclose(f);
        }
    }
    (void)hipFree(paths_prof);
    return 0;
}
static int report_trace_profile(unsigned long long *d_prof) {
    unsigned long long h[16];
    HIP_TRY(hipMemcpy(h, d_prof, sizeof(h), hipMemcpyDeviceToHost));
    fprintf(stderr, "trace profile: waves %llu outer_it %llu refills %llu | inner_it %llu avg_lanes %.1f | leaf_it %llu avg_lanes %.1f | "
                    "tri_it %llu avg_lanes %.1f | active lanes at loop top %.1f | finalised lanes per refill %.1f\n",
            h[10], h[0], h[1], h[2], h[2] ? (double)h[3] / h[2] : 0.0, h[4], h[4] ? (double)h[5] / h[4] : 0.0, h[6],
            h[6] ? (double)h[7] / h[6] : 0.0, h[0] ? (double)h[8] / h[0] : 0.0, h[1] ? (double)h[9] / h[1] : 0.0);
    (void)hipFree(d_prof);
    return 0;
}
#endif

// ---- asynchronous part of the frame: ONE persistent launch (k_paths, or a table's k_paths<PathsRays> / k_paths<PathsKeyed>), sized
// by rt_launch_plan.h
int FrameRun::run_persistent() {
    const int paths_cap = lds_stack_cap(scene, kPathsLdsStack);
    // (the uniforms hold the source of camera rays: a Camera or a table no larger, or a counted frame's CountsCamera)
    const size_t fixed_lds = (lds_tables ? sizeof(float) * (size_t)((scene->tab_dwords + 3) & ~3) : 0) + (counted ? sizeof(CountsCamera) : sizeof(Camera)) + sizeof(AdvanceParams);
    const rtplan::PathsLaunch p = rtplan::plan_paths_launch(c.n, cus, scene->wide, scene->n_nodes, paths_cap, !rays, ap.width, ap.spp, fixed_lds);
    top_records_in_lds = p.top_n;
    unsigned long long *paths_prof = nullptr;
#ifdef RT_TRACE_PROFILE
    const size_t prof_bytes = 8 * kProfHead + 8 * kProfRec * (size_t)(grid_for(c.n) * (kBlock / 64));
    HIP_TRY(hipMalloc((void **)&paths_prof, prof_bytes));
    HIP_TRY(hipMemset(paths_prof, 0, prof_bytes));
#endif
    auto launch_paths = [&](auto kernel, const auto &src, int top_n) {
        hipLaunchKernelGGL(kernel, dim3(p.blocks), dim3(kBlock), p.lds_bytes, st, sc, c.pools, src, ap, d_sum, c.d_rows, paths_cap, c.d_over,
                           p.adv_batch, (flags & 0x100u) ? 1 : 0, paths_prof, top_n, p.prio_rotate, p.rot_wave, p.rot_set, p.gen_batch, p.tri_follow, &c.d_ctr->pad2[0],
                           &c.d_ctr->vstat[0]);
    };
    HIP_TRY(hipEventRecord(c.ev_a, st));
    // (the reference-walk build is passed top_n = 0, while top_n * 64 bytes of LDS stay reserved and reported in reserved[2])
    // (a chunk > 0 launches k_paths<PathsChunked>, 4-waves-per-SIMD reference-mode builds that keep no records in LDS: their `top_n`
    // carries the chunk; a frame of one generation runs no chain in k_paths -- every slot parks at once -- and keeps the static
    // deal, and so do ray tables)
    int chunk = (rays || p.few_blocks || per_sample || ap.last_gen < 1 || ap.n != c.n) ? 0 : rtplan::slot_chunk_for(p, ap.last_gen);
    // (a rectangle smaller than the frame: the builds that pass over background pixels)
    const bool bg = !rays && (long long)ap.bg_w * ap.bg_h < (long long)ap.width * ap.height;
    ran_bg = bg;
    const PathsPick pick{p.few_blocks, per_sample, mode.literal, mode.verify};
    const PathsKernel<Camera> chunked = bg ? paths_kernel<PathsChunkedBg>(lds_tables, scene->wide, pick) : paths_kernel<PathsChunked>(lds_tables, scene->wide, pick);
    if (chunk > 0) {  // (its semaphores are 2 KB of static LDS: beside large tables in LDS they would cost a resident workgroup)
        int per_cu = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, chunked, kBlock, p.lds_bytes));
        chunk = rtplan::slot_chunk_if_resident(chunk, per_cu);
    }
    // (the static head travels above G's 21 bits)
    slot_head = chunk > 0 ? rtplan::slot_head_for(p, ap.n / (p.blocks * kBlock)) : 0;
    static_assert(rtplan::kDealtSetsMax == (int)rtchunks::kDealtSetsMax, "the plan deals what the semaphores hold");
    slot_chunk = chunk;
    if (rays && rays->keyed) launch_paths(paths_kernel<PathsKeyed>(lds_tables, true, pick), rays->keyed_table, p.top_n);
    else if (rays) launch_paths(paths_kernel<PathsRays>(lds_tables, true, pick), rays->table, p.top_n);
    else if (counted) launch_paths(paths_kernel<PathsCounts>(lds_tables, true, pick), counts_src, p.top_n);
    else if (chunk > 0) launch_paths(chunked, cam, chunk | (slot_head << rtplan::kChunkHeadShift));
    else if (bg) launch_paths(paths_kernel<PathsBg>(lds_tables, scene->wide, pick), cam, mode.literal ? 0 : p.top_n);
    else launch_paths(paths_kernel<PathsCamera>(lds_tables, scene->wide, pick), cam, mode.literal ? 0 : p.top_n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c.ev_b, st));
    HIP_TRY(hipEventSynchronize(c.ev_b));
    HIP_TRY(hipEventElapsedTime(&ms_paths, c.ev_a, c.ev_b));
#ifdef RT_TRACE_PROFILE
    if (report_paths_profile(paths_prof, p.blocks)) return 1;
#endif
    finished = true;
    return 0;
}

// ---- the same part on the round-per-launch pipeline (RT_PERSISTENT=0; a table's frame on a 2-wide scene)
// Rounds are enqueued in batches; after each batch the counters are snapshotted into pinned
// host memory.  The host looks at the snapshot of batch b-2 before enqueuing batch b, so the
// GPU always has work queued, and stops when a whole batch traced no ray.
int FrameRun::run_rounds() {
    const int kBatch = 8;  // == ap.batch_mask + 1
    // RT_FLAG_TIME_KERNELS: every kTimeStride-th round is bracketed with HIP events on the launch
    // stream (no host synchronisation); the events are resolved after the loop.
    const int kTimeStride = 4;
    const bool time_kernels = (flags & RT_FLAG_TIME_KERNELS) != 0;
    const long long generations = (ap.cam_end + kW - 1) / kW;
    const long long max_rounds = (generations + 1) * (long long)(ap.max_bounces + 2) + 64;
    int batch = 0;
    while (!finished && rounds < max_rounds) {
        for (int k = 0; k < kBatch; k++) {
            ap.round = (int)(rounds & 0x3fffffff);
            const bool timed = time_kernels && (rounds % kTimeStride) == 0;
            hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr;
            if (timed && (next_event(&e0) || next_event(&e1) || next_event(&e2) || next_event(&e3))) return 1;
            if (timed) HIP_TRY(hipEventRecord(e0, st));
            launch_advance();
            if (timed) HIP_TRY(hipEventRecord(e1, st));
            launch_trace();
            if (timed) HIP_TRY(hipEventRecord(e2, st));
            if (timed) HIP_TRY(hipEventRecord(e3, st));
            rounds++;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&c.h_ctr[batch & 3], c.d_ctr, sizeof(DCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(c.ev_ring[batch & 3], st));
        if (batch >= 1) {
            int prev = (batch - 1) & 3;
            HIP_TRY(hipEventSynchronize(c.ev_ring[prev]));
            // k_advance records liveness only in the round that closes a batch (liveness is monotone):
            // if the closing round of batch b-1 traced nothing, every slot is finished
            if ((long long)c.h_ctr[prev].last_live_round < (long long)batch * kBatch - 1) finished = true;
        }
        batch++;
    }
    return 0;
}

// ---- final generation in lockstep (see k_advance): round 0 generates, every later round is one
// reference iteration; the render ends at the first round in which nothing shades (render.cuh:436)
// All max_bounces + 2 rounds are enqueued back to back; which of them still belong to the render is decided on the
// device (k_advance / k_trace look at lock_shades), and the host learns the number of rounds that ran afterwards.
// The rounds go out in chunks of kLockChunk: the reference's 12 rounds (max_bounces = 10) are ONE chunk -- no host
// read-back inside the frame --, and a caller with max_bounces in the thousands does not pay thousands of empty launches
// once the render has ended: between chunks the host looks at the last round's counter (ADVICE r4).
int FrameRun::run_lockstep() {
    const int n_lock = ap.max_bounces + 2;
    ran_lockstep = finished && !per_sample;
    if (!ran_lockstep) return 0;
    if (n_lock > c.lock_cap) {  // (the stop rule's counters: one word per round, grown on demand)
        HIP_TRY(hipStreamSynchronize(st));
        (void)hipFree(c.d_lock);
        c.d_lock = nullptr;
        c.lock_cap = 0;
        HIP_TRY(hipMalloc((void **)&c.d_lock, sizeof(unsigned) * (size_t)std::max(n_lock, 64)));
        c.lock_cap = std::max(n_lock, 64);
    }
    HIP_TRY(hipMemsetAsync(c.d_lock, 0, sizeof(unsigned) * (size_t)n_lock, st));
    while (lock_enqueued < n_lock) {
        const int hi = std::min(n_lock, lock_enqueued + kLockChunk);
        for (int j = lock_enqueued; j < hi; j++) {
            ap.round = (int)((rounds + j) & 0x3fffffff);
            ap.lockstep = 1 + j;
            launch_advance();
            tpp.lock_shades = c.d_lock;
            tpp.lock_round = j;
            launch_trace();
        }
        HIP_TRY(hipGetLastError());
        lock_enqueued = hi;
        if (hi < n_lock) {  // (more than one chunk: max_bounces >= 15)
            unsigned last = 1u;
            HIP_TRY(hipMemcpyAsync(&last, c.d_lock + (hi - 1), sizeof(unsigned), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (last == 0u && hi - 1 >= 1) break;  // that round shaded nothing: the render is over (render.cuh:436)
        }
    }
    return 0;
}

// ---- after the frame's last event: the lockstep rounds that ran, the counters, the times, the stats
int FrameRun::frame_stats(rt_stats *stats) {
    if (ran_lockstep) {  // rounds that ran: up to and including the first one (after the generating round) that shaded nothing
        std::vector<unsigned> h_lock((size_t)lock_enqueued);
        HIP_TRY(hipMemcpy(h_lock.data(), c.d_lock, sizeof(unsigned) * (size_t)lock_enqueued, hipMemcpyDeviceToHost));
        int ran = lock_enqueued;
        for (int j = 1; j < lock_enqueued; j++)
            if (h_lock[(size_t)j] == 0u) {
                ran = j + 1;
                break;
            }
        rounds += ran;
    }
#ifdef RT_TRACE_PROFILE
    if (report_trace_profile(tpp.prof)) return 1;
#endif
    float ms_total = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms_total, ev_start, ev_stop));
    DCounters h_final{};
    HIP_TRY(hipMemcpy(&h_final, c.d_ctr, sizeof(DCounters), hipMemcpyDeviceToHost));
    std::vector<DWaveRow> h_rows((size_t)c.n_rows);
    HIP_TRY(hipMemcpy(h_rows.data(), c.d_rows, sizeof(DWaveRow) * (size_t)c.n_rows, hipMemcpyDeviceToHost));
    unsigned long long fin[C_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (const DWaveRow &r : h_rows)
        for (int k = 0; k < C_COUNT; k++) fin[k] += r.c[k];
    const std::vector<hipEvent_t> &evs = c.timing_events;
    double t_adv = 0, t_ch = 0;
    long long n_sampled = (long long)(ev_used / 4);
    for (size_t q = 0; q + 3 < ev_used; q += 4) {
        float ms;
        HIP_TRY(hipEventElapsedTime(&ms, evs[q], evs[q + 1]));
        t_adv += ms;
        HIP_TRY(hipEventElapsedTime(&ms, evs[q + 1], evs[q + 2]));
        t_ch += ms;
        HIP_TRY(hipEventElapsedTime(&ms, evs[q + 2], evs[q + 3]));  // (an empty bracket: asked for as before, not used)
    }
    if (!finished) return fail("rt_render_shard: round limit reached before the path pool drained");
    if (!stats) return 0;
    memset(stats, 0, sizeof(*stats));
    stats->camera_rays = (int64_t)fin[C_CAMERA];
    stats->shade_events = (int64_t)fin[C_SHADE];
    stats->closest_rays = (int64_t)fin[C_CLOSEST];
    stats->any_rays = (int64_t)fin[C_ANY];
    stats->emission_adds = (int64_t)fin[C_EMIT];
    stats->shadow_adds = (int64_t)fin[C_SHADOW_ADD];
    stats->rr_draws = (int64_t)fin[C_RR];
    stats->iterations = rounds;
    stats->bvh_nodes = scene->n_nodes;
    stats->bvh_depth = scene->max_depth;
    stats->seconds_render = ms_total * 1e-3;
    stats->seconds_rng_init = rng_seconds;
    // sampled every fourth round (run_rounds); scaled to all rounds (average launch duration x launches)
    double scale_up = n_sampled > 0 ? (double)rounds / (double)n_sampled : 0.0;
    stats->seconds_trace = t_ch * 1e-3 * scale_up;
    stats->seconds_reference_tree = ref_tree_seconds;
    stats->seconds_advance = t_adv * 1e-3 * scale_up;
    stats->launches_trace = rounds;
    stats->reserved[0] = n_sampled;
    if (persistent) {  // the frame's dominant kernel is the one k_paths launch
        stats->seconds_trace = ms_paths * 1e-3;
        stats->seconds_advance = 0.0;
        stats->launches_trace = 1;
        stats->reserved[0] = 1;
        stats->reserved[1] = 1 + slot_chunk + ((int64_t)slot_head << 32) + ((int64_t)(ran_bg ? 1 : 0) << 48);
        stats->reserved[2] = top_records_in_lds;
    }
    rare_path_counters(h_final.vstat, &stats->reserved[4]);
    return 0;
}

// The prepass of a counted frame on `st`, in the context's scratch (the caller holds c.busy): the (first, count) pairs are checked
// and the offenders counted before anything is written; then the prefix sum of the counts into c.d_counts_offset, the caller's
// d_samples add, and the sum of the counts into *total (held to the camera-ray range of a frame).
static int counts_prepass(Context &c, const CountsFrame &cf, int n_pixels, uint32_t stride, hipStream_t st, long long *total) {
    const int n_tiles = (n_pixels + kCountsTile - 1) / kCountsTile;
    if (c.counts_pixels < (size_t)n_pixels) {
        HIP_TRY(hipStreamSynchronize(st));
        (void)hipFree(c.d_counts_offset);
        (void)hipFree(c.d_counts_words);
        c.d_counts_offset = nullptr;
        c.d_counts_words = nullptr;
        c.counts_pixels = 0;
        HIP_TRY(hipMalloc((void **)&c.d_counts_offset, sizeof(uint32_t) * ((size_t)n_pixels + 1)));
        HIP_TRY(hipMalloc((void **)&c.d_counts_words, sizeof(unsigned long long) * ((size_t)n_tiles + 2)));
        c.counts_pixels = (size_t)n_pixels;
    }
    HIP_TRY(hipMemsetAsync(c.d_counts_words, 0, sizeof(unsigned long long) * 2, st));
    hipLaunchKernelGGL(k_counts_sums, dim3(n_tiles), dim3(256), 0, st, cf.d_first, cf.d_count, n_pixels, stride, c.d_counts_words);
    hipLaunchKernelGGL(k_counts_scan, dim3(1), dim3(256), 0, st, c.d_counts_words, n_tiles);
    HIP_TRY(hipGetLastError());
    unsigned long long *h = (unsigned long long *)&c.h_ctr[1];  // (pinned; the frame's own use of the ring starts after this)
    static_assert(sizeof(DCounters) >= 2 * sizeof(unsigned long long), "two words of staging");
    HIP_TRY(hipMemcpyAsync(h, c.d_counts_words, sizeof(unsigned long long) * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h[0])
        return fail("rt_render_shard: " + std::to_string(h[0]) + " pixel(s) with count < 0, first < 0 or first + count > sample_stride (" + std::to_string(stride) + ")");
    if ((long long)h[1] + 13LL * kW >= (1LL << 31))
        return fail("rt_render_shard: the counts add up to " + std::to_string(h[1]) + " camera rays, beyond the int32 camera-ray range of one call");
    *total = (long long)h[1];
    if (h[1] == 0) return 0;  // (nothing to add to d_samples either)
    hipLaunchKernelGGL(k_counts_offsets, dim3(n_tiles), dim3(256), 0, st, cf.d_count, n_pixels, (const unsigned long long *)c.d_counts_words, c.d_counts_offset,
                       cf.d_samples);
    HIP_TRY(hipGetLastError());
    return 0;
}

int render_shard_impl(const rt_scene *scene, const rt_camera *camera, int width, int height, int spp,
                      int max_bounces, uint64_t seed, int shard_index, int shard_count, uint32_t flags,
                      float *d_sum, hipStream_t st, rt_stats *stats, int ctx_lane = 0, const RayFrame *rays = nullptr,
                      const CountsFrame *counts = nullptr) {
    if (!scene || (!camera && !rays) || !d_sum) return fail("rt_render_shard: null argument");
    if (width <= 0 || height <= 0 || spp <= 0 || max_bounces < 0) return fail("rt_render_shard: bad dimensions");
    if (max_bounces > (1 << 24)) return fail("rt_render_shard: max_bounces exceeds 16777216");
    if (shard_count <= 0 || kW % shard_count != 0 || shard_index < 0 || shard_index >= shard_count)
        return fail("rt_render_shard: shard_count must divide 1048576 and 0 <= shard_index < shard_count");
    if ((long long)width * height > (long long)(0x7fffffff / 3))  // framebuffer values are indexed with 32 bits
        return fail("rt_render_shard: width*height exceeds 715827882 pixels");
    // (camera rays start at lookfrom: camera.cuh:22-26; a table's origins: rt_render_rays_*'s prepass has seen to them)
    if (!rays)
        if (int rc = ensure_origin_radius(scene, camera->lookfrom)) return rc;
    // RT_FLAG_RNG_PER_SAMPLE: this rank renders the whole frame at num_samples / shard_count samples per pixel with ALL W
    // slots; camera ray `cid` of the rank has the global key cid * shard_count + shard_index, so the keys of a pixel's
    // samples are the same set whatever the shard count (see AdvanceParams)
    const bool per_sample = (flags & RT_FLAG_RNG_PER_SAMPLE) != 0;
    const HitMode mode = hit_mode(flags, per_sample);
    if (mode.literal && per_sample) return fail("rt_render_shard: RT_FLAG_REFERENCE_WALK is a parity mode and RT_FLAG_RNG_PER_SAMPLE is not: pick one");
    if (refuse_both_hit_flags("rt_render_shard", flags)) return 1;
    if (per_sample) {
        if (spp % shard_count != 0) return fail("rt_render_shard: RT_FLAG_RNG_PER_SAMPLE needs num_samples divisible by shard_count");
        spp /= shard_count;
    }
    // (a counted frame's camera rays are the sum of its counts: known, and held to the same range, after the prepass below)
    long long cam_end = rays ? rays->n_rays : counts ? 0 : (long long)width * height * spp;
    if (cam_end + 13LL * kW >= (1LL << 31))  // the reference's int32 camera_ray ids (render.cuh:370-371,440)
        return fail("rt_render_shard: width*height*spp exceeds the reference's int32 camera-ray range");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != scene->device) return fail("rt_render_shard: scene was created on another device");
    double ref_tree_seconds = 0.0;
    if (mode.ref_tree()) {
        bool built = false;
        if (ensure_ref_tree(scene, &built)) return 1;
        if (built) ref_tree_seconds = scene->build_seconds_ref;  // (this call paid for it)
    }
    const int n = per_sample ? kW : kW / shard_count;
    const int slot_lo = per_sample ? 0 : shard_index * n;
    Context *cp = nullptr;
    if (get_context(n, ctx_lane, &cp)) return 1;
    Context &c = *cp;
    std::lock_guard<std::mutex> busy_lock(c.busy);  // concurrent callers with the same (device, n) queue up here
    FrameRun f{c, scene, rays, st, d_sum, flags, per_sample, mode};
    f.ref_tree_seconds = ref_tree_seconds;
    if (counts) {
        if (int rc = counts_prepass(c, *counts, width * height, (uint32_t)spp, st, &cam_end)) return rc;
        if (cam_end == 0) {  // nothing to render: no event, nothing written
            if (stats) {
                memset(stats, 0, sizeof(*stats));
                stats->bvh_nodes = scene->n_nodes;
                stats->bvh_depth = scene->max_depth;
            }
            return 0;
        }
        f.counted = true;
        f.counts_src.offset = c.d_counts_offset;
        f.counts_src.first = counts->d_first;
        f.counts_src.stride = (uint32_t)spp;
        f.counts_src.n_pixels = width * height;
    }
    if (ensure_rng(c, seed, slot_lo, st, &f.rng_seconds)) return 1;

    f.sc = scene->dev();
    if (!rays) memcpy(&f.cam, camera, sizeof(Camera));
    f.counts_src.cam = f.cam;
    {
        DCounters zero{};
        zero.last_live_round = -1;
        c.h_ctr[0] = zero;  // pinned staging
        HIP_TRY(hipMemcpyAsync(c.d_ctr, &c.h_ctr[0], sizeof(DCounters), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(c.d_rows, 0, sizeof(DWaveRow) * (size_t)c.n_rows, st));  // (n / 64 rows of 64 bytes: 1 MB for the full pool)
        HIP_TRY(hipStreamSynchronize(st));  // h_ctr[0] is reused as a snapshot slot below
    }
    f.stack_cap = lds_stack_cap(scene, kLdsStack);
    f.lds_bytes = sizeof(int) * (size_t)kBlock * (size_t)(f.stack_cap + 2);  // stack (+ 1 row: push_if) + pending
    // one buffer serves the context's k_trace and k_paths grids (never in flight together); k_paths keeps fewer
    // entries in LDS, so it needs the deeper overflow
    // (the literal walk of the reference's tree -- depth <= 30 -- borrows the lane's stack: reference_walk)
    const int stack_need = std::max(scene->stack_bound, mode.ref_tree() ? 32 : 0);
    if (ensure_overflow(c.d_over, c.over_levels, stack_need - std::min(f.stack_cap, lds_stack_cap(scene, kPathsLdsStack)))) return 1;
    // Slots of this shard that ever get a camera ray: slot s serves the camera rays s, s + W, ..., so in a frame of fewer than
    // W camera rays the slots from cam_end on never do anything -- the kernels of such a frame (it is nothing but the
    // lockstep rounds: 256 x 256 x 4 uses a quarter of the slots) are launched over the live slots only.  Frames of more
    // than one generation: all n.  (Per-sample streams: a lane draws its camera rays whatever its slot: all n.)
    const int n_live = per_sample ? n : (int)std::max<long long>(1, std::min<long long>(n, cam_end - (long long)slot_lo));
    hipLaunchKernelGGL(k_pool_init, dim3(grid_for(n_live)), dim3(kBlock), 0, st, c.pools, n_live, max_bounces);
    HIP_TRY(hipGetLastError());

    AdvanceParams &ap = f.ap;
    ap.n = n_live;
    ap.slot_lo = slot_lo;
    ap.width = width;
    ap.height = height;
    ap.spp = spp;
    ap.max_bounces = max_bounces;
    ap.cam_end = cam_end;
    ap.last_gen = per_sample ? 0x7fffffff : (int)((cam_end + kW - 1) / kW) - 1;  // (per-sample streams: no lockstep final generation)
    ap.per_sample = per_sample ? 1 : 0;
    ap.key_mul = per_sample ? shard_count : 1;
    ap.key_add = per_sample ? shard_index : 0;
    ap.seed_lo = (uint32_t)seed;
    ap.seed_hi = (uint32_t)(seed >> 32);
    ap.batch_mask = 7;  // (round and lockstep start at 0)
    ap.fb_fixed = (flags & kFlagFixedFb) ? 1 : 0;
    ap.w_over_spp = (kW % spp == 0 && !rays && !counts) ? kW / spp : 0;  // (the pixel stepping is the camera frames')
    ap.dpx = ap.w_over_spp % width;
    ap.dpy = (ap.w_over_spp > 0 && width < 32768 && height < 32768) ? ap.w_over_spp / width : -1;
    // The pixels whose camera rays can hit something (rt_background.h): k_paths<PathsBg> / k_paths<PathsChunkedBg> make no ray outside them.  Per
    // call, from the bounds of the records as they are now (after a refit, a rebuild or an edit: the new ones) and the radius they
    // are padded for.  Camera frames of 4-wide scenes; the whole frame otherwise, and with RT_BG_SKIP=0 (an experiment knob).
    ap.bg_x0 = ap.bg_y0 = 0;
    ap.bg_w = width;
    ap.bg_h = height;
    if (!rays && scene->wide) {
        bool skip = true;
        if (const char *e = knob("RT_BG_SKIP")) skip = atoi(e) != 0;
        std::lock_guard<std::mutex> pad_lock(scene->pad_mutex);  // (h_quads and origin_radius: their writers hold it)
        if (skip && scene->h_quads.size() >= 2) {
            float lo[3], hi[3];
            rtbg::root_bounds(scene->h_quads.data(), (int)rtbvh::kNoChild, lo, hi);  // (no child: lo > hi, the empty rectangle)
            const rtbg::Rect r = rtbg::background_rect((const float *)camera, width, height, lo, hi, scene->origin_radius);
            ap.bg_x0 = r.x0;
            ap.bg_y0 = r.y0;
            ap.bg_w = r.x1 - r.x0;
            ap.bg_h = r.y1 - r.y0;
        }
    }
    f.lds_tables = scene->n_mats <= kLdsTable && scene->n_lights <= kLdsTable;

    HIP_TRY(hipEventCreate(&f.ev_start));
    HIP_TRY(hipEventCreate(&f.ev_stop));
    HIP_TRY(hipEventRecord(f.ev_start, st));

    // persistent trace kernels: as many workgroups as the chip keeps resident (never more than the
    // advance grid, whose wave count sizes the counter rows)
    int occ_c = 0;
    HIP_TRY(hipDeviceGetAttribute(&f.cus, hipDeviceAttributeMultiprocessorCount, dev));
    f.trace = trace_kernel(mode.literal, mode.verify, scene->wide);
    // (every k_trace build runs 8 waves per SIMD without static LDS: the grid does not depend on which one this is)
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_c, f.trace, kBlock, f.lds_bytes));
    int per_cu = std::max(1, occ_c);
    if (const char *e = knob("RT_TRACE_BLOCKS_PER_CU")) per_cu = std::max(1, std::min(per_cu, atoi(e)));
    f.grid_trace = dim3(std::min(grid_for(n_live), std::max(1, f.cus * per_cu)));
    f.tpp.total = n_live;
    f.tpp.fb = d_sum;
    f.tpp.rows = c.d_rows;
    f.tpp.debug_no_deposit = (flags & 0x100u) ? 1 : 0;
    f.tpp.fb_fixed = (flags & kFlagFixedFb) ? 1 : 0;
    f.tpp.vstat = &c.d_ctr->vstat[0];
#ifdef RT_TRACE_PROFILE
    HIP_TRY(hipMalloc((void **)&f.tpp.prof, sizeof(unsigned long long) * 16));
    HIP_TRY(hipMemset(f.tpp.prof, 0, sizeof(unsigned long long) * 16));
#endif
    // ONE persistent launch, or -- RT_PERSISTENT=0 -- the round-per-launch pipeline that the lockstep final generation also uses
    if (const char *e = knob("RT_PERSISTENT")) f.persistent = atoi(e) != 0;
    if (rays && !scene->wide) f.persistent = false;  // (k_paths<PathsRays> walks 4-wide nodes; the round pipeline walks either format)
    if (per_sample && !f.persistent) return fail("rt_render_shard: RT_FLAG_RNG_PER_SAMPLE runs on the persistent kernel only");
    if (f.persistent ? f.run_persistent() : f.run_rounds()) return 1;
    if (f.run_lockstep()) return 1;
    HIP_TRY(hipEventRecord(f.ev_stop, st));
    HIP_TRY(hipEventSynchronize(f.ev_stop));
    return f.frame_stats(stats);
}

// A persistent query-style grid: what the device holds at once (never more lanes than the overflow stacks' columns) or n needs.
template <class KERNEL>
static int resident_grid(KERNEL kernel, size_t lds_bytes, int cus, int n, int *grid) {
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, lds_bytes));
    const int resident = std::min(std::max(per_cu, 1) * std::max(cus, 1), kOverStride / kBlock);
    *grid = std::max(1, std::min(resident, (int)(((size_t)n + kBlock - 1) / kBlock)));
    return 0;
}

// The walk of a query on `st`, after whatever the entry point checks: `qp` arrives with the rays, the caller's exclusions and
// the answers' buffers, all on the device.  The inverse leaf order (made by the first any-hit call that excludes), the
// overflow stacks, the kernel for the scene and the hit definition, the launch sized from the device, one wait, and the
// rare-path counters of this call into `counters_out`.  The caller holds the scene's query lock, has entered the scene's
// device and has zeroed q.d_words->vstat on `st` (validate_table does).
using QueryKernel = decltype(&k_query<Q_CLOSEST, false, false, false>);
template <int KIND>
static QueryKernel query_kernel(bool literal, bool verify, bool wide) {
    if (literal) return k_query<KIND, false, true, false>;
    if (verify) return wide ? k_query<KIND, true, false, true> : k_query<KIND, false, false, true>;
    return wide ? k_query<KIND, true, false, false> : k_query<KIND, false, false, false>;
}
template <int KIND>
static int run_query(const rt_scene *scene, HitMode mode, QueryParams qp, hipStream_t st, int64_t counters_out[3]) {
    rt_scene::QueryState &q = scene->query;
    if (KIND == Q_ANY && qp.excluded && !q.d_inverse && scene->n_tris > 0) {
        HIP_TRY(hipMalloc((void **)&q.d_inverse, sizeof(int) * (size_t)scene->n_tris));
        hipLaunchKernelGGL(k_query_inverse, dim3((scene->n_tris + 255) / 256), dim3(256), 0, st, scene->d_order, scene->n_tris, q.d_inverse);
    }
    const int stack_cap = lds_stack_cap(scene, kLdsStack);
    if (ensure_overflow(q.d_over, q.over_levels, std::max(scene->stack_bound, 32) - stack_cap)) return 1;
    qp.n_tris = scene->n_tris;
    qp.inverse = q.d_inverse;
    qp.vstat = q.d_words->vstat;
    const QueryKernel kernel = query_kernel<KIND>(mode.literal, mode.verify, scene->wide);
    const size_t lds = sizeof(int) * kBlock * (size_t)(stack_cap + 1);
    int grid = 0;
    if (resident_grid(kernel, lds, q.cus, qp.n, &grid)) return 1;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, st, scene->dev(), qp, stack_cap, q.d_over);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(q.h_words->vstat, q.d_words->vstat, sizeof(q.h_words->vstat), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    rare_path_counters(q.h_words->vstat, counters_out);
    return 0;
}

// rt_query_closest_device / rt_query_any_device.  Every kernel of a query is ordered on `st`; the host waits twice: for the
// table's validation (validate_table: the directions, and the origin radius the 4-wide records must be padded for) and for
// the walk.
template <int KIND>
static int query_impl(const rt_scene *scene, uint32_t flags, int n, const float *d_o, const float *d_d, const float *d_tmax,
                      const int32_t *d_excluded, int32_t *d_out_i, float *d_t, float *d_u, float *d_v, hipStream_t st) {
    const std::string w(KIND == Q_CLOSEST ? "rt_query_closest_device" : "rt_query_any_device");
    if (!scene) return fail(w + ": null scene");
    if (n < 0 || n > (1 << 30)) return fail(w + ": n = " + std::to_string(n) + " is outside 0 .. 2^30");
    if (flags & ~(uint32_t)(RT_FLAG_REFERENCE_WALK | RT_FLAG_WATERTIGHT)) return fail(w + ": flags other than RT_FLAG_REFERENCE_WALK / RT_FLAG_WATERTIGHT");
    if (refuse_both_hit_flags(w, flags)) return 1;
    if (n > 0 && (!d_o || !d_d || !d_out_i))
        return fail(w + ": null " + (!d_o ? "d_origin_xyz" : !d_d ? "d_dir_xyz" : KIND == Q_CLOSEST ? "d_hit_tri" : "d_occluded"));
    if (n == 0) return 0;
    const HitMode mode = hit_mode(flags);
    rt_scene::QueryState &q = scene->query;
    std::lock_guard<std::mutex> lock(q.mutex);
    DeviceGuard dev;
    if (dev.enter(scene->device)) return 1;
    if (ensure_query_state(scene, false)) return 1;
    if (mode.ref_tree() && ensure_ref_tree(scene)) return 1;
    if (int rc = validate_table(scene, w, n, d_o, d_d, nullptr, 0, st)) return rc;
    QueryParams qp{};
    qp.n = n;
    qp.o3 = d_o;
    qp.d3 = d_d;
    qp.tmax = d_tmax;
    qp.excluded = d_excluded;
    qp.out_i = d_out_i;
    qp.out_t = d_t;
    qp.out_u = d_u;
    qp.out_v = d_v;
    return run_query<KIND>(scene, mode, qp, st, q.counters);
}

// rt_trace_closest_flags / rt_trace_any_flags, the host-pointer form of the queries (the entry points have checked their
// pointers): the caller's arrays go to the device as they are, the walk is run_query's on the null stream, the answers come
// back.  The uploads are waited for before the walk, the copies back are synchronous.  What differs from query_impl: the
// origins' radius is taken on the host, the directions are the caller's to keep within the header's precondition (no
// validate_table: nothing is refused for them), and the counters of the call stay local -- rt_query_last_counters speaks
// of the last QUERY.
template <int KIND>
static int trace_hook(const rt_scene *scene, uint32_t flags, int n, const float *origin_xyz, const float *dir_xyz, const float *tmax,
                      const int32_t *excluded_tri, int32_t *out_i, float *t, float *u, float *v) {
    const HitMode mode = hit_mode(flags);
    rt_scene::QueryState &q = scene->query;
    std::lock_guard<std::mutex> lock(q.mutex);
    DeviceGuard dev;
    if (dev.enter(scene->device)) return 1;
    if (ensure_query_state(scene, false)) return 1;
    if (mode.ref_tree() && ensure_ref_tree(scene)) return 1;
    {
        float need[3] = {0.f, 0.f, 0.f};  // the 4-wide records must be padded for these origins (ensure_origin_radius)
        for (int i = 0; i < n; i++)
            for (int a = 0; a < 3; a++)
                if (std::isfinite(origin_xyz[3 * (size_t)i + a])) need[a] = std::max(need[a], std::fabs(origin_xyz[3 * (size_t)i + a]));
        if (int rc = ensure_origin_radius(scene, need)) return rc;
    }
    DevScope tmp;
    QueryParams qp{};
    qp.n = n;
    if (stage(tmp, origin_xyz, 3 * (size_t)n, nullptr, qp.o3) || stage(tmp, dir_xyz, 3 * (size_t)n, nullptr, qp.d3) ||
        stage(tmp, tmax, (size_t)n, nullptr, qp.tmax) || (KIND == Q_ANY && stage(tmp, excluded_tri, (size_t)n, nullptr, qp.excluded)))
        return 1;
    if (tmp.alloc(qp.out_i, (size_t)n)) return 1;
    if (KIND == Q_CLOSEST && (tmp.alloc(qp.out_t, (size_t)n) || tmp.alloc(qp.out_u, (size_t)n) || tmp.alloc(qp.out_v, (size_t)n))) return 1;
    HIP_TRY(hipMemsetAsync(q.d_words, 0, sizeof(QueryWords), nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));  // (the caller's arrays have been read)
    int64_t counters[3];
    if (int rc = run_query<KIND>(scene, mode, qp, nullptr, counters)) return rc;
    HIP_TRY(hipMemcpy(out_i, qp.out_i, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    if (KIND == Q_CLOSEST) {
        HIP_TRY(hipMemcpy(t, qp.out_t, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(u, qp.out_u, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(v, qp.out_v, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    }
    return 0;
}
// rt_trace_closest[_flags] and rt_trace_any[_flags]: the pointer checks, then the hook
static int trace_closest_impl(const rt_scene *scene, uint32_t flags, int n, const float *origin_xyz, const float *dir_xyz, const float *tmax,
                              int32_t *hit_tri, float *t, float *u, float *v) {
    if (!scene || n < 0 || (n > 0 && (!origin_xyz || !dir_xyz || !tmax || !hit_tri || !t || !u || !v)))
        return fail("rt_trace_closest: bad argument");
    if (n == 0) return 0;
    return trace_hook<Q_CLOSEST>(scene, flags, n, origin_xyz, dir_xyz, tmax, nullptr, hit_tri, t, u, v);
}
static int trace_any_impl(const rt_scene *scene, uint32_t flags, int n, const float *origin_xyz, const float *dir_xyz, const float *tmax,
                          const int32_t *excluded_tri, int32_t *occluded) {
    if (!scene || n < 0 || (n > 0 && (!origin_xyz || !dir_xyz || !tmax || !excluded_tri || !occluded)))
        return fail("rt_trace_any: bad argument");
    if (n == 0) return 0;
    return trace_hook<Q_ANY>(scene, flags, n, origin_xyz, dir_xyz, tmax, excluded_tri, occluded, nullptr, nullptr, nullptr);
}

// rt_render_rays_device / rt_render_rays_fixed_device: host-side argument checks, the table's validation on the device
// (validate_table; nothing is written before it has passed), then the frame through render_shard_impl.
static int render_rays_impl(const rt_scene *scene, int64_t n_rays, const float *d_o, const float *d_d, const int32_t *d_pixel,
                            int rays_per_pixel, int n_pixels, int max_bounces, uint64_t seed, uint32_t flags, float *d_sum,
                            hipStream_t st, rt_stats *stats) {
    const std::string w((flags & kFlagFixedFb) ? "rt_render_rays_fixed_device" : "rt_render_rays_device");
    if (check_table_pointers(w, scene, d_o, d_d, d_sum, "sum buffer")) return 1;
    if (flags & RT_FLAG_REFERENCE_WALK) return fail(w + ": RT_FLAG_REFERENCE_WALK is not supported for ray tables");
    if (flags & RT_FLAG_RNG_PER_SAMPLE) return fail(w + ": RT_FLAG_RNG_PER_SAMPLE is not supported for ray tables");
    if (flags & ~(uint32_t)(RT_FLAG_WATERTIGHT | RT_FLAG_TIME_KERNELS | kFlagFixedFb)) return fail(w + ": flags other than RT_FLAG_WATERTIGHT / RT_FLAG_TIME_KERNELS");
    if (check_table_args(w, n_rays, "the reference's int32 camera-ray range", n_pixels, &max_bounces)) return 1;
    KeyedRayTable rows;  // (row c has the key c: only its rays_per_pixel is used)
    if (check_key_range(w, "ray", n_rays, 0, 1, d_o, d_d, d_pixel, rays_per_pixel, n_pixels, &rows)) return 1;
    DeviceGuard dev;
    if (dev.enter(scene->device)) return 1;
    {  // (the prepass borrows the scene's query scratch under its lock)
        std::lock_guard<std::mutex> lock(scene->query.mutex);
        if (ensure_query_state(scene, false)) return 1;
        if (int rc = validate_table(scene, w, (int)n_rays, d_o, d_d, d_pixel, n_pixels, st)) return rc;
    }
    RayFrame rays;
    rays.table = RayTable{d_o, d_d, d_pixel};
    rays.n_rays = n_rays;
    return render_shard_impl(scene, nullptr, n_pixels, 1, (int)rows.rays_per_pixel, max_bounces, seed, 0, 1, flags, d_sum, st, stats, 0, &rays);
}

// rt_render_rays_keyed_device / rt_render_rays_keyed_fixed_device: render_rays_impl's checks and validation, the checks of
// the keys, then the frame through render_shard_impl in the per-sample mode (full pool, no parking, no lockstep final
// generation) with k_paths<PathsKeyed>: row c's stream is rng_sample_stream(seed, key_first + c * key_stride).
static int render_rays_keyed_impl(const rt_scene *scene, int64_t n_rays, const float *d_o, const float *d_d, const int32_t *d_pixel,
                                  int rays_per_pixel, int n_pixels, int max_bounces, uint64_t seed, uint64_t key_first,
                                  uint32_t key_stride, uint32_t flags, float *d_sum, hipStream_t st, rt_stats *stats) {
    const std::string w((flags & kFlagFixedFb) ? "rt_render_rays_keyed_fixed_device" : "rt_render_rays_keyed_device");
    if (check_table_pointers(w, scene, d_o, d_d, d_sum, "sum buffer")) return 1;
    if (flags & RT_FLAG_REFERENCE_WALK) return fail(w + ": RT_FLAG_REFERENCE_WALK is not supported for keyed ray tables");
    // (RT_FLAG_RNG_PER_SAMPLE and RT_FLAG_WATERTIGHT are what the mode is: accepted, and change nothing)
    if (flags & ~(uint32_t)(RT_FLAG_RNG_PER_SAMPLE | RT_FLAG_WATERTIGHT | RT_FLAG_TIME_KERNELS | kFlagFixedFb))
        return fail(w + ": flags other than RT_FLAG_RNG_PER_SAMPLE / RT_FLAG_WATERTIGHT / RT_FLAG_TIME_KERNELS");
    if (check_table_args(w, n_rays, "the int32 camera-ray range of one call", n_pixels, &max_bounces)) return 1;
    RayFrame rays;
    rays.table = RayTable{};
    rays.n_rays = n_rays;
    rays.keyed = true;
    if (check_key_range(w, "key", n_rays, key_first, key_stride, d_o, d_d, d_pixel, rays_per_pixel, n_pixels, &rays.keyed_table)) return 1;
    if (!scene->wide) return fail(w + ": keyed ray tables need the 4-wide tree (the scene was created with RT_BVH_WIDE=0)");
    if (const char *e = knob("RT_PERSISTENT"))
        if (atoi(e) == 0) return fail(w + ": keyed ray tables run on the persistent kernel only (RT_PERSISTENT=0 is set)");
    DeviceGuard dev;
    if (dev.enter(scene->device)) return 1;
    {  // (the prepass borrows the scene's query scratch under its lock)
        std::lock_guard<std::mutex> lock(scene->query.mutex);
        if (ensure_query_state(scene, false)) return 1;
        if (int rc = validate_table(scene, w, (int)n_rays, d_o, d_d, d_pixel, n_pixels, st)) return rc;
    }
    const uint32_t mode = (flags & (RT_FLAG_TIME_KERNELS | kFlagFixedFb)) | RT_FLAG_RNG_PER_SAMPLE;
    if (int rc = render_shard_impl(scene, nullptr, n_pixels, 1, (int)rays.keyed_table.rays_per_pixel, max_bounces, seed, 0, 1, mode, d_sum, st, stats, 0, &rays)) {
        fail(w + ": " + g_last_error);  // (what the frame itself refused, under this entry point's name)
        return rc;
    }
    return 0;
}

// rt_render_aov_fixed / rt_render_aov_rays_fixed_device, their followed forms (rt_render_aov_follow_*) / rt_render_motion: the entry points check their arguments (and, for a table, run the
// device prepasses) and hand the ray source over; this is the one body behind both -- the reference's tree where the hit
// definition needs it, the overflow stacks, the launch sized from the device, the kernel's time and the rare-path counters.
// The caller holds the scene's query lock and has entered the scene's device; q.d_words is zeroed on `st`.
template <class SRC>
using AovKernel = void (*)(DScene, SRC, AovParams, int, int *);
template <class SRC>
static AovKernel<SRC> aov_kernel(bool literal, bool verify, bool wide) {
    if (literal) return k_aov<SRC, false, true, false>;
    if (verify) return wide ? k_aov<SRC, true, false, true> : k_aov<SRC, false, false, true>;
    return wide ? k_aov<SRC, true, false, false> : k_aov<SRC, false, false, false>;
}
static int aov_flags(const std::string &w, uint32_t flags) {
    if (flags & ~(uint32_t)(RT_FLAG_WATERTIGHT | RT_FLAG_REFERENCE_WALK | RT_FLAG_TIME_KERNELS))
        return fail(w + ": flags other than RT_FLAG_WATERTIGHT / RT_FLAG_REFERENCE_WALK / RT_FLAG_TIME_KERNELS");
    return refuse_both_hit_flags(w, flags);
}
// The launch behind the AOV entry points and rt_render_motion: `kernel` is a stream-walker kernel, launch(grid, lds, stack_cap,
// overflow) enqueues it with its own parameters (which hold q.d_words->vstat), n is the number of rays.
template <class KERNEL, class LAUNCH>
static int walker_launch(const rt_scene *scene, const HitMode &mode, KERNEL kernel, int n, hipStream_t st, rt_stats *stats, LAUNCH launch) {
    rt_scene::QueryState &q = scene->query;
    if (mode.ref_tree() && ensure_ref_tree(scene)) return 1;
    const int stack_cap = lds_stack_cap(scene, kLdsStack);
    if (ensure_overflow(q.d_over, q.over_levels, std::max(scene->stack_bound, 32) - stack_cap)) return 1;
    const size_t lds = sizeof(int) * kBlock * (size_t)(stack_cap + 1);
    int grid = 0;
    if (resident_grid(kernel, lds, q.cus, n, &grid)) return 1;
    HIP_TRY(hipEventRecord(q.ev_a, st));
    launch(grid, lds, stack_cap, q.d_over);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(q.ev_b, st));
    // (the rare-path counters and, behind them, the chain rays of k_aov_follow: zero after every other kernel)
    static_assert(offsetof(QueryWords, chain_rays) == offsetof(QueryWords, vstat) + sizeof(QueryWords::vstat), "one copy");
    HIP_TRY(hipMemcpyAsync(q.h_words->vstat, q.d_words->vstat, sizeof(q.h_words->vstat) + sizeof(q.h_words->chain_rays), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, q.ev_a, q.ev_b));
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->camera_rays = n;
        stats->closest_rays = n + (long long)q.h_words->chain_rays;
        stats->bvh_nodes = scene->n_nodes;
        stats->bvh_depth = scene->max_depth;
        stats->seconds_render = ms * 1e-3;
        stats->seconds_trace = ms * 1e-3;
        stats->launches_trace = 1;
        rare_path_counters(q.h_words->vstat, &stats->reserved[4]);
    }
    return 0;
}
template <class SRC>
using AovFollowKernel = void (*)(DScene, SRC, AovParams, AovFollowParams, int, int *);
template <class SRC>
static AovFollowKernel<SRC> aov_follow_kernel(bool literal, bool verify, bool wide) {
    if (literal) return k_aov_follow<SRC, false, true, false>;
    if (verify) return wide ? k_aov_follow<SRC, true, false, true> : k_aov_follow<SRC, false, false, true>;
    return wide ? k_aov_follow<SRC, true, false, false> : k_aov_follow<SRC, false, false, false>;
}
// max_specular = 0: k_aov (the first-hit entry points, and the followed ones at a cap of 0); 1 .. RT_AOV_FOLLOW_MAX: k_aov_follow.
template <class SRC>
static int aov_launch(const rt_scene *scene, const SRC &src, int n, uint32_t flags, uint64_t seed, int max_specular, int64_t *d_aov,
                      int32_t *d_ids, hipStream_t st, rt_stats *stats) {
    const HitMode mode = hit_mode(flags);
    AovParams ap{};
    ap.n = n;
    ap.sums = (unsigned long long *)d_aov;
    ap.ids = d_ids;
    ap.vstat = scene->query.d_words->vstat;
    if (max_specular > 0) {
        AovFollowParams fp{};
        fp.seed_lo = (uint32_t)seed;
        fp.seed_hi = (uint32_t)(seed >> 32);
        fp.max_specular = max_specular;
        fp.chain_rays = &scene->query.d_words->chain_rays;
        const AovFollowKernel<SRC> kernel = aov_follow_kernel<SRC>(mode.literal, mode.verify, scene->wide);
        return walker_launch(scene, mode, kernel, n, st, stats, [&](int grid, size_t lds, int stack_cap, int *d_over) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, st, scene->dev(), src, ap, fp, stack_cap, d_over);
        });
    }
    const AovKernel<SRC> kernel = aov_kernel<SRC>(mode.literal, mode.verify, scene->wide);
    return walker_launch(scene, mode, kernel, n, st, stats, [&](int grid, size_t lds, int stack_cap, int *d_over) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, st, scene->dev(), src, ap, stack_cap, d_over);
    });
}
// the followed entry points' own check, after the argument checks they share with the first-hit ones
static int aov_follow_cap(const std::string &w, int max_specular) {
    if (max_specular < 0 || max_specular > RT_AOV_FOLLOW_MAX)
        return fail(w + ": max_specular = " + std::to_string(max_specular) + " is outside 0 .. RT_AOV_FOLLOW_MAX (" + std::to_string(RT_AOV_FOLLOW_MAX) + ")");
    return 0;
}

// `name`, max_specular: rt_render_aov_fixed (0) or rt_render_aov_follow_fixed
static int render_aov_impl(const char *name, const rt_scene *scene, const rt_camera *camera, int width, int height, int spp, uint64_t seed,
                           int shard_index, int shard_count, uint32_t flags, int max_specular, int64_t *d_aov, int32_t *d_ids,
                           hipStream_t st, rt_stats *stats) {
    const std::string w(name);
    if (!scene) return fail(w + ": null scene");
    if (!camera || !d_aov) return fail(w + ": null " + (!camera ? "camera" : "d_aov_fixed"));
    if (aov_flags(w, flags)) return 1;
    if (width < 1 || height < 1 || spp < 1)
        return fail(w + ": width, height and num_samples must be at least 1 (" + std::to_string(width) + " x " + std::to_string(height) + " x " + std::to_string(spp) + ")");
    if ((long long)width * height > (long long)(0x7fffffff / 3)) return fail(w + ": width*height exceeds 715827882 pixels");
    if ((long long)width * height * spp + 13LL * kW >= (1LL << 31)) return fail(w + ": width*height*num_samples exceeds the int32 camera-ray range");
    if (shard_count < 1 || shard_index < 0 || shard_index >= shard_count)
        return fail(w + ": shard_index = " + std::to_string(shard_index) + " is outside 0 .. shard_count - 1 (shard_count = " + std::to_string(shard_count) + ")");
    if (spp % shard_count != 0)
        return fail(w + ": num_samples = " + std::to_string(spp) + " is not divisible by shard_count = " + std::to_string(shard_count));
    if (aov_follow_cap(w, max_specular)) return 1;
    DeviceGuard dev;
    if (dev.enter(scene->device)) return 1;
    // (camera rays start at lookfrom: as render_shard_impl)
    if (int rc = ensure_origin_radius(scene, camera->lookfrom)) return rc;
    rt_scene::QueryState &q = scene->query;
    std::lock_guard<std::mutex> lock(q.mutex);
    if (ensure_query_state(scene, true)) return 1;
    HIP_TRY(hipMemsetAsync(q.d_words, 0, sizeof(QueryWords), st));
    AovCamera src{};
    memcpy(&src.cam, camera, sizeof(Camera));
    src.width = width;
    src.height = height;
    src.spp = (unsigned)(spp / shard_count);
    src.key_mul = (unsigned)shard_count;
    src.key_add = (unsigned)shard_index;
    src.seed_lo = (uint32_t)seed;
    src.seed_hi = (uint32_t)(seed >> 32);
    const int n = (int)((long long)width * height * (spp / shard_count));
    // the sample with G % num_samples == 0 has G % shard_count == 0: it is shard 0's
    return aov_launch(scene, src, n, flags, seed, max_specular, d_aov, shard_index == 0 ? d_ids : nullptr, st, stats);
}

// `name`, seed, max_specular: rt_render_aov_rays_fixed_device (no stream: 0, 0) or rt_render_aov_follow_rays_fixed_device
static int render_aov_rays_impl(const char *name, const rt_scene *scene, int64_t n_rays, const float *d_o, const float *d_d,
                                const int32_t *d_pixel, int rays_per_pixel, int n_pixels, uint64_t seed, uint64_t key_first,
                                uint32_t key_stride, uint32_t flags, int max_specular, int64_t *d_aov, int32_t *d_ids, hipStream_t st,
                                rt_stats *stats) {
    const std::string w(name);
    if (check_table_pointers(w, scene, d_o, d_d, d_aov, "d_aov_fixed")) return 1;
    if (aov_flags(w, flags)) return 1;
    if (d_ids && d_pixel) return fail(w + ": d_ids together with d_pixel (ids belong to the pixels of the key rule: pass d_pixel = NULL)");
    if (check_table_args(w, n_rays, "the int32 camera-ray range of one call", n_pixels, nullptr)) return 1;
    KeyedRayTable src;
    if (check_key_range(w, "key", n_rays, key_first, key_stride, d_o, d_d, d_pixel, rays_per_pixel, n_pixels, &src)) return 1;
    if (aov_follow_cap(w, max_specular)) return 1;
    DeviceGuard dev;
    if (dev.enter(scene->device)) return 1;
    std::lock_guard<std::mutex> lock(scene->query.mutex);
    if (ensure_query_state(scene, true)) return 1;
    if (int rc = validate_table(scene, w, (int)n_rays, d_o, d_d, d_pixel, n_pixels, st)) return rc;
    return aov_launch(scene, src, (int)n_rays, flags, seed, max_specular, d_aov, d_ids, st, stats);
}

// rt_render_motion: the AOV entry point's checks where they apply, the same query state and launch, k_motion's parameters.
using MotionKernel = void (*)(DScene, MotionParams, int, int *);
static MotionKernel motion_kernel(bool literal, bool verify, bool wide) {
    if (literal) return k_motion<false, true, false>;
    if (verify) return wide ? k_motion<true, false, true> : k_motion<false, false, true>;
    return wide ? k_motion<true, false, false> : k_motion<false, false, false>;
}
static int render_motion_impl(const rt_scene *scene, const rt_camera *camera, int width, int height, const rt_camera *prev_camera,
                              const float *d_prev_tris, uint32_t flags, float *d_motion, hipStream_t st, rt_stats *stats) {
    const std::string w("rt_render_motion");
    if (!scene) return fail(w + ": null scene");
    if (!camera || !prev_camera || !d_motion) return fail(w + ": null " + (!camera ? "camera" : !prev_camera ? "prev_camera" : "d_motion"));
    if (aov_flags(w, flags)) return 1;
    if (width < 1 || height < 1)
        return fail(w + ": width and height must be at least 1 (" + std::to_string(width) + " x " + std::to_string(height) + ")");
    if ((long long)width * height > (long long)(0x7fffffff / 3)) return fail(w + ": width*height exceeds 715827882 pixels");
    if ((uintptr_t)d_motion % 16) return fail(w + ": d_motion must be 16-byte aligned");
    DeviceGuard dev;
    if (dev.enter(scene->device)) return 1;
    if (int rc = ensure_origin_radius(scene, camera->lookfrom)) return rc;  // (camera rays start at lookfrom: as render_shard_impl)
    rt_scene::QueryState &q = scene->query;
    std::lock_guard<std::mutex> lock(q.mutex);
    if (ensure_query_state(scene, true)) return 1;
    HIP_TRY(hipMemsetAsync(q.d_words, 0, sizeof(QueryWords), st));
    const HitMode mode = hit_mode(flags);
    MotionParams mp{};
    memcpy(&mp.cam, camera, sizeof(Camera));
    tm_camera(prev_camera->lookfrom, width, height, &mp.prev);  // (rt_camera is twelve consecutive floats)
    mp.n = width * height;
    mp.width = width;
    mp.height = height;
    mp.prev_tris = d_prev_tris;
    mp.out = (float4 *)d_motion;
    mp.vstat = q.d_words->vstat;
    const MotionKernel kernel = motion_kernel(mode.literal, mode.verify, scene->wide);
    return walker_launch(scene, mode, kernel, mp.n, st, stats, [&](int grid, size_t lds, int stack_cap, int *d_over) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, st, scene->dev(), mp, stack_cap, d_over);
    });
}


// rt_render_counts_fixed: the host-side checks, then the frame through render_shard_impl in the per-sample mode as one more source
// of camera rays (CountsFrame): the prepass on the device, k_paths<PathsCounts>.
static int render_counts_impl(const rt_scene *scene, const rt_camera *camera, int width, int height, int sample_stride, const int32_t *d_first,
                              const int32_t *d_count, int max_bounces, uint64_t seed, uint32_t flags, int64_t *d_sum_fixed, int32_t *d_samples,
                              hipStream_t st, rt_stats *stats) {
    const std::string w("rt_render_counts_fixed");
    if (!scene) return fail(w + ": null scene");
    if (!camera || !d_count || !d_sum_fixed) return fail(w + ": null " + (!camera ? "camera" : !d_count ? "d_count" : "d_sum_fixed"));
    if (flags & RT_FLAG_REFERENCE_WALK) return fail(w + ": RT_FLAG_REFERENCE_WALK is not supported for counted frames");
    // (RT_FLAG_RNG_PER_SAMPLE and RT_FLAG_WATERTIGHT are what the mode is: accepted, and change nothing)
    if (flags & ~(uint32_t)(RT_FLAG_RNG_PER_SAMPLE | RT_FLAG_WATERTIGHT | RT_FLAG_TIME_KERNELS))
        return fail(w + ": flags other than RT_FLAG_RNG_PER_SAMPLE / RT_FLAG_WATERTIGHT / RT_FLAG_TIME_KERNELS");
    if (width < 1 || height < 1) return fail(w + ": width and height must be at least 1 (" + std::to_string(width) + " x " + std::to_string(height) + ")");
    if ((long long)width * height > (long long)(0x7fffffff / 3)) return fail(w + ": width*height exceeds 715827882 pixels");
    if (sample_stride < 1) return fail(w + ": sample_stride = " + std::to_string(sample_stride) + " is outside 1 .. 2147483647");
    if (max_bounces < 0 || max_bounces > (1 << 24)) return fail(w + ": max_bounces = " + std::to_string(max_bounces) + " is outside 0 .. 16777216");
    if (!scene->wide) return fail(w + ": counted frames need the 4-wide tree (the scene was created with RT_BVH_WIDE=0)");
    if (const char *e = knob("RT_PERSISTENT"))
        if (atoi(e) == 0) return fail(w + ": counted frames run on the persistent kernel only (RT_PERSISTENT=0 is set)");
    DeviceGuard dev;
    if (dev.enter(scene->device)) return 1;
    const CountsFrame counts{d_first, d_count, d_samples};
    const uint32_t mode = (flags & RT_FLAG_TIME_KERNELS) | kFlagFixedFb | RT_FLAG_RNG_PER_SAMPLE;
    if (int rc = render_shard_impl(scene, camera, width, height, sample_stride, max_bounces, seed, 0, 1, mode, (float *)d_sum_fixed, st, stats, 0, nullptr, &counts)) {
        fail(w + ": " + g_last_error);  // (what the frame itself refused, under this entry point's name)
        return rc;
    }
    return 0;
}
