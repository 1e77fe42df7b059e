// rt_stream_kernels.inc -- the kernels that walk a stream of rays: k_trace (the pools of a round), the query prepasses, the
// stream walker of every dense ray array with its four kernels, k_query (rays from device buffers: the queries and their
// host-pointer form, the trace hooks), k_aov (first-hit feature buffers), k_aov_follow (the same behind mirror and glass) and
// k_motion (rt_render_motion).  Included by rtcuda_amd.hip, once, after rt_walk.inc.
struct TraceParams {
    int total;             // number of slots
    int debug_no_deposit;  // perf experiments only: skip the framebuffer atomics
    int fb_fixed;          // framebuffer holds 64-bit fixed-point sums (see deposit())
    float *fb;             // raw-sum framebuffer
    DWaveRow *rows;        // counter rows
    unsigned long long *prof;  // RT_TRACE_PROFILE builds only
    // lockstep rounds: nothing to trace in a round that shaded nothing (see k_advance); null / 0 otherwise
    const unsigned int *lock_shades;
    int lock_round;
    unsigned long long *vstat;  // VERIFY builds: DCounters::vstat
};

// k_trace traces BOTH ray kinds of a round in one launch: the path ray of every live slot
// (closest hit, ch()) and the shadow ray of every slot that spawned one (any hit, ah()).  A lane
// carries its kind with its ray, so closest-hit and any-hit rays share waves; the two kinds differ
// only in what a triangle hit does and in how the finished ray is finalised.
// LDS layout (dynamic): [stack: (stack_cap + 1) x kBlock ints (push_if)][pending: kBlock ints]
// The register budget is 8 waves per SIMD (64 VGPRs).
// LITERAL (RT_FLAG_REFERENCE_WALK): a lane traverses its whole ray with reference_walk -- the scheduling around it
// (chunks, refill, finalisation) is unchanged, WIDE is not looked at.
// VERIFY (the default; off with RT_FLAG_WATERTIGHT): the product's walk with the reference's decisions -- see ref_visible.
template <bool WIDE, bool LITERAL = false, bool VERIFY = false>
__global__ void __launch_bounds__(kBlock, 8) k_trace(DScene sc, DPools p, TraceParams tp, int stack_cap, int *overflow) {
    if (tp.lock_shades != nullptr && tp.lock_round >= 1 && tp.lock_shades[tp.lock_round] == 0u) return;
    extern __shared__ int s_lds[];
    int *stack = s_lds + threadIdx.x;
    int *over = overflow + (blockIdx.x * kBlock + threadIdx.x);
    volatile int *pend = s_lds + (stack_cap + 1) * kBlock + (threadIdx.x & ~63);  // this wave's 64 entries
    const int total = tp.total;
    const int n_chunks = (total + 63) >> 6;  // chunks per ray kind
    const int all_chunks = 2 * n_chunks;     // [closest chunks][any chunks]
    const unsigned lane = lane_id();
    constexpr int kAnyBit = 1 << 30;  // ray id = slot | kAnyBit for shadow rays

    // wave-uniform work bookkeeping.  Candidates come in chunks of 64 consecutive slots, dealt
    // round-robin over the waves of the grid (chunk = wave id + k * waves): no shared head counter
    // -- a same-address atomic costs ~5 ns on this chip and 16k of them per launch formed a convoy.
    // The valid candidates of a chunk (live slots / slots that spawned a shadow ray this round) are
    // compacted into `pend` with ballot + mbcnt and handed to idle lanes from there, so the ray
    // queues of the reference (flag arrays + cub::DeviceSelect, render.cuh:431-443) exist only as
    // 64 ints of LDS per wave.
    int pend_lo = 0, pend_hi = 0;
    int next_chunk = (int)wave_index();
    const int grid_waves = (int)(gridDim.x * (kBlock / 64));
    bool exhausted = false;
    // per-lane ray state.  `tri` is the best hit so far (closest) or the excluded triangle (any);
    // `hu` doubles as the occluded flag of an any-hit ray.
    int id = -1, cur = kEntryDone, sp = 0, tri = -1;
    V3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
    float tmax = 0.f, hu = 0.f, hv = 0.f;
    unsigned long long deposits = 0;
#ifdef RT_TRACE_PROFILE
    unsigned long long pf_outer = 0, pf_refill = 0, pf_inner_it = 0, pf_inner_lanes = 0, pf_leaf_it = 0, pf_leaf_lanes = 0,
                       pf_tri_it = 0, pf_tri_lanes = 0, pf_act_at_top = 0, pf_fin_lanes = 0, pf_new_lanes = 0;
#endif

    while (true) {
        unsigned long long act = wave_ballot(id >= 0 && cur != kEntryDone);
#ifdef RT_TRACE_PROFILE
        pf_outer++;
        pf_act_at_top += __popcll(act);
#endif
        if (__popcll(act) <= kRefillAt) {
            // ---- finalise finished lanes
            const bool fin = id >= 0 && cur == kEntryDone;
#ifdef RT_TRACE_PROFILE
            pf_refill++;
            pf_fin_lanes += wave_count((fin));
#endif
            const bool is_any = (id & kAnyBit) != 0;
            // a path ray started with no limit: that is where its literal re-trace starts again
            if (VERIFY && !LITERAL && fin && !is_any && tri >= 0)
                verify_closest(sc, o, d, [] { return kFltMax; }, tmax, tri, hu, hv, tp.vstat, stack, over, stack_cap);
            deposits += wave_count((fin && is_any && hu == 0.f));
            if (fin) {
                const int slot = id & (kAnyBit - 1);
                if (!is_any) {
                    // hit record in the form mat() consumes (render.cuh:152-153, 311-316)
                    int info = -1;
                    if (tri >= 0) {
                        Tri tr = load_tri(sc.tris, tri);
                        int2 ml = sc.tri_info[(unsigned)tri];
                        V3 hp = tri_point(tr, hu, hv);
                        V3 hn = neg(unit(tr.n));
                        p.hpx(slot) = hp.x;
                        p.hpy(slot) = hp.y;
                        p.hpz(slot) = hp.z;
                        p.hnx(slot) = hn.x;
                        p.hny(slot) = hn.y;
                        p.hnz(slot) = hn.z;
                        info = (ml.x & 0xffff) | ((ml.y + 1) << 16);
                    }
                    p.hit_info(slot) = info;
                } else if (hu == 0.f && !tp.debug_no_deposit) {  // unoccluded: render.cuh:291-293
                    int pixel = p.pixel(slot);
                    deposit(tp.fb, tp.fb_fixed, pixel, p.slr(slot), p.slg(slot), p.slb(slot));
                }
                id = -1;
            }
            // ---- refill idle lanes (up to three chunks per refill: shadow rays are sparse)
            for (int tries = 0; tries < 3; tries++) {
                unsigned long long idle = wave_ballot(id < 0);
                int n_idle = __popcll(idle);
                if (n_idle == 0) break;
                if (pend_lo == pend_hi && !exhausted) {
                    int chunk = next_chunk;
                    next_chunk += grid_waves;
                    if (chunk >= all_chunks) {
                        exhausted = true;
                    } else {
                        const bool any_chunk = chunk >= n_chunks;
                        int cand = (any_chunk ? chunk - n_chunks : chunk) * 64 + (int)lane;
                        bool valid = cand < total;
                        if (valid) valid = any_chunk ? p.stmax(cand) >= 0.f : (p.bounces(cand) != kDone && p.bounces(cand) != kParked);
                        unsigned long long vm = wave_ballot(valid);
                        if (valid) pend[prefix_popc(vm)] = any_chunk ? (cand | kAnyBit) : cand;
                        pend_lo = 0;
                        pend_hi = __popcll(vm);
                    }
                }
                int avail = pend_hi - pend_lo;
                if (avail > 0) {
                    int r = (int)prefix_popc(idle);
                    if (id < 0 && r < avail) {
                        int my = pend[pend_lo + r];
                        int slot = my & (kAnyBit - 1);
                        if (my & kAnyBit) {
                            o = mk(p.sox(slot), p.soy(slot), p.soz(slot));
                            d = mk(p.sdx(slot), p.sdy(slot), p.sdz(slot));
                            tmax = p.stmax(slot);
                            tri = p.starget(slot);
                        } else {
                            o = mk(p.ox(slot), p.oy(slot), p.oz(slot));
                            d = mk(p.dx(slot), p.dy(slot), p.dz(slot));
                            tmax = kFltMax;
                            tri = -1;
                        }
                        id = my;
                        inv = inv_dir(d);
                        cur = 0;  // root pair
                        sp = 0;
                        hu = 0.f;
                    }
                    pend_lo += min(avail, n_idle);
                } else if (exhausted) {
                    break;
                }
            }
            act = wave_ballot(id >= 0 && cur != kEntryDone);
            if (act == 0) {
                if (exhausted && pend_lo == pend_hi) break;  // nothing in flight, nothing pending, no chunks left
                continue;
            }
        }
        if (LITERAL) {
            if (cur >= 0) {
                if ((id & kAnyBit) != 0) reference_walk<true>(sc, o, d, tmax, tri, hu, hv, stack, over, stack_cap);
                else reference_walk<false>(sc, o, d, tmax, tri, hu, hv, stack, over, stack_cap);
                cur = kEntryDone;
            }
            continue;
        }
        // ---- inner phase: step through node records until no lane holds an inner entry
        while (wave_ballot(cur >= 0) != 0) {
#ifdef RT_TRACE_PROFILE
            pf_inner_it++;
            pf_inner_lanes += wave_count((cur >= 0));
#endif
            if (cur >= 0) inner_step<WIDE>(sc, o, inv, tmax, cur, sp, stack, over, stack_cap);
        }
        // ---- leaf phase: every lane that holds a leaf tests its triangles (triangle.cuh:39-58).  The ray kind is a run-time
        // value of the lane here, so the two hit rules of leaf_hits (rt_walk.inc) stand side by side in one loop.
#ifdef RT_TRACE_PROFILE
        {
            unsigned long long lm = wave_ballot(cur != kEntryDone && cur < 0);
            if (lm) {
                pf_leaf_it++;
                pf_leaf_lanes += __popcll(lm);
                int cnt_l = (cur != kEntryDone && cur < 0) ? ((~cur) & 7) : 0;
                int mx = cnt_l, sm = cnt_l;
                for (int off = 32; off > 0; off >>= 1) { mx = max(mx, __shfl_xor(mx, off)); sm += __shfl_xor(sm, off); }
                pf_tri_it += mx;
                pf_tri_lanes += sm;
            }
        }
#endif
        if (cur != kEntryDone && cur < 0) {
            const bool is_any = (id & kAnyBit) != 0;
            int ref = ~cur;
            int first = ref >> 3, count = ref & 7;
            bool stop = false;
            for (int k = first; k < first + count; k++) {
                Tri tr = load_tri(sc.tris, k);
                float t, u, v;
                if (tri_intersect(tr, o, d, tmax, t, u, v)) {
                    if (is_any) {
                        // bvh.cuh:243: first accepted hit that is not the excluded triangle (VERIFY: and that the reference's
                        // walk can see at all)
                        if (k != tri && (!VERIFY || ref_visible(sc, o, d, tr, k, tp.vstat))) {
                            hu = 1.f;    // occluded
                            stop = true;
                            break;
                        }
                    } else {
                        const bool tie = t == tmax && tri >= 0;
                        if (closest_hit_wins(sc, t, tmax, k, tri)) {  // bvh.cuh:227-231 (t <= tmax)
                            tmax = t;
                            hu = u;
                            hv = v;
                            tri = k;
                        }
                        // VERIFY: an exact tie is the reference's tree order to decide (triangle.cuh:49): marked in the
                        // sign of hv (v >= 0 for an accepted hit; a closer hit later overwrites the mark with its own v)
                        if (VERIFY && tie) hv = __uint_as_float(__float_as_uint(hv) | 0x80000000u);
                    }
                }
            }
            if (stop) {
                cur = kEntryDone;
            } else if (sp > 0) {
                cur = stack_pop(stack, over, sp, stack_cap);
            } else {
                cur = kEntryDone;
            }
        }
    }
    if (deposits != 0 && lane == 0) atomicAdd(&tp.rows[wave_index()].c[C_SHADOW_ADD], deposits);
#ifdef RT_TRACE_PROFILE
    if (lane == 0 && tp.prof) {
        atomicAdd(&tp.prof[0], pf_outer); atomicAdd(&tp.prof[1], pf_refill); atomicAdd(&tp.prof[2], pf_inner_it);
        atomicAdd(&tp.prof[3], pf_inner_lanes); atomicAdd(&tp.prof[4], pf_leaf_it); atomicAdd(&tp.prof[5], pf_leaf_lanes);
        atomicAdd(&tp.prof[6], pf_tri_it); atomicAdd(&tp.prof[7], pf_tri_lanes); atomicAdd(&tp.prof[8], pf_act_at_top);
        atomicAdd(&tp.prof[9], pf_fin_lanes); atomicAdd(&tp.prof[10], 1ull);
    }
#endif
}

// ============================================================================ k_query: ray queries on device buffers
// rt_query_closest_device / rt_query_any_device and their host-pointer form, rt_trace_closest / rt_trace_any: the caller's rays,
// from device buffers, through the same shared device functions as k_trace and k_paths (inv_dir, inner_step, tri_intersect,
// closest_hit_wins, ref_visible, reference_walk, the stack helpers) -- the hit decisions are theirs, only the way from a buffer
// to them and back is this kernel's.
enum { Q_CLOSEST = 0, Q_ANY = 1 };
struct QueryWords {           // the scratch of one query call (rt_scene::QueryState::d_words), zeroed before the prepass
    unsigned radius_bits[3];  // per axis: max |origin| over the finite origin components, as the bits of that float
    unsigned bad_dirs;        // rays with a direction component that is not finite or reaches 2^126
    unsigned bad_pixels;      // rt_render_rays_*: rays whose pixel index is outside the sum buffer (k_pixel_prepass)
    unsigned short_dirs;      // rays whose direction is not zero and has no component of 2^-60 or more (rt_bvh.h, kMinDirLength)
    unsigned long long vstat[4];  // V_OWN_FAIL, V_LOST, V_TIE, V_LITERAL of this call (rt_query_last_counters)
    unsigned long long chain_rays;  // k_aov_follow: rays traced beyond the first of each sample (directly behind vstat: one copy)
};
struct QueryParams {
    int n, n_tris;
    const float *o3, *d3, *tmax;         // tmax null: FLT_MAX for every ray
    const int *excluded, *inverse;       // Q_ANY: the caller's index (may be null) and caller order -> leaf order
    int *out_i;                          // hit triangle in the caller's order / occluded flag
    float *out_t, *out_u, *out_v;        // Q_CLOSEST, each may be null
    unsigned long long *vstat;
};

// One pass over the rays before the walk: what ensure_origin_radius needs to know about the origins, and whether every
// direction keeps the precondition of the walk (finite, every component below 2^126 in magnitude: 1 / d and the slab
// products of the reference's box test stay finite; not shorter than rtbvh::kMinDirLength, or the cull's floor under 1 / d would
// walk another ray than the triangle test sees).  A non-negative float orders like its bit pattern, so the maximum is
// an integer atomicMax: one per wave and axis after a wave reduction.
__global__ void __launch_bounds__(kBlock) k_query_prepass(const float *__restrict__ o3, const float *__restrict__ d3, int n,
                                                          QueryWords *__restrict__ words) {
    float mx = 0.f, my = 0.f, mz = 0.f;
    unsigned bad = 0, shrt = 0;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < (size_t)n; i += stride) {
        const float ox = fabsf(o3[3 * i]), oy = fabsf(o3[3 * i + 1]), oz = fabsf(o3[3 * i + 2]);
        if (ox <= kFltMax) mx = fmaxf(mx, ox);  // (false for +inf and NaN)
        if (oy <= kFltMax) my = fmaxf(my, oy);
        if (oz <= kFltMax) mz = fmaxf(mz, oz);
        const float dm = fmaxf(fabsf(d3[3 * i]), fmaxf(fabsf(d3[3 * i + 1]), fabsf(d3[3 * i + 2])));
        const bool nan = d3[3 * i] != d3[3 * i] || d3[3 * i + 1] != d3[3 * i + 1] || d3[3 * i + 2] != d3[3 * i + 2];
        bad += (nan || !(dm < 0x1p126f)) ? 1u : 0u;
        shrt += (dm > 0.f && dm < rtbvh::kMinDirLength) ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, off));
        my = fmaxf(my, __shfl_xor(my, off));
        mz = fmaxf(mz, __shfl_xor(mz, off));
        bad += __shfl_xor(bad, off);
        shrt += __shfl_xor(shrt, off);
    }
    if (lane_id() == 0) {
        if (mx > 0.f) atomicMax(&words->radius_bits[0], __float_as_uint(mx));
        if (my > 0.f) atomicMax(&words->radius_bits[1], __float_as_uint(my));
        if (mz > 0.f) atomicMax(&words->radius_bits[2], __float_as_uint(mz));
        if (bad) atomicAdd(&words->bad_dirs, bad);
        if (shrt) atomicAdd(&words->short_dirs, shrt);
    }
}
// rt_render_rays_*: every pixel index of the table inside the sum buffer?  The same pass for the d_pixel array.
__global__ void __launch_bounds__(kBlock) k_pixel_prepass(const int *__restrict__ pixel, int n, int n_pixels,
                                                          QueryWords *__restrict__ words) {
    unsigned bad = 0;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < (size_t)n; i += stride) bad += (unsigned)pixel[i] >= (unsigned)n_pixels ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off);
    if (lane_id() == 0 && bad) atomicAdd(&words->bad_pixels, bad);
}
// caller order -> leaf order of the scene's triangles, on the device (rt_query_any_device maps the excluded triangle when a
// lane takes its ray, not per candidate in the leaf loop)
__global__ void k_query_inverse(const int *__restrict__ order, int n, int *__restrict__ inverse) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) inverse[order[k]] = k;
}

// ============================================================================ the stream walker of k_query and k_aov
// One persistent launch per call, the grid sized from the device and not from n.  A wave takes chunks of 64 consecutive ray
// ids round-robin (wave id + k x waves of the grid; no shared head counter, for the reason given in k_trace: a same-address
// atomic costs ~5 ns on this chip and thousands of them per launch form a convoy) and hands the rays of its current chunk to
// idle lanes by ballot + mbcnt: every ray of a chunk is wanted, so the pending rays are the id range [pend_lo, pend_hi) in two
// scalars where k_trace compacts slots into LDS.  Once at most kQueryRefillAt lanes still traverse, finished lanes hand their
// result over and take the next rays.  What a kernel adds is its two ends, a struct ENDS with three members:
//   take(id, o, d, tmax, tri)                 a lane takes ray `id`: its origin, direction and limit, and the excluded triangle
//                                             (any hit; leaf order) or -1
//   restart_tmax(id)                          the limit the literal re-trace of ray `id` starts from (verify_closest)
//   finish(fin, id, d, tmax, tri, hu, hv)     called by EVERY lane of the wave in wave-uniform control flow, once per refill pass;
//                                             `fin`: this lane holds a finished ray (closest: tri < 0 = a miss, hv's sign is
//                                             clear; any hit: hu != 0 = occluded).  An end may therefore vote and permute
//                                             across the wave (aov_deposit).
// A refill pass, in this order: the VERIFY finalisation of finished closest-hit lanes, finish, the lane gives up its id, up to
// two refill tries, the termination test.
// An end that declares `static constexpr bool kRearms = true` (k_aov_follow's) has, in place of finish,
//   finish_or_rearm(fin, id, o, d, tmax, tri, hu, hv) -> bool   called like finish; true (only where fin): the lane KEEPS its id
//                                             and walks the ray the end has written into o, d, tmax and tri (-1) from the root.
// The walker does not bound the re-arming: the end must (k_aov_follow: a counter per lane that only grows, below a cap).  For
// every other end the branch does not exist (if constexpr): their kernels are instruction for instruction what they were.
// LDS (dynamic): the stack columns, (stack_cap + 1) x kBlock ints (push_if).
// Registers: no pool, shading or camera state is carried, but the VERIFY finalisation (ref_visible + the literal re-trace)
// and the 4-wide node step with its seven 16-byte loads in flight want 71 VGPRs -- over the 64 of 8 waves per SIMD, where
// the dense-array modes k_trace once had spilled 26.  Measured on C2, 2^22 rays (tools/query_time.py, device time of the whole call): budget 8
// 0.689 / 0.912 / 0.703 ms for camera / bounce / shadow rays, budgets 4 to 7 (one and the same code: 71 VGPRs, 7 waves per SIMD,
// no spill, no scratch) 0.565 / 0.730 / 0.680 ms.  kQueryRefillAt: 24, 32, 48 and 56 all land within 1 % of each other on the
// three batches (the spread of one setting's repetitions is 2 %), so k_trace's 40 stays.
// ANY: the hit rule of the stream (leaf_hits); WIDE / LITERAL / VERIFY: as k_trace's.
#ifndef RT_QUERY_MIN_WAVES
#define RT_QUERY_MIN_WAVES 4
#endif
#ifndef RT_QUERY_REFILL_AT
#define RT_QUERY_REFILL_AT 40
#endif
constexpr int kQueryMinWaves = RT_QUERY_MIN_WAVES;
constexpr int kQueryRefillAt = RT_QUERY_REFILL_AT;
template <class ENDS, class = void>
struct ends_rearm : std::false_type {};
template <class ENDS>
struct ends_rearm<ENDS, std::void_t<decltype(ENDS::kRearms)>> : std::bool_constant<ENDS::kRearms> {};
template <bool ANY, bool WIDE, bool LITERAL, bool VERIFY, class ENDS>
__device__ __forceinline__ void stream_walk(const DScene &sc, ENDS &ends, int n, unsigned long long *vstat, int stack_cap,
                                            int *overflow) {
    extern __shared__ int s_lds[];
    int *stack = s_lds + threadIdx.x;
    const unsigned lane_of_grid = blockIdx.x * kBlock + threadIdx.x;  // (every launch is of kBlock lanes per workgroup)
    int *over = overflow + lane_of_grid;
    const int n_chunks = (int)(((unsigned)n + 63u) >> 6);
    const int grid_waves = (int)(gridDim.x * (kBlock / 64));
    int next_chunk = (int)(lane_of_grid >> 6);
    int pend_lo = 0, pend_hi = 0;  // wave-uniform: ray ids of the current chunk that no lane has taken yet
    // per-lane ray state, as in k_trace: `tri` is the best hit so far (closest) or the excluded triangle (any), leaf order;
    // `hu` doubles as the occluded flag of an any-hit ray
    int id = -1, cur = kEntryDone, sp = 0, tri = -1;
    V3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
    float tmax = 0.f, hu = 0.f, hv = 0.f;

    while (true) {
        unsigned long long act = wave_ballot(id >= 0 && cur != kEntryDone);
        if (__popcll(act) <= kQueryRefillAt) {
            // ---- finalise finished lanes: the reference's decisions first, then the kernel's end
            const bool fin = id >= 0 && cur == kEntryDone;
            if (!ANY && VERIFY && !LITERAL && fin && tri >= 0)
                verify_closest(sc, o, d, [&] { return ends.restart_tmax(id); }, tmax, tri, hu, hv, vstat, stack, over, stack_cap);
            if constexpr (ends_rearm<ENDS>::value) {
                // the lane keeps its id and walks the ray the end has put into (o, d, tmax, tri)
                if (ends.finish_or_rearm(fin, id, o, d, tmax, tri, hu, hv)) {
                    inv = inv_dir(d);
                    cur = 0;  // root
                    sp = 0;
                    hu = hv = 0.f;
                } else if (fin) {
                    id = -1;
                }
            } else {
                ends.finish(fin, id, d, tmax, tri, hu, hv);
                if (fin) id = -1;
            }
            // ---- refill idle lanes (a second chunk when the current one runs out half-way)
            for (int tries = 0; tries < 2; tries++) {
                const unsigned long long idle = wave_ballot(id < 0);
                const int n_idle = __popcll(idle);
                if (n_idle == 0) break;
                if (pend_lo == pend_hi) {
                    if (next_chunk >= n_chunks) break;
                    pend_lo = next_chunk << 6;
                    pend_hi = min(pend_lo + 64, n);
                    next_chunk += grid_waves;
                }
                const int avail = pend_hi - pend_lo, r = (int)prefix_popc(idle);
                if (id < 0 && r < avail) {
                    id = pend_lo + r;
                    ends.take(id, o, d, tmax, tri);
                    inv = inv_dir(d);
                    cur = 0;  // root
                    sp = 0;
                    hu = hv = 0.f;
                }
                pend_lo += min(avail, n_idle);
            }
            act = wave_ballot(id >= 0 && cur != kEntryDone);
            if (act == 0) {
                if (pend_lo == pend_hi && next_chunk >= n_chunks) break;  // nothing in flight, nothing pending, no chunks left
                continue;
            }
        }
        if (LITERAL) {
            if (cur >= 0) {
                reference_walk<ANY>(sc, o, d, tmax, tri, hu, hv, stack, over, stack_cap);
                cur = kEntryDone;
            }
            continue;
        }
        // ---- inner phase: step through node records until no lane holds an inner entry
        while (wave_ballot(cur >= 0) != 0) {
            if (cur >= 0) inner_step<WIDE>(sc, o, inv, tmax, cur, sp, stack, over, stack_cap);
        }
        // ---- leaf phase: every lane that holds a leaf tests its triangles
        if (cur != kEntryDone && cur < 0) {
            const bool stop = leaf_hits<ANY, VERIFY>(sc, o, d, ~cur, tmax, tri, hu, hv, vstat);
            cur = (!stop && sp > 0) ? stack_pop(stack, over, sp, stack_cap) : kEntryDone;
        }
    }
}

// k_query: the rays come from the caller's buffers and the answers go back into them.
// KIND: Q_CLOSEST (the hit triangle in the caller's order, t, u, v; zeros on a miss) or Q_ANY (the occluded flag; the caller's
// excluded triangle goes through `inverse` to leaf order, an index outside 0 .. n_tris - 1 excludes nothing).
// WIDE / LITERAL / VERIFY: as k_trace's.
template <int KIND>
struct QueryEnds {
    const DScene &sc;
    const QueryParams &qp;
    __device__ __forceinline__ float restart_tmax(int id) const { return qp.tmax ? qp.tmax[id] : kFltMax; }
    __device__ __forceinline__ void take(int id, V3 &o, V3 &d, float &tmax, int &tri) const {
        const size_t at = 3 * (size_t)id;
        o = mk(qp.o3[at], qp.o3[at + 1], qp.o3[at + 2]);
        d = mk(qp.d3[at], qp.d3[at + 1], qp.d3[at + 2]);
        tmax = restart_tmax(id);
        tri = -1;
        if (KIND == Q_ANY && qp.excluded) {
            const int e = qp.excluded[id];
            if (e >= 0 && e < qp.n_tris) tri = qp.inverse[e];
        }
    }
    __device__ __forceinline__ void finish(bool fin, int id, V3, float tmax, int tri, float hu, float hv) const {
        if (!fin) return;
        if (KIND == Q_CLOSEST) {
            const bool hit = tri >= 0;
            qp.out_i[id] = hit ? sc.order[(unsigned)tri] : -1;
            if (qp.out_t) qp.out_t[id] = hit ? tmax : 0.f;
            if (qp.out_u) qp.out_u[id] = hit ? hu : 0.f;
            if (qp.out_v) qp.out_v[id] = hit ? hv : 0.f;
        } else {
            qp.out_i[id] = hu != 0.f ? 1 : 0;
        }
    }
};
template <int KIND, bool WIDE, bool LITERAL, bool VERIFY>
__global__ void __launch_bounds__(kBlock, kQueryMinWaves) k_query(DScene sc, QueryParams qp, int stack_cap, int *overflow) {
    QueryEnds<KIND> ends{sc, qp};
    stream_walk<KIND == Q_ANY, WIDE, LITERAL, VERIFY>(sc, ends, qp.n, qp.vstat, stack_cap, overflow);
}

// ============================================================================ k_aov: first-hit feature buffers
// rt_render_aov_fixed / rt_render_aov_rays_fixed_device (DESIGN.md section 2.6): per pixel the albedo, the normal, the emission,
// the depth and the hit count of the FIRST hit of every sample, as int64 fixed-point sums, and optionally the ids of a pixel's
// first sample.  The stream walker (stream_walk: one persistent launch, chunks of 64 consecutive sample ids per wave, idle lanes
// refilled by ballot, the shared walk of rt_walk.inc) with ends of its own: a lane MAKES its ray (SRC = AovCamera: camera ray G of an RT_FLAG_RNG_PER_SAMPLE
// frame, formed as gen_core's per-sample branch forms it) or reads row c of a keyed table (SRC = KeyedRayTable, streamed past
// the caches as gen_core reads it), and a finished lane deposits instead of writing a hit record.
// Nothing of a sample is carried but its id: the pixel (and whether the sample writes ids) is a function of the id and is
// recomputed at the deposit, so the register budget is k_query's.
struct AovCamera {
    Camera cam;
    int width, height;
    unsigned spp;               // samples per pixel of THIS shard (num_samples / shard_count): local sample c -> pixel c / spp
    unsigned key_mul, key_add;  // global sample G = c * shard_count + shard_index (AdvanceParams::key_mul / key_add)
    uint32_t seed_lo, seed_hi;
};
struct AovParams {
    int n;                       // samples of this call
    unsigned long long *sums;    // n_pixels x RT_AOV_CHANNELS int64, ADDED to
    int *ids;                    // n_pixels x 2 {triangle in the caller's order, material}, or null
    unsigned long long *vstat;
};
// -> the sample's stream after the two jitter draws (k_aov_follow goes on with it; k_aov drops it)
__device__ __forceinline__ Rng aov_ray_stream(const AovCamera &s, int id, V3 &o, V3 &d) {
    // gen_core, per-sample streams: pixel = id / spp, the stream of the global id, jitter x then y, camera.get_ray
    const int pixel = (int)((unsigned)id / s.spp);
    const int py = (int)((unsigned)pixel / (unsigned)s.width);
    const int px = pixel - py * s.width;
    Rng rs = rng_sample_stream(s.seed_lo, s.seed_hi, (unsigned long long)id * s.key_mul + s.key_add);
    const float jx = rng_uniform(rs);  // x first, then y (Appendix A.7)
    const float jy = rng_uniform(rs);
    camera_get_ray(s.cam, (px + jx) / s.width, (py + jy) / s.height, o, d);
    return rs;
}
__device__ __forceinline__ void aov_ray(const AovCamera &s, int id, V3 &o, V3 &d) { (void)aov_ray_stream(s, id, o, d); }
__device__ __forceinline__ void aov_ray(const KeyedRayTable &s, int id, V3 &o, V3 &d) {
    const float *o3 = s.o3 + 3 * (size_t)id, *d3 = s.d3 + 3 * (size_t)id;
    o = mk(table_load(o3), table_load(o3 + 1), table_load(o3 + 2));
    d = mk(table_load(d3), table_load(d3 + 1), table_load(d3 + 2));
}
// the pixel of sample `id`, and whether it is the sample that writes its pixel's ids (G % spp == 0: shard 0 only, the host
// passes no id buffer to the others; K % rays_per_pixel == 0, never with a pixel array)
__device__ __forceinline__ int aov_pixel(const AovCamera &s, int id, bool &first) {
    const unsigned pixel = (unsigned)id / s.spp;
    first = (unsigned)id - pixel * s.spp == 0u;
    return (int)pixel;
}
__device__ __forceinline__ int aov_pixel(const KeyedRayTable &s, int id, bool &first) {
    first = false;
    if (s.pixel) return table_load(s.pixel + (unsigned)id);
    const unsigned long long t = s.rem_first + (unsigned long long)(unsigned)id * s.key_stride;  // (as gen_core: K / rpp = pix_first + t / rpp)
    const unsigned long long q = (t >> 32) ? t / s.rays_per_pixel : (unsigned long long)((unsigned)t / s.rays_per_pixel);
    first = t - q * s.rays_per_pixel == 0ull;
    return s.pix_first + (int)q;  // (below n_pixels: the host checks the last key)
}
// The deposit of one finalisation, called by the whole wave (the caller's branch is wave-uniform).  `dep`: this lane holds a
// hit; `pixel` its pixel (-1 otherwise); val[0 .. 9] its fixed-point values.
// RT_AOV_PRE_REDUCE = 0, the first version: one 64-bit atomic per non-zero channel and hitting lane.  Measured on C2 at
// 1920 x 1080 x 16 (tools/aov_time.py): 91 % of the kernel -- the samples of a pixel sit in neighbouring lanes, 16 lanes of an
// atomic instruction on ONE address.
// RT_AOV_PRE_REDUCE = 1 (the product): the lanes of the wave that hold the same pixel are summed first.  The sums are integers,
// so the result is the first version's bit for bit whatever is summed where.  The depositing lanes are packed to the front of
// the wave in lane order (ds_permute: consecutive sample ids, handed out to idle lanes in lane order, become neighbours
// again), runs of equal pixels are added up by a segmented scan over lane distances 1, 2, 4, ... that stops as soon as no run
// is longer (none at one sample per pixel, four steps at sixteen), and the last lane of each run issues the atomics.
#ifndef RT_AOV_PRE_REDUCE
#define RT_AOV_PRE_REDUCE 1
#endif
__device__ __forceinline__ long long aov_pull(int from_lane, long long x) {  // x of lane `from_lane` (ds_bpermute)
    const int lo = __builtin_amdgcn_ds_bpermute(from_lane << 2, (int)(unsigned)(unsigned long long)x);
    const int hi = __builtin_amdgcn_ds_bpermute(from_lane << 2, (int)(unsigned)((unsigned long long)x >> 32));
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ long long aov_push(int to_lane, long long x) {  // this lane's x to lane `to_lane` (ds_permute; a permutation)
    const int lo = __builtin_amdgcn_ds_permute(to_lane << 2, (int)(unsigned)(unsigned long long)x);
    const int hi = __builtin_amdgcn_ds_permute(to_lane << 2, (int)(unsigned)((unsigned long long)x >> 32));
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// `hit`: what a depositing lane adds to the hit count (k_aov_follow: 0 for a chain that left the scene behind a specular vertex).
__device__ __forceinline__ void aov_deposit(const AovParams &ap, bool dep, int pixel, long long (&val)[RT_AOV_HITS], int hit = 1) {
#ifdef RT_AOV_NO_DEPOSIT
    if (ap.n != 0x7fffffff) return;  // measurement build (tools/aov_time.py): always taken, the host refuses such a frame
#endif
    int hits = dep ? hit : 0;
    if (RT_AOV_PRE_REDUCE) {
        const unsigned long long dm = wave_ballot(dep);
        if (dm == 0) return;
        const int lane = (int)lane_id(), n_dep = __popcll(dm);
        // pack: depositing lanes to 0 .. n_dep - 1 in lane order, the others behind them (every lane sends, every lane receives)
        const int to = dep ? (int)prefix_popc(dm) : n_dep + (int)prefix_popc(~dm);
        pixel = __builtin_amdgcn_ds_permute(to << 2, pixel);
        hits = __builtin_amdgcn_ds_permute(to << 2, hits);
#pragma unroll
        for (int c = 0; c < RT_AOV_HITS; c++) val[c] = aov_push(to, val[c]);
        // runs of equal pixels: `stop` is set once a lane's sum reaches back to the head of its run
        const int prev = __builtin_amdgcn_ds_bpermute((lane - 1) << 2, pixel), next = __builtin_amdgcn_ds_bpermute((lane + 1) << 2, pixel);
        int stop = (lane == 0 || pixel < 0 || prev != pixel) ? 1 : 0;
        for (int k = 1; k < 64; k <<= 1) {
            if (wave_ballot(stop == 0) == 0) break;
            const bool take = stop == 0 && lane >= k;
            const int stop_k = __builtin_amdgcn_ds_bpermute((lane - k) << 2, stop), hits_k = __builtin_amdgcn_ds_bpermute((lane - k) << 2, hits);
#pragma unroll
            for (int c = 0; c < RT_AOV_HITS; c++) {
                const long long v_k = aov_pull(lane - k, val[c]);
                if (take) val[c] += v_k;
            }
            if (take) {
                hits += hits_k;
                stop = stop_k;
            }
        }
        dep = pixel >= 0 && (lane == 63 || next != pixel);  // the last lane of a run holds the run's sums
    }
    if (dep) {
        unsigned long long *p = ap.sums + (size_t)(unsigned)pixel * RT_AOV_CHANNELS;
#pragma unroll
        for (int c = 0; c < RT_AOV_HITS; c++)
            if (val[c] != 0) atomicAdd(p + c, (unsigned long long)val[c]);
        atomicAdd(p + RT_AOV_HITS, (unsigned long long)hits);
    }
}
template <class SRC>
struct AovEnds {
    const DScene &sc;
    const SRC &src;
    const AovParams &ap;
    __device__ __forceinline__ float restart_tmax(int) const { return kFltMax; }
    __device__ __forceinline__ void take(int id, V3 &o, V3 &d, float &tmax, int &tri) const {
        aov_ray(src, id, o, d);
        tmax = kFltMax;
        tri = -1;
    }
    // the deposit: what mat() would shade with (tri_shade, the material) and what init() deposits at bounce 0
    __device__ __forceinline__ void finish(bool fin, int id, V3 d, float tmax, int tri, float, float) const {
        bool first = false;
        int pixel = -1, mat = -1;
        long long val[RT_AOV_HITS];  // the ten fixed-point values of this lane's sample (zero: nothing to add)
#pragma unroll
        for (int c = 0; c < RT_AOV_HITS; c++) val[c] = 0;
        if (fin) pixel = aov_pixel(src, id, first);
        const bool dep = fin && tri >= 0;
        if (dep) {
            const float4 sh = sc.tri_shade[(unsigned)tri];
            const int info = __float_as_int(sh.w);
            mat = info & 0xffff;
            const int light = ((info >> 16) & 0xffff) - 1;
            V3 nn = mk(sh.x, sh.y, sh.z);
            if (dot(nn, d) > 0.f) nn = neg(nn);  // faced to the viewer (mat_sample_f's flip)
            const Material m = tab_material(sc.tables, mat);
            val[RT_AOV_ALBEDO + 0] = to_fixed(m.ax);
            val[RT_AOV_ALBEDO + 1] = to_fixed(m.ay);
            val[RT_AOV_ALBEDO + 2] = to_fixed(m.az);
            val[RT_AOV_NORMAL + 0] = to_fixed(nn.x);
            val[RT_AOV_NORMAL + 1] = to_fixed(nn.y);
            val[RT_AOV_NORMAL + 2] = to_fixed(nn.z);
            if (light >= 0) {  // render.cuh:98-103
                const Light l = tab_light(sc.tables, sc.num_mats, light);
                val[RT_AOV_EMISSION + 0] = to_fixed(l.lx);
                val[RT_AOV_EMISSION + 1] = to_fixed(l.ly);
                val[RT_AOV_EMISSION + 2] = to_fixed(l.lz);
            }
            val[RT_AOV_DEPTH] = to_fixed(tmax);
        }
        if (fin && ap.ids && first) {
            ap.ids[2 * (size_t)(unsigned)pixel] = tri >= 0 ? sc.order[(unsigned)tri] : -1;
            ap.ids[2 * (size_t)(unsigned)pixel + 1] = mat;
        }
        aov_deposit(ap, dep, dep ? pixel : -1, val);
    }
};
template <class SRC, bool WIDE, bool LITERAL, bool VERIFY>
__global__ void __launch_bounds__(kBlock, kQueryMinWaves) k_aov(DScene sc, SRC src, AovParams ap, int stack_cap, int *overflow) {
    AovEnds<SRC> ends{sc, src, ap};
    stream_walk<false, WIDE, LITERAL, VERIFY>(sc, ends, ap.n, ap.vstat, stack_cap, overflow);
}

// ============================================================================ k_aov_follow: features of the first diffuse vertex
// rt_render_aov_follow_fixed / rt_render_aov_follow_rays_fixed_device (DESIGN.md section 2.11): k_aov's buffers, but a sample
// whose hit is a mirror or glass goes on as sample G of the RT_FLAG_RNG_PER_SAMPLE beauty frame goes on -- mat()'s step there,
// draw for draw -- for up to max_specular vertices, and deposits the features of the vertex its chain ends on.  The fourth pair
// of ends on the stream walker, and the one that re-arms: a finished lane whose hit is specular with j < max_specular keeps its
// id and takes the next ray of its chain in place.  j grows by one with every re-arm and the host refuses a cap above
// RT_AOV_FOLLOW_MAX, so a lane re-arms at most five times.
// Carried per lane (12 registers more than k_aov): the stream (6 words), beta, the path length, and one word that holds j and
// the first hit's light.  (Re-deriving the stream from the key and a draw count would carry 1 word for 6 and pay a
// rng_sample_stream and up to 17 steps per vertex; not built.)
struct AovFollowParams {
    uint32_t seed_lo, seed_hi;       // the table form's streams (the camera form's seed travels in AovCamera)
    int max_specular;                // 1 .. RT_AOV_FOLLOW_MAX (0 is served by k_aov)
    unsigned long long *chain_rays;  // QueryWords::chain_rays: the rays traced beyond the first of each sample
};
__device__ __forceinline__ Rng aov_ray_stream(const KeyedRayTable &s, const AovFollowParams &fp, int id, V3 &o, V3 &d) {
    aov_ray(s, id, o, d);
    Rng rs = rng_sample_stream(fp.seed_lo, fp.seed_hi, s.key_first + (unsigned long long)(unsigned)id * s.key_stride);
    rng_next(rs);  // the two jitter draws, made and thrown away (gen_core's keyed branch)
    rng_next(rs);
    return rs;
}
__device__ __forceinline__ Rng aov_ray_stream(const AovCamera &s, const AovFollowParams &, int id, V3 &o, V3 &d) {
    return aov_ray_stream(s, id, o, d);
}
template <class SRC>
struct AovFollowEnds {
    static constexpr bool kRearms = true;
    const DScene &sc;
    const SRC &src;
    const AovParams &ap;
    const AovFollowParams &fp;
    // per lane, from take() to the deposit
    Rng rs;
    V3 beta;
    float path;  // ((t_0 + t_1) + ...) + t_j
    int jl;      // j | (light of the first hit + 1) << 8
    // per wave
    unsigned long long rearmed = 0;
    __device__ __forceinline__ float restart_tmax(int) const { return kFltMax; }
    __device__ __forceinline__ void take(int id, V3 &o, V3 &d, float &tmax, int &tri) {
        rs = aov_ray_stream(src, fp, id, o, d);
        beta = mk(1.f, 1.f, 1.f);
        path = 0.f;
        jl = 0;
        tmax = kFltMax;
        tri = -1;
    }
    __device__ __forceinline__ bool finish_or_rearm(bool fin, int id, V3 &o, V3 &d, float &tmax, int &tri, float hu, float hv) {
        bool first = false, again = false;
        int pixel = -1, mat = -1, hit = 0;
        long long val[RT_AOV_HITS];
#pragma unroll
        for (int c = 0; c < RT_AOV_HITS; c++) val[c] = 0;
        if (fin) pixel = aov_pixel(src, id, first);
        const int j = jl & 0xff, hit_tri = tri;
        if (fin && tri >= 0) {
            const float4 sh = sc.tri_shade[(unsigned)tri];
            const int info = __float_as_int(sh.w);
            mat = info & 0xffff;
            if (j == 0) jl = ((info >> 16) & 0xffff) << 8;  // the light of the first hit (+ 1)
            V3 n = mk(sh.x, sh.y, sh.z);
            const Material m = tab_material(sc.tables, mat);
            path = path + tmax;  // (0.f + t_0 is t_0)
            if (m.type != 0 && j < fp.max_specular) {
                // ---- mat() :139-248 at this vertex: the new ray, beta, and the stream behind everything mat() draws there
                const Tri tr = load_tri(sc.tris, tri);
                V3 wi;
                float pdf;
                int again_draws;
                const V3 f = mat_sample_f(m, d, rs, n, wi, pdf, again_draws);
                o = offset_ray_origin(tri_point(tr, hu, hv), n);
                beta = mul(beta, divf(scale(f, dot(wi, n)), pdf));  // :166
                d = wi;
                if (sc.num_lights > 0) {
                    const int light_idx = min((int)(rng_uniform(rs) * sc.num_lights), sc.num_lights - 1);  // :178
                    if (tab_light(sc.tables, sc.num_mats, light_idx).type != 0) {
                        rng_next(rs);  // Triangle::sample_p
                        rng_next(rs);
                        if (again_draws >= 1) rng_next(rs);  // the second sample_f call
                        if (again_draws >= 2) rng_next(rs);
                    }
                }
                tmax = kFltMax;
                tri = -1;
                jl += 1;
                again = true;
            } else {
                if (dot(n, d) > 0.f) n = neg(n);  // faced against the arriving direction
                val[RT_AOV_ALBEDO + 0] = to_fixed(beta.x * m.ax);
                val[RT_AOV_ALBEDO + 1] = to_fixed(beta.y * m.ay);
                val[RT_AOV_ALBEDO + 2] = to_fixed(beta.z * m.az);
                val[RT_AOV_NORMAL + 0] = to_fixed(n.x);
                val[RT_AOV_NORMAL + 1] = to_fixed(n.y);
                val[RT_AOV_NORMAL + 2] = to_fixed(n.z);
                val[RT_AOV_DEPTH] = to_fixed(path);
                hit = 1;
            }
        }
        if (fin && j == 0 && ap.ids && first) {  // the ids stay the first hit's
            ap.ids[2 * (size_t)(unsigned)pixel] = hit_tri >= 0 ? sc.order[(unsigned)hit_tri] : -1;
            ap.ids[2 * (size_t)(unsigned)pixel + 1] = mat;
        }
        const int light = (jl >> 8) - 1;
        const bool ends_here = fin && !again;
        if (ends_here && light >= 0) {  // render.cuh:98-103: the first hit's, wherever the chain ends
            const Light l = tab_light(sc.tables, sc.num_mats, light);
            val[RT_AOV_EMISSION + 0] = to_fixed(l.lx);
            val[RT_AOV_EMISSION + 1] = to_fixed(l.ly);
            val[RT_AOV_EMISSION + 2] = to_fixed(l.lz);
        }
        // a chain that left the scene behind a specular vertex: its emission, no hit
        const bool dep = ends_here && (hit != 0 || light >= 0);
        aov_deposit(ap, dep, dep ? pixel : -1, val, hit);
        rearmed += wave_count((again));
        return again;
    }
};
// Registers (profiles/aov_follow_resources.md): under k_aov's budget of 4 waves per SIMD (128 VGPRs, which k_aov's deposit
// fills to 113 - 124) the twelve words more spill 1 to 4 VGPRs in every build but the literal ones; at 3 waves nothing spills.
constexpr int kAovFollowMinWaves = 3;
template <class SRC, bool WIDE, bool LITERAL, bool VERIFY>
__global__ void __launch_bounds__(kBlock, kAovFollowMinWaves) k_aov_follow(DScene sc, SRC src, AovParams ap, AovFollowParams fp, int stack_cap,
                                                                      int *overflow) {
    AovFollowEnds<SRC> ends{sc, src, ap, fp};
    stream_walk<false, WIDE, LITERAL, VERIFY>(sc, ends, ap.n, ap.vstat, stack_cap, overflow);
    if (lane_id() == 0 && ends.rearmed != 0) atomicAdd(fp.chain_rays, ends.rearmed);
}

// ============================================================================ k_motion: where a pixel's first hit was one frame ago
// rt_render_motion (DESIGN.md section 2.9): the third pair of ends on the stream walker.  Ray `id` is the ray through the centre
// of pixel `id` (the AOV ray with both jitters 0.5f, no stream drawn); a finished lane maps its hit to the caller's order, forms
// the point (u, v) of that triangle on the PREVIOUS vertices -- row k of the caller's array, or the scene's own record when the
// vertices did not move --, projects it into the previous camera (tm_project, rt_temporal.h: shared with the CPU twin and stated
// in the header) and writes {sx, sy, dist, bits of k} as one 16-byte store; a miss writes {0, 0, 0, bits of -1}.
// Nothing is carried per lane but the id.  Registers (profiles/motion_resources.md): no spill and no scratch, 74 - 77 VGPRs in the
// 4-wide builds against k_query's 71 - 72 -- one step past the seven-wave budget, so six waves per SIMD where k_query has seven.
struct MotionParams {
    Camera cam;
    TmCamera prev;             // the previous camera, prepared on the host (tm_camera)
    int n, width, height;
    const float *prev_tris;    // n_tris x 9 in the caller's order, or null: the scene's records
    float4 *out;               // n records
    unsigned long long *vstat;
};
struct MotionEnds {
    const DScene &sc;
    const MotionParams &mp;
    __device__ __forceinline__ float restart_tmax(int) const { return kFltMax; }
    __device__ __forceinline__ void take(int id, V3 &o, V3 &d, float &tmax, int &tri) const {
        const int py = (int)((unsigned)id / (unsigned)mp.width);
        const int px = id - py * mp.width;
        camera_get_ray(mp.cam, (px + 0.5f) / mp.width, (py + 0.5f) / mp.height, o, d);
        tmax = kFltMax;
        tri = -1;
    }
    __device__ __forceinline__ void finish(bool fin, int id, V3, float, int tri, float hu, float hv) const {
        if (!fin) return;
        float4 rec = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
        if (tri >= 0) {
            const int k = sc.order[(unsigned)tri];
            float P[3], r3[3];
            if (mp.prev_tris) {
                const float *q = mp.prev_tris + 9 * (size_t)(unsigned)k;
                const float q9[9] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]};
                tm_point_of_vertices(q9, hu, hv, P);
            } else {
                const Tri tr = load_tri(sc.tris, tri);
                const float q0[3] = {tr.p0.x, tr.p0.y, tr.p0.z}, e1[3] = {tr.e1.x, tr.e1.y, tr.e1.z}, e2[3] = {tr.e2.x, tr.e2.y, tr.e2.z};
                tm_point(q0, e1, e2, hu, hv, P);
            }
            tm_project(&mp.prev, P, r3);
            rec = make_float4(r3[0], r3[1], r3[2], __int_as_float(k));
        }
        mp.out[(unsigned)id] = rec;
    }
};
template <bool WIDE, bool LITERAL, bool VERIFY>
__global__ void __launch_bounds__(kBlock, kQueryMinWaves) k_motion(DScene sc, MotionParams mp, int stack_cap, int *overflow) {
    MotionEnds ends{sc, mp};
    stream_walk<false, WIDE, LITERAL, VERIFY>(sc, ends, mp.n, mp.vstat, stack_cap, overflow);
}

// rt_aov_resolve: sums -> floats, one thread per value.  s = float(double(sum) * 2^-30) as k_post_process_fixed forms it;
// albedo, normal, emission: s / spp (the mean normal is not renormalised); depth: the mean over the HITS; channel 10: coverage.
__global__ void k_aov_resolve(const long long *__restrict__ sums, float *__restrict__ out, long long n_values, float inv_spp) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_values) return;
    const long long p = i / RT_AOV_CHANNELS;
    const int ch = (int)(i - p * RT_AOV_CHANNELS);
    const long long hits = sums[p * RT_AOV_CHANNELS + RT_AOV_HITS];
    const float s = (float)((double)sums[i] * (1.0 / 1073741824.0));
    float r;
    if (ch == RT_AOV_HITS) r = (float)hits * inv_spp;
    else if (ch == RT_AOV_DEPTH) r = hits > 0 ? s / (float)hits : 0.f;
    else r = s * inv_spp;
    out[i] = r;
}
