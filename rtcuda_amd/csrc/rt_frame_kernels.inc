// The kernels of a frame: k_advance (one round of init() + mat() + gen() for all slots, state in the pools) and k_paths (the
// persistent kernel).  Two templates, included by rtcuda_amd.hip once:
//   k_advance<SRC, LDS_TABLES>   SRC: the source of camera rays -- Camera (gen()'s pinhole) or RayTable (the caller's rays,
//                                rt_render_rays_*): see gen_core
//   k_paths<BUILD, ...>          BUILD: one of the tags defined in front of the include (PathsCamera, PathsRays, PathsKeyed,
//                                PathsChunked, PathsBg, PathsChunkedBg, PathsCounts), which carries
//     BUILD::Src                 the source type: Camera, RayTable, KeyedRayTable (a per-sample stream per row) or CountsCamera
//     BUILD::kChunks             the chunked deal (rt_slot_chunks.h) is compiled in; only 4-waves-per-SIMD reference-mode instances
//                                of such a build are ever launched
//     BUILD::kBg                 gen() passes over background pixels (gen_background)
//     BUILD::kCounts             (with kBg) a counted frame (rt_render_counts_fixed): a drawn id's pixel and sample come from the
//                                count map's prefix sum
// What a build does not have is discarded by `if constexpr` when it is instantiated: it carries no instruction of it.
//   RT_CHUNK_RELEASE_WAIT      (experiment define) 0: the chunked deal's release leaves the wait for the state's stores to the
//                              compiler's memory model, which has none at workgroup scope
#ifndef RT_CHUNK_RELEASE_WAIT
#define RT_CHUNK_RELEASE_WAIT 1
#endif

// k_advance: one slot per thread, state in the pools.
// Every per-slot input is indexed by the slot id, so all of a lane's loads are issued together
// (one memory round trip); the small shared tables are staged in LDS with one more independent
// round trip; the hit record written by k_trace<MODE_POOL> already carries the shading point,
// the flipped unit normal and the material / light ids, so no triangle is gathered here.  The
// kernel has no atomics on shared words and one barrier (the table staging): the shadow ray goes
// to the slot's own record, event counts go to the wave's own counter row.
// Thread t serves slot t of its block, whatever the material (the reference shades in compacted-queue order too:
// render.cuh:139-145).  Sorting the block's slots by material, so that a wave runs one branch of Material::sample_f, was
// measured on C2's whole frame through the round pipeline (RT_PERSISTENT=0): k_advance took 87 ms sorted against 70 ms in
// slot order (profiles/r04_experiments.md) -- the kernel streams 36 arrays of slot state and is bound by that traffic; the
// sort costs a dependent load phase and two barriers in front of it, while the divergence it removes was not what the
// kernel waited for.
template <class SRC, bool LDS_TABLES>
__global__ void __launch_bounds__(kBlock)
k_advance(DScene sc, DPools p, SRC cam, AdvanceParams ap, float *__restrict__ fb, DCounters *__restrict__ ctr,
             DWaveRow *__restrict__ rows, unsigned int *__restrict__ lock_shades) {
    // Lockstep rounds (final generation): the reference's host loop ends at the first iteration in which nothing shades
    // (render.cuh:436).  The rounds are all enqueued at once; lock_shades[j] counts the mat() events of round j, and a round
    // finds out on the device whether the render ended before it: round j >= 2 does nothing if round j - 1 shaded nothing
    // (round 0 only generates; once a round is skipped it counts nothing, so every later one is skipped too).  No host poll.
    if (ap.lockstep >= 3 && lock_shades[ap.lockstep - 2] == 0u) return;
    __shared__ float s_tab[LDS_TABLES ? kTabDwordsMax : 1];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in_range = i < ap.n;
    // ---- issue all per-slot loads up front
    SlotState st;
    st.bounces = kDone;
    st.hit_info = -1;
    st.pixel = 0;
    st.gen = 0;
    st.rs = Rng{0, 0, 0, 0, 0, 0};
    st.beta = st.wo = st.isect_p = st.isect_n = mk(0, 0, 0);
    if (in_range) {
        st.bounces = p.bounces(i);
        st.hit_info = p.hit_info(i);
        st.pixel = p.pixel(i);
        st.gen = p.gen(i);
        st.rs = Rng{p.rd(i), p.r0(i), p.r1(i), p.r2(i), p.r3(i), p.r4(i)};
        st.beta = mk(p.br(i), p.bg(i), p.bb(i));
        st.wo = mk(p.dx(i), p.dy(i), p.dz(i));
        st.isect_p = mk(p.hpx(i), p.hpy(i), p.hpz(i));
        st.isect_n = mk(p.hnx(i), p.hny(i), p.hnz(i));
    }
    const float *tab = sc.tables;
    if (LDS_TABLES) {
        for (int k = threadIdx.x; k < sc.tab_dwords; k += kBlock) s_tab[k] = sc.tables[k];
        __syncthreads();
        tab = s_tab;
    }
    // Final generation: the reference stops the whole render at the first iteration in which no slot
    // shades (render.cuh:436), which can cut off slots that Russian roulette would have revived
    // later.  That is a global condition, so the last generation runs in lockstep: slots that finish
    // generation last_gen - 1 park, and once all are parked the rounds run one init() per slot each (all enqueued at once:
    // see the top of this kernel for how a round knows that the render ended before it).
    if (ap.lockstep && st.bounces == kParked) {
        st.bounces = ap.max_bounces;  // routes the slot to gen() below
        st.hit_info = -1;
    }
    const bool alive = st.bounces != kDone && st.bounces != kParked;
    AdvanceOut out;
    out.did_gen = out.did_shade = out.has_shadow = out.did_emit = out.new_ray = false;
    out.rr_draws = 0;
    if (alive) {
        const int gen_before = st.gen;
        advance_core<false>(sc, tab, cam, ap, ap.slot_lo + i, st, out, fb);
        if (out.new_ray) {
            p.ox(i) = out.ray_o.x;
            p.oy(i) = out.ray_o.y;
            p.oz(i) = out.ray_o.z;
            p.dx(i) = out.ray_d.x;
            p.dy(i) = out.ray_d.y;
            p.dz(i) = out.ray_d.z;
        }
        if (st.gen != gen_before) {
            p.gen(i) = st.gen;
            p.pixel(i) = st.pixel;
        }
        if (out.has_shadow) {
            p.sox(i) = out.s_o.x;
            p.soy(i) = out.s_o.y;
            p.soz(i) = out.s_o.z;
            p.sdx(i) = out.s_d.x;
            p.sdy(i) = out.s_d.y;
            p.sdz(i) = out.s_d.z;
            p.slr(i) = out.s_L.x;
            p.slg(i) = out.s_L.y;
            p.slb(i) = out.s_L.z;
            p.starget(i) = out.s_target;
            p.stmax(i) = out.s_tmax;
        }
        p.br(i) = st.beta.x;
        p.bg(i) = st.beta.y;
        p.bb(i) = st.beta.z;
        p.bounces(i) = st.bounces;
        p.rd(i) = st.rs.d;
        p.r0(i) = st.rs.v0;
        p.r1(i) = st.rs.v1;
        p.r2(i) = st.rs.v2;
        p.r3(i) = st.rs.v3;
        p.r4(i) = st.rs.v4;
    }
    if (in_range && !out.has_shadow) p.stmax(i) = -1.f;  // no shadow ray from this slot this round

    // ---- event counters: this wave's own row
    unsigned long long traced = wave_ballot(out.did_gen || out.did_shade);
    int rr_tot = out.rr_draws;
    if (wave_ballot(out.rr_draws != 0)) {
        for (int off = 32; off > 0; off >>= 1) rr_tot += __shfl_xor(rr_tot, off);
    } else {
        rr_tot = 0;
    }
    unsigned long long v[C_COUNT] = {(unsigned long long)wave_count((out.did_gen)),
                                     (unsigned long long)wave_count((out.did_shade)),
                                     (unsigned long long)__popcll(traced),
                                     (unsigned long long)wave_count((out.has_shadow)),
                                     (unsigned long long)wave_count((out.did_emit)),
                                     0ull,
                                     (unsigned long long)rr_tot,
                                     0ull};
    row_add(rows, v);
    // liveness is monotone (a finished slot never restarts), so the host only needs it for the
    // round that closes a batch: one plain store per live wave in 1 round out of 8
    if ((ap.round & ap.batch_mask) == ap.batch_mask && traced != 0 && lane_id() == 0) ctr->last_live_round = ap.round;
    if (ap.lockstep) {
        unsigned long long sm = wave_ballot(out.did_shade);
        if (sm != 0 && lane_id() == 0) atomicAdd(&lock_shades[ap.lockstep - 1], (unsigned)__popcll(sm));
    }
}

template <class BUILD, bool LDS_TABLES, bool WIDE, int MIN_WAVES, bool DRAW_CIDS = false, bool LITERAL = false, bool VERIFY = false>
__global__ void __launch_bounds__(kBlock, MIN_WAVES)
k_paths(DScene sc, DPools p, typename BUILD::Src cam_arg, AdvanceParams ap_arg, float *__restrict__ fb, DWaveRow *__restrict__ rows,
        int stack_cap, int *overflow, int adv_batch, int debug_no_deposit, unsigned long long *prof, int top_n,
        int prio_period, int rot_wave, int rot_set, int gen_batch, int tri_follow, unsigned int *__restrict__ next_cid,
        unsigned long long *__restrict__ vstat) {
    using SRC = typename BUILD::Src;
    // The GEN block exists where the chip is short of issue slots (4 waves per SIMD): there it takes a third of the
    // lanes out of the long ADV block (+3 %, and the ADV block no longer spills).  On small shards (2 waves per
    // SIMD) a slot-round is a latency chain and one more block in it costs 5 %: gen() stays inside ADV there.
    constexpr bool SPLIT_GEN = MIN_WAVES != 2;
    // Code placement: where the hot blocks fall within 64-byte instruction-cache lines is worth 0.7 % of the frame.  With
    // the body 8 bytes earlier than these two s_nop put it, C2's k_paths took 108.7 ms against 107.9 ms (same instructions
    // otherwise).  Time the frame (tools/ab_bench.py) after any edit that moves the code of this kernel.
    asm volatile("s_nop 0\n\ts_nop 0");
    extern __shared__ int s_lds[];
    int *stack = s_lds + threadIdx.x;
    float *park = (float *)(s_lds + (stack_cap + 1) * kBlock) + threadIdx.x;  // element k at park[k * kBlock]
    int *over = overflow + (blockIdx.x * kBlock + threadIdx.x) % kOverStride;
    int *cold = s_lds + (stack_cap + 10) * kBlock + threadIdx.x;  // element k at cold[k * kBlock]
    float *acc = (float *)(s_lds + (stack_cap + 23) * kBlock) + threadIdx.x;  // sample accumulator (acc_add / acc_flush)
    float *s_tab = (float *)(s_lds + (stack_cap + 26) * kBlock);
    const float *tab = sc.tables;
    // small shards (MIN_WAVES == 2: at most 2 workgroups per CU, LDS to spare, latency-bound): the top of
    // the BVH is staged in LDS, so the first levels of every traversal do not leave the CU
    const float4 *s_top = (const float4 *)(s_tab + (LDS_TABLES ? ((sc.tab_dwords + 3) & ~3) : 0));  // (tables: what the scene needs)
    // The chunked deal (rt_slot_chunks.h) of the 4-waves-per-SIMD reference-mode builds: G > 0 camera rays per task, 0 = the
    // static deal.  These builds keep no records of the tree in LDS, so G travels in `top_n`, and above G's bits the static
    // head: the slot sets a lane runs as in the static deal before it draws its first task.
    constexpr bool CHUNKS = BUILD::kChunks && SPLIT_GEN && !DRAW_CIDS;
    // [0]: the workgroup's next task; [1]: G; [2 .. 4]: rtchunks::multiple_of(G); [5]: the static head; [6] (the skipping build):
    // rtchunks::next_multiple_mul(G).  The GEN block reads G, the words and the head from here: as scalars kept across the main
    // loop they pushed other scalars out into VGPR lanes (53 more v_readlane in the default build, and the static deal 2.5 %
    // slower than without this code).
    __shared__ __attribute__((aligned(16))) unsigned s_task[CHUNKS ? 8 : 1];
    // the semaphores of the workgroup's dealt entries, two 16-bit fields to a word (rt_slot_chunks.h): all banked
    __shared__ unsigned s_sem[CHUNKS ? rtchunks::kSemWords : 1];
    const unsigned chunk_g0 = (CHUNKS && top_n > 0) ? (unsigned)top_n & ((1u << rtplan::kChunkHeadShift) - 1u) : 0u;
    const unsigned chunk_head0 = (CHUNKS && top_n > 0) ? (unsigned)top_n >> rtplan::kChunkHeadShift : 0u;  // (both only used before the main loop)
    if (CHUNKS) {
        for (unsigned k = threadIdx.x; k < rtchunks::kSemWords; k += kBlock) s_sem[k] = rtchunks::kSemWordInit;
        if (threadIdx.x == 0) {
            const rtchunks::Multiple m = rtchunks::multiple_of(chunk_g0 ? chunk_g0 : 1u);
            s_task[0] = 0u;
            s_task[1] = chunk_g0;
            s_task[2] = m.inv;
            s_task[3] = m.shift;
            s_task[4] = m.limit;
            s_task[5] = chunk_head0;
            if constexpr (BUILD::kBg) s_task[6] = rtchunks::next_multiple_mul(chunk_g0 ? chunk_g0 : 1u);  // [6]: for the limit of a run over background pixels
        }
    }
    const bool chunk_start = CHUNKS && chunk_g0 && chunk_head0 == 0u;  // no static head: the lane starts without a slot
    if (MIN_WAVES != 2) top_n = 0;
    for (int k = threadIdx.x; k < top_n * 4; k += kBlock) ((float4 *)s_top)[k] = sc.nodes[k];
    if (LDS_TABLES) {
        for (int k = threadIdx.x; k < sc.tab_dwords; k += kBlock) s_tab[k] = sc.tables[k];
        tab = s_tab;
    }
    // The camera and the frame parameters are only needed inside the GEN / ADV blocks: kept as kernel arguments
    // they occupy ~30 SGPRs for the whole loop and push other scalars out into VGPR lanes (v_readlane /
    // v_writelane are VALU work).  Staged in LDS they are read where they are used.
    struct Uniforms {
        SRC cam;
        AdvanceParams ap;
    };
    static_assert(sizeof(Uniforms) % 4 == 0, "dword copy");
    Uniforms *s_uni = (Uniforms *)(s_top + 4 * (size_t)top_n);
    {
        Uniforms u;
        u.cam = cam_arg;
        u.ap = ap_arg;
        const int *srcw = (const int *)&u;
        for (int k = threadIdx.x; k < (int)(sizeof(Uniforms) / 4); k += kBlock) ((int *)s_uni)[k] = srcw[k];
    }
    __syncthreads();
    const SRC &cam = s_uni->cam;
    const AdvanceParams &ap = s_uni->ap;
    // what the scheduling loop itself needs stays scalar
    const int ap_n = ap_arg.n, ap_max_bounces = ap_arg.max_bounces, ap_fb_fixed = ap_arg.fb_fixed;
    // RT_FLAG_RNG_PER_SAMPLE: camera rays are not tied to slots, so the wave DRAWS them -- kCidChunk ids at a time from the
    // frame's counter (one global atomic per chunk), handed to its lanes as they ask for one -- and no lane is left with more
    // work than the others at the end of the frame (the static deal of slots costs 6 % there, 23 % on a 1/8 frame)
    // (a build of its own -- DRAW_CIDS -- so that the reference-mode kernel carries none of it)
    constexpr bool draw_cids = DRAW_CIDS && SPLIT_GEN;
    int cid_next = 0, cid_end = 0;
    // A counted frame (BUILD::kCounts): the pixels of the first and of the last id of the wave's chunk, found once when the chunk is drawn, by
    // all lanes together.  A lane looks for its id's pixel between them: at most kCidChunk pixels with samples, plus whatever
    // runs of pixels without samples lie among them (counts_find takes the last pixel of such a run).
    // cid_win: lane j's copy of the offset of pixel cid_plo + j, read once per chunk -- the window in which a lane finds its id's
    // pixel by shuffles instead of loads; only the ids whose pixel lies beyond the window's 64 pixels (fewer than 8 samples to
    // a pixel, or a run without samples inside the chunk) go on to search memory, between the window's last pixel and cid_phi.
    int cid_plo = 0, cid_phi = 0;
    unsigned cid_win = 0u;
    // A lane works through the slots i, i + G, i + 2G, ... (G = lanes of the grid), each for the whole
    // frame, one after the other: with G dividing the slot count every lane gets the same number of
    // slots, so all lanes -- and all workgroups, which are all resident -- finish together.
    const int lanes_in_grid = (int)(gridDim.x * blockDim.x);
    // Which slots.  Slot s works through the pixels (s + g W) / spp, g = 0, 1, ...: a lattice of a few image
    // columns (every 128th at 1920 x 1080 x 256 spp), the same lattice for slots s and s + 64 * lattice_blocks.
    // A wave always owns 64 CONSECUTIVE slots (samples of one pixel: coherent primary rays; splitting waves
    // into quarters was measured and loses more than it balances), but with plain striding the four waves of a
    // workgroup, the four workgroups of a CU and all successive slot sets of a lane fall on ONE lattice, and
    // whole CUs differ by +-5 % in work (bunny or no bunny in their columns) -- which the slowest one turns
    // into frame time.  So the j-th wave of a workgroup is shifted by j quarter periods and the k-th slot set
    // by k * 5/16 of a period.  A bijection between (set, 64-slot block) and (set, wave).  +6 % at 1 GPU.
    // (rtchunks::slot_of, for any lane of the workgroup: the chunked deal hands a lane the slots of the others)
    auto slot_of = [&](int set, unsigned lane_in_wg) {  // (everything recomputed here: nothing of this lives across the main loop)
        // (the grid is a power of two: W is, shard counts divide it, and the host halves from there)
        return rtchunks::slot_of((unsigned)set, blockIdx.x * blockDim.x + lane_in_wg, (unsigned)lanes_in_grid, (unsigned)rot_wave, (unsigned)rot_set);
    };
    int slot_set = 0;
    int i = slot_of(0, threadIdx.x);
    // persistent slot state
    int bounces = kDone, pixel = 0, gen = 0;
    Rng rs{0, 0, 0, 0, 0, 0};
    V3 beta = mk(0, 0, 0);
    auto load_slot = [&](int k) {
        bounces = p.bounces(k);
        pixel = p.pixel(k);
        gen = p.gen(k);
        rs = Rng{p.rd(k), p.r0(k), p.r1(k), p.r2(k), p.r3(k), p.r4(k)};
        beta = mk(p.br(k), p.bg(k), p.bb(k));
    };
    // hand a finished slot back to the pools: the lockstep rounds of the final generation continue from there
    auto store_slot = [&](int k) {
        p.bounces(k) = bounces;
        p.pixel(k) = pixel;
        p.gen(k) = gen;
        p.hit_info(k) = -1;
        p.stmax(k) = -1.f;
        p.br(k) = beta.x;
        p.bg(k) = beta.y;
        p.bb(k) = beta.z;
        p.rd(k) = rs.d;
        p.r0(k) = rs.v0;
        p.r1(k) = rs.v1;
        p.r2(k) = rs.v2;
        p.r3(k) = rs.v3;
        p.r4(k) = rs.v4;
    };
    auto cold_save = [&]() {
        cold[0 * kBlock] = bounces;
        cold[1 * kBlock] = pixel;
        cold[2 * kBlock] = gen;
        cold[3 * kBlock] = (int)rs.d;
        cold[4 * kBlock] = (int)rs.v0;
        cold[5 * kBlock] = (int)rs.v1;
        cold[6 * kBlock] = (int)rs.v2;
        cold[7 * kBlock] = (int)rs.v3;
        cold[8 * kBlock] = (int)rs.v4;
        cold[9 * kBlock] = __float_as_int(beta.x);
        cold[10 * kBlock] = __float_as_int(beta.y);
        cold[11 * kBlock] = __float_as_int(beta.z);
    };
    auto cold_rng = [&]() {
        return Rng{(uint32_t)cold[3 * kBlock], (uint32_t)cold[4 * kBlock], (uint32_t)cold[5 * kBlock],
                   (uint32_t)cold[6 * kBlock], (uint32_t)cold[7 * kBlock], (uint32_t)cold[8 * kBlock]};
    };
    auto cold_load = [&]() {
        bounces = cold[0 * kBlock];
        pixel = cold[1 * kBlock];
        gen = cold[2 * kBlock];
        rs = cold_rng();
        beta = mk(__int_as_float(cold[9 * kBlock]), __int_as_float(cold[10 * kBlock]), __int_as_float(cold[11 * kBlock]));
    };
    // the GEN block's view of the column: it reads the generation counter and the RNG, and writes back what gen() leaves in any
    // case -- bounces (0, or the kDone / kParked sentinel), gen, the RNG
    auto cold_save_gen = [&](int b, int g, const Rng &r) {
        cold[0 * kBlock] = b;
        cold[2 * kBlock] = g;
        cold[3 * kBlock] = (int)r.d;
        cold[4 * kBlock] = (int)r.v0;
        cold[5 * kBlock] = (int)r.v1;
        cold[6 * kBlock] = (int)r.v2;
        cold[7 * kBlock] = (int)r.v3;
        cold[8 * kBlock] = (int)r.v4;
    };
    int phase = PH_IDLE;
    int tri = -1;
    // the ray being traced, and the traversal cursor (`tri`: best hit so far / excluded triangle;
    // `hu` doubles as the occluded flag of a shadow ray, exactly as in k_trace).  Between the end of
    // a closest-hit trace and the ADV block, (tri, hu, hv, d) ARE the hit record.
    V3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
    float tmax = 0.f, hu = 0.f, hv = 0.f;
    int cur = kEntryDone, sp = 0;
    // hand a slot that has no camera ray left (or is parked for the lockstep final generation) back to the pools and take
    // the lane's next one; `first_phase`: what an untouched slot does first (its bounces = INT_MAX makes that a gen())
    auto next_slot = [&](int first_phase) {
        cold_load();
        store_slot(i);
        phase = PH_IDLE;
        tri = -1;
        slot_set++;
        i = slot_of(slot_set, threadIdx.x);
        if (i < ap_n) {
            load_slot(i);
            if (bounces != kDone && bounces != kParked) {
                phase = first_phase;
                cold_save();
                cold[12 * kBlock] = -1;
            } else {
                i = ap_n;  // (cannot happen: untouched slots start alive)
            }
        }
    };
    // Speculative traversal (kSpeculate): a lane that reaches a leaf inside a node block does not stop there -- it sets
    // the leaf aside in `pend` and goes on with the next stack entry, so the up-to-8 node steps of a block are used by
    // most lanes to the end (without it half of them idle from the middle of the block on), and the triangle block
    // finds two leaves per lane.  The triangles of the postponed leaf are tested a little later, with whatever tmax the
    // ray has then: the closest hit is the minimum over the accepted hits whatever the order (ties: closest_hit_wins),
    // an occluder is an occluder whenever it is found; the price is a few node visits a fresher tmax would have culled.
    int pend = kEntryDone;
    acc[0 * kBlock] = acc[1 * kBlock] = acc[2 * kBlock] = 0.f;
    if (chunk_start) {
        i = ap_n;  // no slot yet: a lane in PH_GEN without a slot draws a task in the GEN block
        phase = PH_GEN;
        cold[12 * kBlock] = -1;
    } else if (i < ap_n) {
        load_slot(i);
        phase = (bounces != kDone && bounces != kParked) ? (SPLIT_GEN ? PH_GEN : PH_ADV) : PH_IDLE;  // (untouched slots: bounces = INT_MAX)
        cold_save();
        cold[12 * kBlock] = -1;  // no previous pixel
    }
    // wave-uniform event counters
    unsigned long long n_gen = 0, n_shade = 0, n_traced = 0, n_shadow = 0, n_emit = 0, n_deposit = 0, n_rr = 0;
    unsigned n_bg_lane = 0;  // per lane: background camera rays the GEN block passed over (below 2^31 in a frame)
#ifdef RT_TRACE_PROFILE
    unsigned long long pf[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long pf_gen_cycles = 0, pf_fin_cycles = 0, pf_fin_lanes = 0, pf_fin_iters = 0;
    unsigned long long pf_handovers = 0, pf_handover_blocks = 0;  // releases at a chunk's end (lanes), and the GEN blocks that made one
    unsigned long long pf_rr_turns = 0, pf_rr_blocks = 0;  // turns of the Russian-roulette chain the wave went round (a block's longest chain), and the ADV blocks that went round at all
    const unsigned long long pf_t0 = __builtin_readcyclecounter();
    // per lane: the start (cycles since pf_t0) of the last fin section it left with work in hand; from there to the wave's
    // exit the lane sits through whole-wave blocks that do nothing for it (the lane-idle tail)
    unsigned long long pf_last_work = 0;
#endif

    // The SIMD's issue arbiter prefers the OLDEST of its waves.  Left alone, the four waves of a SIMD (one from
    // each of the CU's four resident workgroups) finish in dispatch order at 0.63 / 0.73 / 0.81 / 0.92 of the
    // kernel's duration although they carry the same work, and the SIMD spends the last third of the frame with
    // three, two, one wave -- too few to hide anything.  Rotating the waves' priorities makes them progress
    // together (0.87 .. 0.92; +7 % throughput): every 2^prio_period scheduling decisions a wave takes the next of
    // the four levels, starting from its workgroup's residency rank.  (Steering the priority by measured
    // progress against the grid's average was tried and is worse than the plain rotation.)
    unsigned prio_tick = 0;
    const unsigned prio_rank = (4u * blockIdx.x) / gridDim.x;
    while (true) {
        RT_MARK("loop.head");
        if (prio_period && (prio_tick++ & ((1u << prio_period) - 1u)) == 0u) {
            unsigned lvl = ((prio_tick >> prio_period) + prio_rank) & 3u;
            // ties go to the older wave, which left the two younger waves of a SIMD 5 % behind the two older ones;
            // never dropping them to the lowest level evens that out (ranks finish at 0.95 .. 0.97 of the frame)
            lvl = max(lvl, prio_rank >> 1);
            switch (lvl) {
                case 0: __builtin_amdgcn_s_setprio(0); break;
                case 1: __builtin_amdgcn_s_setprio(1); break;
                case 2: __builtin_amdgcn_s_setprio(2); break;
                default: __builtin_amdgcn_s_setprio(3); break;
            }
        }
        // ---- what each lane wants next: the ADV block, a node step, or triangle tests
        bool trav = phase == PH_ANY || phase == PH_CLOSEST;
        bool want_node = trav && cur >= 0;
        bool want_tri = trav && ((cur != kEntryDone && cur < 0) || (kSpeculate && pend != kEntryDone));
        int n_adv = wave_count((phase == PH_ADV));
        const int n_genw = wave_count((phase == PH_GEN));
        int n_node = wave_count((want_node));
        int n_tri = wave_count((want_tri));
        if (n_adv + n_genw + n_node + n_tri == 0) break;
        // After a GEN or ADV block the wave goes straight on to the traversal blocks of this scheduling round (its lanes have
        // just been given rays at the root): the lanes' wishes are taken again and the round trip through the loop head is
        // saved (+3.8 % on C2).
        auto retake = [&]() {
            trav = phase == PH_ANY || phase == PH_CLOSEST;
            want_node = trav && cur >= 0;
            want_tri = trav && ((cur != kEntryDone && cur < 0) || (kSpeculate && pend != kEntryDone));
            n_adv = wave_count((phase == PH_ADV));
            n_node = wave_count((want_node));
            n_tri = wave_count((want_tri));
        };
        // Every block is issued for the whole wave whatever the number of lanes that need it.  The ADV
        // block is ~15x longer than a node step or a triangle test, so it waits for `adv_batch` lanes
        // unless nothing else can run, and the ADV lanes must also be at least half as many as the node and as the triangle
        // lanes.  (Requiring a full majority measured 1 % slower.  Dropping the half condition is as fast in logic, but when
        // the kernel sat exactly at 128 VGPRs that source shape tipped the register allocation into 21 spills: -6 %.  The
        // kernel has since come down to 115, but `make resource-usage` after any edit here all the same: "VGPRs Spill" of
        // k_paths<..., 4, ...> must stay 0 (a CPU test checks it).)
        const bool run_adv = n_adv > 0 && ((n_adv >= adv_batch && 2 * n_adv >= n_node && 2 * n_adv >= n_tri) || n_node + n_tri == 0);
        // ---------------- GEN block: gen() (render.cuh:250-275) for the lanes whose path certainly ended -- it missed
        // or ran out of bounces (a third of all ADV work), or the ADV block found it Russian-roulette-killed to the
        // last bounce.  A tenth of the ADV block's length, so it runs for far fewer waiting lanes.
        if (SPLIT_GEN && !run_adv && n_genw > 0 && (n_genw >= gen_batch || n_node + n_tri == 0)) {
            RT_MARK("gen.begin");
#ifdef RT_TRACE_PROFILE
            pf[12]++; pf[15] += n_genw;
            const unsigned long long pf_tg = __builtin_readcyclecounter();
#endif
            // (what the block changes in the lane's loop-carried registers is applied by selects after the divergent part,
            // and the rare hand-back of a finished slot sits behind a wave-uniform branch: as assignments inside the
            // branches these cost the wave ~45 register moves per GEN block at the merges)
            AdvanceOut out;
            out.did_gen = out.new_ray = false;
            out.ray_o = o;
            out.ray_d = d;
            bool hand_back = false;
            long long my_cid = -1;
            int my_plo = 0, my_phi = 0;  // (a counted frame: where the lane's drawn id's pixel lies)
            if (draw_cids) {
                const unsigned long long m = wave_ballot(phase == PH_GEN);
                const int need = (int)__popcll(m), rank = (int)prefix_popc(m);
                int served = 0;
                while (served < need) {
                    if (cid_next == cid_end) {
                        unsigned base = 0;
                        if (lane_id() == 0) base = atomicAdd(next_cid, (unsigned)kCidChunk);
                        // (past the frame's end: "none left".  The clamp leaves room for cid_end = cid_next + kCidChunk below
                        // INT_MAX; ids that large are never rendered anyway: render_shard_impl refuses frames whose camera-ray
                        // ids come within 13 W of 2^31, and a wave overshoots the frame's end by at most one chunk)
                        static_assert(0x7ffff000u + (unsigned)kCidChunk < 0x7fffffffu, "cid_end must not overflow int");
                        cid_next = (int)min(__builtin_amdgcn_readfirstlane(base), 0x7ffff000u);
                        cid_end = cid_next + kCidChunk;
                        if constexpr (BUILD::kCounts) {
                            const int ids = __builtin_amdgcn_readfirstlane((int)ap.cam_end);  // (below 2^31 - 13 W: render_shard_impl)
                            if (cid_next < ids) {  // (a chunk past the frame's end is not looked up: its lanes stop)
                                const int n_px = __builtin_amdgcn_readfirstlane(cam.n_pixels);
                                cid_plo = __builtin_amdgcn_readfirstlane(counts_find_wave(cam.offset, 0, n_px - 1, (unsigned)cid_next));
                                cid_phi = __builtin_amdgcn_readfirstlane(counts_find_wave(cam.offset, cid_plo, n_px - 1, (unsigned)(min(cid_end, ids) - 1)));
                                cid_win = cam.offset[min(cid_plo + (int)lane_id(), n_px)];  // (offset[n_px]: the total, above every id)
                            }
                        }
                    }
                    const int take = min(need - served, cid_end - cid_next);
                    if constexpr (BUILD::kCounts) {
                        // (every lane of the wave makes the six shuffles, also those that take no id here: their result is dropped.
                        // The window's offsets do not decrease and its first is at most the chunk's first id, so the last lane whose
                        // offset is at most c holds c's pixel -- unless that is the window's last lane.)
                        const int c_here = cid_next + max(rank - served, 0);
                        int win_at = 0;
#pragma unroll
                        for (int s = 32; s > 0; s >>= 1) win_at = __shfl(cid_win, win_at + s) <= (unsigned)c_here ? win_at + s : win_at;
                        if (phase == PH_GEN && rank >= served && rank < served + take) {
                            my_cid = c_here;
                            my_plo = min(cid_plo + win_at, cid_phi);
                            my_phi = win_at < 63 ? my_plo : cid_phi;
                        }
                    } else {
                        if (phase == PH_GEN && rank >= served && rank < served + take) my_cid = cid_next + (rank - served);
                    }
                    cid_next += take;
                    served += take;
                }
            }
            const unsigned chunk_g = CHUNKS ? __builtin_amdgcn_readfirstlane(s_task[1]) : 0u;
            // the skipping build: the deal's other words, out of the LDS once per block and as scalars: [2 .. 3] and [4 .. 7] in one
            // read each
            unsigned tk_inv = 1u, tk_shift = 0u, tk_limit = 0u, tk_head = 0u, tk_mul = 0u;
            if constexpr (BUILD::kBg && CHUNKS) {
                const uint2 lo = *(const uint2 *)&s_task[2];
                const uint4 hi = *(const uint4 *)&s_task[4];
                tk_inv = __builtin_amdgcn_readfirstlane(lo.x);
                tk_shift = __builtin_amdgcn_readfirstlane(lo.y);
                tk_limit = __builtin_amdgcn_readfirstlane(hi.x);
                tk_head = __builtin_amdgcn_readfirstlane(hi.y);
                tk_mul = __builtin_amdgcn_readfirstlane(hi.z);
            }
            // the chunked deal's static head where the block needs it again: the skipping build has read it once, as a scalar
            auto gen_chunk_head = [&]() { return BUILD::kBg ? (int)tk_head : (int)s_task[5]; };
            // The camera ray that ended: its sum goes to its pixel AFTER the hand-over (whose waits for the state's stores and
            // loads would otherwise also sit through the float atomics' acknowledgements), so the pixel is read before the
            // hand-over puts another slot's state into the lane's column.  A lane that comes without a slot has an empty sum.
            const bool chunk_was_gen = CHUNKS && phase == PH_GEN;
            const int chunk_acc_pixel = CHUNKS ? cold[1 * kBlock] : 0;
            if (CHUNKS && chunk_g) {
                const rtchunks::Multiple chunk_m = BUILD::kBg ? rtchunks::Multiple{tk_inv, tk_shift, tk_limit} : rtchunks::Multiple{s_task[2], s_task[3], s_task[4]};
                const unsigned chunk_head = BUILD::kBg ? tk_head : __builtin_amdgcn_readfirstlane(s_task[5]);
                // A lane past its static head: without a slot it takes one; with its slot at a chunk's end it banks it (or keeps
                // it, if another lane has left a claim) -- rt_slot_chunks.h.  Behind a wave vote: once per G camera rays of a lane.
                // (a lane inside its static head, slot_set < head, has a slot until the head is done and is at no chunk's end)
                bool need = phase == PH_GEN && i >= ap_n;
                const bool at_end = phase == PH_GEN && i < ap_n && slot_set >= (int)chunk_head &&
                                    rtchunks::chunk_ends((unsigned)cold[2 * kBlock], chunk_m, cold[0 * kBlock] == kChunkFresh);
                if (wave_ballot(need || at_end)) {
#ifdef RT_TRACE_PROFILE
                    bool pf_released = false;
#endif
                    if (at_end) {
                        cold_load();
                        // (a chain at its end is not banked: gen() below hands the slot back for good)
                        const bool ends = gen == ap.last_gen || (long long)gen * kW + (ap.slot_lo + i) >= ap.cam_end;
                        if (!ends) {
                            bounces = ap_max_bounces;  // alive, starts with gen() (as k_pool_init leaves a slot)
                            store_slot(i);
                            // the slot's entry among the workgroup's dealt ones
                            const rtchunks::Owner own = rtchunks::owner_of((unsigned)i, (unsigned)lanes_in_grid, (unsigned)rot_wave, (unsigned)rot_set);
                            const unsigned idx = (own.set - chunk_head) * rtchunks::kLanes + (own.lane_in_grid & (rtchunks::kLanes - 1u));
#if RT_CHUNK_RELEASE_WAIT
                            // vmcnt(0): the state's stores are acknowledged before the semaphore says so.  (At workgroup scope
                            // the compiler's release does not wait for them: it relies on one CU's vector memory operations
                            // reaching its L1 in the order they were issued.  The semaphore goes through the LDS, not that queue.)
                            __builtin_amdgcn_s_waitcnt(0x0f70);
#endif
                            const unsigned old = __hip_atomic_fetch_add(&s_sem[rtchunks::sem_word(idx) & (rtchunks::kSemWords - 1u)], rtchunks::sem_unit(idx),
                                                                        __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                            if (!rtchunks::runner_keeps(rtchunks::sem_value(old, idx))) {
                                i = ap_n;
                                need = true;
                            }
#ifdef RT_TRACE_PROFILE
                            pf_released = true;
#endif
                        }
                    }
#ifdef RT_TRACE_PROFILE
                    pf_handovers += wave_count(pf_released);
                    pf_handover_blocks += wave_ballot(pf_released) != 0 ? 1 : 0;
#endif
                    // dealt slots per lane (lanes_in_grid divides the shard); a slot's chain in this kernel: generations 0 .. last_gen - 1
                    const unsigned chunk_sets = (unsigned)ap_n / (unsigned)lanes_in_grid - chunk_head;
                    const unsigned chunk_tasks = rtchunks::task_count(chunk_sets, (unsigned)ap.last_gen, (unsigned)chunk_g);
                    // (every turn of this loop deals tasks: it ends when the lanes have a slot each or the tasks are out)
                    unsigned long long m;
                    while ((m = wave_ballot(need)) != 0ull) {
                        unsigned base = 0;
                        if (lane_id() == 0) base = atomicAdd(&s_task[0], (unsigned)__popcll(m));
                        const unsigned t = __builtin_amdgcn_readfirstlane(base) + prefix_popc(m);
                        if (need) {
                            if (t >= chunk_tasks) {
                                need = false;
                                phase = PH_IDLE;  // out of tasks: this lane is done (i = ap_n)
                            } else {
                                const rtchunks::Entry e = rtchunks::task_entry(t, chunk_sets);
                                const int k = slot_of((int)(e.set + chunk_head), e.lane);
                                const unsigned idx = e.set * rtchunks::kLanes + e.lane;
                                const unsigned old = k < ap_n ? __hip_atomic_fetch_sub(&s_sem[rtchunks::sem_word(idx) & (rtchunks::kSemWords - 1u)], rtchunks::sem_unit(idx),
                                                                                       __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)
                                                              : rtchunks::kSemBias;  // (no such slot: as a claim)
                                if (rtchunks::taker_runs(rtchunks::sem_value(old, idx))) {
                                    i = k;
                                    load_slot(i);
                                    cold_save();
                                    // (gen() is the slot's next step whatever `bounces` says and overwrites it: until then the word
                                    // marks the slot as fresh on this lane -- a bit of its own, not borrowed from the pixel stepping)
                                    cold[0 * kBlock] = kChunkFresh;
                                    cold[12 * kBlock] = -1;  // no previous pixel on this lane
                                    need = false;
                                }
                            }
                        }
                    }
                }
            }
            if (CHUNKS) {
                // (vmcnt(0), nothing else.  The compiler cannot tell at this merge whether the hand-over's loads are in, and waits
                // for them at the first use of a register they wrote: left alone that is BEHIND the atomics below, whose
                // acknowledgements every GEN block would then sit through.  Here it costs what the same wait cost in front
                // of the flush before: nothing, unless a hand-over has just been made.)
                __builtin_amdgcn_s_waitcnt(0x0f70);
                // (also for a lane that banked its slot and found the tasks out: it is idle from here on)
                if (chunk_was_gen) acc_flush(acc, fb, ap_fb_fixed, chunk_acc_pixel);
            }
            if constexpr (BUILD::kBg) {
                // The pinhole's gen(), as a wave-level loop that passes over background pixels (gen_background): a lane whose
                // next camera ray cannot hit anything counts it, makes its two jitter draws and takes its slot's next generation
                // in the same visit -- no ray, no scheduling round, no root node step, no second visit.  The block waits for
                // the lane with the longest run, so a turn of the loop is kept to what changes from one camera ray to the next:
                // the generation counter, the pixel stepped by (dpx, dpy), the rectangle test, the two steps of the XORWOW shift
                // register, and ONE stop test, `background and below g_limit`.  Everything that can end a run but a pixel inside
                // the rectangle is folded into g_limit before the loop (rtchunks::run_limit): the end of the slot's chain
                // (g_stop), for a dealt lane the next chunk's end, and one turn where the pixel cannot be stepped (dpy < 0) or
                // in the per-sample mode.  What the turns add up to is taken after the loop from the number of turns: the Weyl
                // word of the stream, the two draws (the last two words of the register: the jitter if the pixel is not
                // background) and the count of passed rays.  The rest of gen() -- divisions, camera.get_ray -- stands outside
                // too, and the frame's words come out of the LDS once, as scalars.
                // A lane leaves the loop with a ray to make; at the end of its chain (kDone / kParked: hand_back below); where
                // its dealt chain reaches a chunk's end (it keeps PH_GEN: the next GEN block makes the hand-over, so the
                // semaphores see what they saw without the loop); after its one turn where it has no more (it keeps PH_GEN; in
                // the per-sample mode a background id is dropped without starting its stream and the lane draws another id in
                // the next GEN block).
                static_assert((kW & (kW - 1)) == 0, "a slot's camera rays are counted with a shift");
                const bool was_gen = phase == PH_GEN;
                const int f_width = __builtin_amdgcn_readfirstlane(ap.width), f_dpx = __builtin_amdgcn_readfirstlane(ap.dpx);
                const int f_dpy = __builtin_amdgcn_readfirstlane(ap.dpy), f_last_gen = __builtin_amdgcn_readfirstlane(ap.last_gen);
                const int f_cam_end = __builtin_amdgcn_readfirstlane((int)ap.cam_end);  // (below 2^31 - 13 W: render_shard_impl)
                const int f_slot_lo = __builtin_amdgcn_readfirstlane(ap.slot_lo);
                const int f_x0 = __builtin_amdgcn_readfirstlane(ap.bg_x0), f_y0 = __builtin_amdgcn_readfirstlane(ap.bg_y0);
                const unsigned f_w = (unsigned)__builtin_amdgcn_readfirstlane(ap.bg_w), f_h = (unsigned)__builtin_amdgcn_readfirstlane(ap.bg_h);
                const bool can_loop = !draw_cids && f_dpy >= 0;
                // (the deal's words are scalars of this block only: nothing of the deal lives across the main loop)
                const bool dealt = CHUNKS && chunk_g && slot_set >= (int)tk_head;
                Rng g_rs{0, 0, 0, 0, 0, 0};
                int g_gen = 0, g_stop = 0, g_limit = 0, px = 0, py = 0;
                uint32_t draw_x = 0, draw_y = 0;
                bool looking = false, made = false;  // made: the pixel the lane stopped at is not background
                unsigned long long my_key = 0;  // (a counted frame) p * stride + k of the lane's drawn id
                if (was_gen) {
                    g_gen = cold[2 * kBlock];
                    g_rs = cold_rng();
                    const int pxy = cold[12 * kBlock];
                    if (!CHUNKS) acc_flush(acc, fb, ap_fb_fixed, cold[1 * kBlock]);  // the camera ray that ended: its sum -> its pixel
                    // the generation at which gen()'s end tests stop the slot: its camera rays run out (gen W + slot >= cam_end)
                    // or the lockstep final generation begins; a drawn id stops the lane if it lies past the frame
                    const int slot = f_slot_lo + i;
                    if (draw_cids) g_stop = my_cid >= (long long)f_cam_end ? g_gen : 0x7fffffff;
                    else g_stop = min(f_last_gen, (f_cam_end - slot + (kW - 1)) >> __builtin_ctz((unsigned)kW));
                    looking = g_gen < g_stop;
                    g_limit = (int)rtchunks::run_limit((unsigned)g_gen, (unsigned)g_stop, dealt, can_loop, chunk_g, tk_mul);
                    px = pxy & 0xffff;
                    py = pxy >> 16;
                    if (looking && (pxy < 0 || !can_loop)) {
                        // no previous pixel on this lane, or none to step from (odd spp, a frame too large, a drawn id): the next
                        // pixel by gen()'s divisions, stepped BACK once -- the loop's first turn steps it forward again.  The id
                        // is below cam_end here (g_gen < g_stop), so below 2^31, and gen_pixel's form for a given id divides in
                        // 32 bits: the same integers as the 64-bit quotient.
                        SlotState t;
                        t.gen = g_gen + 1;
                        int qx, qy;
                        const unsigned cid32 = draw_cids ? (unsigned)my_cid : (unsigned)g_gen * (unsigned)kW + (unsigned)slot;
                        if constexpr (BUILD::kCounts) {
                            static_assert(DRAW_CIDS || !SPLIT_GEN, "a counted frame's GEN block serves drawn ids only");
                            counts_locate(cam, cid32, my_plo, my_phi, f_width, t.pixel, qx, qy, my_key);
                        } else {
                            gen_pixel(ap, slot, t, nullptr, (long long)cid32, (long long)cid32, qx, qy);
                        }
                        px = qx - f_dpx;
                        py = qy - f_dpy;
                        if (px < 0) {
                            px += f_width;
                            py--;
                        }
                    }
                }
                if (looking) {
                    // (a lane's own loop: the lanes that are through drop out of the execution mask, and a turn moves no register
                    // for them -- as `while (wave_ballot(looking)) if (looking) ...` it cost 25 register moves per turn)
                    bool bg;
                    const int g_entry = g_gen;
                    RT_MARK("gen.loop.begin");
                    do {
                        g_gen++;
                        // the pixel stepped by (dpx, dpy) with the carry of a row's end: px + dpx < 2 width, so the wrapped
                        // column is the smaller of the two as unsigned numbers
                        px += f_dpx;
                        const bool wrap = px >= f_width;
                        px = (int)min((unsigned)px, (unsigned)(px - f_width));
                        py += f_dpy + (wrap ? 1 : 0);
                        bg = ((unsigned)(px - f_x0) >= f_w) | ((unsigned)(py - f_y0) >= f_h);  // gen_background
                        if (!draw_cids) {  // x first, then y (Appendix A.7): the slot's stream moves on as the reference's does
                            rng_step(g_rs);
                            rng_step(g_rs);
                        }
                    } while (!draw_cids && (bg & (g_gen < g_limit)));  // (per-sample mode: one turn, known when compiled)
                    RT_MARK("gen.loop.end");
                    // (the test again, on the pixel the lane stopped at: carried out of the loop, the bit costs every turn three
                    // scalar instructions that keep it for the lanes already through.  The empty statement emits nothing: it
                    // keeps the compiler from finding the loop's own test in this one and carrying the bit after all.)
                    __asm__ volatile("" : "+v"(px), "+v"(py));
                    made = !(((unsigned)(px - f_x0) >= f_w) | ((unsigned)(py - f_y0) >= f_h));
                    const uint32_t turns = (uint32_t)(g_gen - g_entry);
                    // counted as the camera rays they are (camera_rays, closest_rays): summed at the exit
                    n_bg_lane += turns - (made ? 1u : 0u);
                    if (draw_cids) {  // (every camera ray starts a stream of its own: none for a background id)
                        if (made) {
                            if constexpr (BUILD::kCounts) g_rs = rng_sample_stream(ap.seed_lo, ap.seed_hi, my_key);
                            else g_rs = rng_sample_stream(ap.seed_lo, ap.seed_hi, (unsigned long long)my_cid * (unsigned)ap.key_mul + (unsigned)ap.key_add);
                            draw_x = rng_next(g_rs);
                            draw_y = rng_next(g_rs);
                        }
                    } else {  // rng_next's Weyl word for 2 draws a turn; a draw is the register's newest word plus the Weyl word then
                        static_assert(2u * kRngWeyl < (1u << 24), "a 24-bit multiply");  // (turns <= 2 047)
                        g_rs.d += __umul24(turns, 2u * kRngWeyl);
                        draw_x = g_rs.v3 + (g_rs.d - kRngWeyl);
                        draw_y = g_rs.v4 + g_rs.d;
                    }
                }
                if (made) {
                    camera_get_ray(cam, (px + rng_to_uniform(draw_x)) / ap.width, (py + rng_to_uniform(draw_y)) / ap.height, out.ray_o, out.ray_d);
                    out.new_ray = true;
                    out.did_gen = true;
                }
                if (was_gen) {
                    // the slot state gen() leaves (cold_save_gen), and the stepped pixel coordinates; a new path also has its pixel and
                    // beta = 1
                    int b = 0;
                    if (!made && g_gen >= g_stop) {  // gen()'s end tests, in their order
                        const long long cid = my_cid >= 0 ? my_cid : (long long)g_gen * kW + (f_slot_lo + i);
                        b = cid >= ap.cam_end ? kDone : kParked;
                        hand_back = true;  // (otherwise, without a ray: the lane keeps PH_GEN)
                    }
                    cold_save_gen(b, g_gen, g_rs);
                    cold[12 * kBlock] = px | (py << 16);
                    if (made) {
                        cold[1 * kBlock] = py * f_width + px;
                        cold[9 * kBlock] = __float_as_int(1.f);
                        cold[10 * kBlock] = __float_as_int(1.f);
                        cold[11 * kBlock] = __float_as_int(1.f);
                    }
                }
            } else if (phase == PH_GEN) {
                SlotState st;
                st.gen = cold[2 * kBlock];
                st.rs = cold_rng();
                st.bounces = 0;
                st.pixel = 0;
                st.beta = mk(0, 0, 0);
                int pxy = cold[12 * kBlock];
                if (!CHUNKS) acc_flush(acc, fb, ap_fb_fixed, cold[1 * kBlock]);  // the camera ray that ended: its sum -> its pixel
                gen_core<true>(cam, ap, ap.slot_lo + i, st, out, &pxy, my_cid);
                // the slot state gen() leaves (cold_save_gen); a new path also has its pixel and beta = 1
                cold_save_gen(st.bounces, st.gen, st.rs);
                if (out.new_ray) {
                    cold[1 * kBlock] = st.pixel;
                    cold[9 * kBlock] = __float_as_int(st.beta.x);
                    cold[10 * kBlock] = __float_as_int(st.beta.y);
                    cold[11 * kBlock] = __float_as_int(st.beta.z);
                    cold[12 * kBlock] = pxy;
                } else {
                    hand_back = true;  // out of camera rays, or parked for the lockstep final generation
                }
            }
            const bool nr = out.new_ray;
            o = out.ray_o;
            d = out.ray_d;
            inv = inv_dir(d);  // (for every lane, as after the ADV block: the same value for the lanes that keep their ray)
            phase = nr ? (int)PH_CLOSEST : phase;
            tmax = nr ? kFltMax : tmax;
            tri = nr ? -1 : tri;
            cur = nr ? 0 : cur;
            sp = nr ? 0 : sp;
            if (wave_ballot(hand_back)) {  // rare (once per slot and frame): kept out of the merges above
                if (hand_back) {
                    if (draw_cids) {
                        phase = PH_IDLE;  // (the frame's counter has run out: nothing is tied to this lane's slot)
                    } else if (CHUNKS && chunk_g && slot_set + 1 >= gen_chunk_head()) {
                        // a dealt slot, or the last one of the static head, is finished: its final state goes to the pools, the
                        // lane draws a task next
                        cold_load();
                        store_slot(i);
                        i = ap_n;
                        tri = -1;
                        slot_set = gen_chunk_head();
                    } else {  // (the static deal, or the static head of the chunked one: the lane's own next slot)
                        next_slot(PH_GEN);
                    }
                }
            }
            n_gen += wave_count((out.did_gen));
            n_traced += wave_count((out.new_ray));
#ifdef RT_TRACE_PROFILE
            pf_gen_cycles += __builtin_readcyclecounter() - pf_tg;
#endif
            retake();
            RT_MARK("gen.end");
        }
        if (run_adv) {
#ifdef RT_TRACE_PROFILE
            pf[0]++; pf[1] += n_adv;
            const unsigned long long pf_ta = __builtin_readcyclecounter();
#endif
            // ---------------- ADV block
            RT_MARK("adv.head");
            AdvanceOut out;
            out.did_gen = out.did_shade = out.has_shadow = out.did_emit = out.new_ray = false;
            out.rr_draws = 0;
            out.bg_skipped = 0;
            if (phase == PH_ADV) {
                // the slot state is only live between cold_load() and cold_save() below
                cold_load();
                SlotState st;
                st.wo = d;
                st.hit_info = -1;
                st.isect_p = st.isect_n = mk(0, 0, 0);
                if (tri >= 0) {  // hit record in the form mat() consumes (render.cuh:152-153, 311-316)
                    Tri tr = load_tri(sc.tris, tri);
                    float4 sh = sc.tri_shade[(unsigned)tri];
                    RT_MARK("adv.verify");
                    if (VERIFY) {
                        // (o, d) are still the path ray that ended on `tri`.  A set sign bit of hv: an exact tie at the final
                        // distance (triangle block) -- or a v of -0.0, which costs a needless, equally exact re-trace
                        bool bad = (__float_as_uint(hv) >> 31) != 0u;
                        if (bad) atomicAdd(&vstat[V_TIE], 1ull);
                        else bad = !ref_visible(sc, o, d, tr, tri, vstat);
                        if (bad) {
                            atomicAdd(&vstat[V_LITERAL], 1ull);
                            float tm = kFltMax;
                            tri = -1;
                            hu = hv = 0.f;
                            reference_walk<false>(sc, o, d, tm, tri, hu, hv, stack, over, stack_cap);
                            cold_load();  // (again: what was loaded above need not stay in registers across the walk)
                            if (tri >= 0) {
                                tr = load_tri(sc.tris, tri);
                                sh = sc.tri_shade[(unsigned)tri];
                            }
                        }
                    }
                    RT_MARK("adv.hit_record");
                    if (!VERIFY || tri >= 0) {
                        st.isect_p = tri_point(tr, hu, hv);
                        st.isect_n = mk(sh.x, sh.y, sh.z);
                        st.hit_info = __float_as_int(sh.w);
                    }
                }
                st.bounces = bounces;
                st.pixel = pixel;
                st.gen = gen;
                st.rs = rs;
                st.beta = beta;
                advance_core<SPLIT_GEN, true, true, BUILD::kBg>(sc, tab, cam, ap, ap.slot_lo + i, st, out, fb, acc);
                RT_MARK("adv.tail");
                bounces = st.bounces;
                pixel = st.pixel;
                gen = st.gen;
                rs = st.rs;
                beta = st.beta;
                if (out.has_shadow) {
                    park[0 * kBlock] = out.ray_o.x;
                    park[1 * kBlock] = out.ray_o.y;
                    park[2 * kBlock] = out.ray_o.z;
                    park[3 * kBlock] = out.ray_d.x;
                    park[4 * kBlock] = out.ray_d.y;
                    park[5 * kBlock] = out.ray_d.z;
                    park[6 * kBlock] = out.s_L.x;
                    park[7 * kBlock] = out.s_L.y;
                    park[8 * kBlock] = out.s_L.z;
                    o = out.s_o;
                    d = out.s_d;
                    phase = PH_ANY;
                    tmax = out.s_tmax;
                    tri = out.s_target;
                    hu = 0.f;
                } else if (out.new_ray) {
                    o = out.ray_o;
                    d = out.ray_d;
                    phase = PH_CLOSEST;
                    tmax = kFltMax;
                    tri = -1;
                } else if (SPLIT_GEN) {
                    phase = PH_GEN;  // out.wants_gen: Russian roulette ended the path (its draws are in rs)
                    tri = -1;
                } else {
                    // this slot is out of camera rays (or parked for the lockstep final generation)
                    cold_save();
                    next_slot(PH_ADV);
                }
                if (phase == PH_ANY || phase == PH_CLOSEST) {
                    cur = 0;
                    sp = 0;
                }
                // (the same treatment as in the GEN block -- selects after the divergent part -- was measured here and
                // loses 1 %: the shading block's exits are three-way and the selects outnumber the moves they replace)
                if (phase != PH_IDLE) cold_save();
            }
            // 1 / d for EVERY lane, also those that only sat through the block: three v_rcp_f32, and 1 / d does not have
            // to stay in registers across the ~1 100 vector instructions of the block (three registers that decided
            // between a build with and without spills when the kernel sat at 128 VGPRs)
            inv = inv_dir(d);
            if (!SPLIT_GEN) n_gen += wave_count((out.did_gen));
            if (!SPLIT_GEN && BUILD::kBg) {
                // the background camera rays gen() passed over inside advance_core: camera rays like the others
                int bg = out.bg_skipped;
                if (wave_ballot(bg != 0)) {
                    for (int off = 32; off > 0; off >>= 1) bg += __shfl_xor(bg, off);
                    n_gen += (unsigned long long)bg;
                    n_traced += (unsigned long long)bg;
                }
            }
            n_shade += wave_count((out.did_shade));
            n_traced += wave_count((out.new_ray));
            n_shadow += wave_count((out.has_shadow));
            n_emit += wave_count((out.did_emit));
            int rr = out.rr_draws;
            if (wave_ballot(rr != 0)) {
                for (int off = 32; off > 0; off >>= 1) rr += __shfl_xor(rr, off);
                n_rr += (unsigned long long)rr;
            }
#ifdef RT_TRACE_PROFILE
            pf[8] += __builtin_readcyclecounter() - pf_ta;
            {  // (behind the block's clock: the chain's turns are the longest lane's rolls)
                int turns = out.rr_draws;
                for (int off = 32; off > 0; off >>= 1) turns = max(turns, __shfl_xor(turns, off));
                pf_rr_turns += (unsigned long long)turns;
                pf_rr_blocks += turns != 0 ? 1 : 0;
            }
#endif
            retake();
            RT_MARK("adv.after");
        }
        const bool is_any = phase == PH_ANY;
        // ---------------- node steps for the lanes in `want`
        auto node_block = [&](bool want, int n_want) {
#ifdef RT_TRACE_PROFILE
            pf[2]++; pf[3] += n_want; pf[6] += n_adv;
            const unsigned long long pf_tn = __builtin_readcyclecounter();
#endif
            RT_MARK("node.begin");
            if (LITERAL) {
                if (want) {
                    if (is_any) reference_walk<true>(sc, o, d, tmax, tri, hu, hv, stack, over, stack_cap);
                    else reference_walk<false>(sc, o, d, tmax, tri, hu, hv, stack, over, stack_cap);
                    cur = kEntryDone;
                }
            } else if (want) {
                // a bounded while-while: up to kNodePerStep consecutive node steps (2 triangle tests in the
                // triangle block) per scheduling decision -- measured best at 8 / 2 (+22 % over 1 / 1; 4 / 2: +20 %)
                auto step_general = [&]() {
                    if (cur >= 0) {
                        inner_step<WIDE>(sc, o, inv, tmax, cur, sp, stack, over, stack_cap, s_top, top_n);
                    } else if (kSpeculate && cur != kEntryDone && pend == kEntryDone && sp > 0) {
                        pend = cur;  // a leaf: set it aside, go on with the next entry
                        cur = stack_pop(stack, over, sp, stack_cap);
                    }
                };
                // 4-wide nodes on the full pool: ONE wave vote per step decides between the step without any overflow
                // handling (all lanes of the block hold at most stack_cap - 3 entries: 95 % of the steps) and the general one
                auto step = [&]() {
                    if (!WIDE || MIN_WAVES == 2) {
                        step_general();
                    } else if (wave_ballot(sp > stack_cap - 3) == 0ull) {
                        if (cur >= 0) {
                            inner_step<WIDE, true>(sc, o, inv, tmax, cur, sp, stack, over, stack_cap);
                        } else if (kSpeculate && cur != kEntryDone && pend == kEntryDone && sp > 0) {
                            pend = cur;
                            sp--;
                            cur = stack[sp * kBlock];
                        }
                    } else {
                        step_general();
                    }
                };
                if (kNodeCont == 0 || !WIDE) {
#pragma unroll
                    for (int rep = 0; rep < (WIDE ? kNodePerStepWide : kNodePerStep); rep++) step();
                } else {
                    // adaptive: the fixed steps, then kNodeExtra more if enough lanes of the wave still have one to make
#pragma unroll
                    for (int rep = 0; rep < kNodePerStepWide; rep++) step();
                    if (wave_count(cur >= 0) >= kNodeCont) {
#pragma unroll
                        for (int rep = 0; rep < kNodeExtra; rep++) step();
                    }
                }
            }
#ifdef RT_TRACE_PROFILE
            pf[9] += __builtin_readcyclecounter() - pf_tn;
#endif
            RT_MARK("node.end");
        };
        // ---------------- triangle tests (triangle.cuh:39-58) for the lanes in `want`: the leaf reference is the cursor
        auto tri_block = [&](bool want, int n_want) {
#ifdef RT_TRACE_PROFILE
            pf[4]++; pf[5] += n_want; pf[7] += n_adv;
            const unsigned long long pf_tt = __builtin_readcyclecounter();
#endif
            RT_MARK("tri.begin");
            if (want) {
                // kTriPerStep tests per lane, and ALL their triangle records are fetched before the first test: which
                // triangles come next does not depend on the outcome of a test (only whether they are still wanted does: an
                // occluded shadow ray is finished), so the block waits for one memory round trip instead of one per test.
                // The lane's walk through its leaves is made up front on copies of (pend, cur):
                //   the postponed leaf first, then the leaf under the cursor; when the cursor's leaf is used up, the next
                //   stack entry -- popped on the spot: a ray that turns out occluded has no use for its stack any more.
                // Straight-line bookkeeping: every outcome is a select, not a branch (the merges of the branchy version cost
                // the wave ~30 register moves per test); the only branches left are the rare ones (a tie between two hits;
                // a pop from the overflow column).
                int pd = pend, cu = cur;
                int ks[kTriPerStep] = {};  // (0 = a valid triangle address for lanes that have nothing to fetch)
                bool act[kTriPerStep];
                Tri tr[kTriPerStep];
#pragma unroll
                for (int j = 0; j < kTriPerStep; j++) {
                    const bool fp = kSpeculate && pd != kEntryDone;
                    const bool leaf = cu != kEntryDone && cu < 0;
                    act[j] = fp || leaf;
                    const int enc = fp ? pd : cu;  // ~((first << 3) | count)
                    ks[j] = act[j] ? (~enc) >> 3 : ks[0];  // (an address that is valid in any case)
                    const bool more = ((~enc) & 7) > 1;
                    const int rest = more ? enc - 7 : kEntryDone;  // one triangle further: first + 1, count - 1
                    int popped = kEntryDone;
                    // (the same wave vote as in the node step -- no lane has entries in the overflow part -- measured here: +1 %
                    // SLOWER, it undoes the node step's gain: profiles/r05_experiments.md)
                    if (act[j] && !fp && !more && sp > 0) popped = stack_pop(stack, over, sp, stack_cap);
                    pd = (act[j] && fp) ? rest : pd;
                    cu = (act[j] && !fp) ? (more ? rest : popped) : cu;
                    tr[j] = load_tri(sc.tris, ks[j]);
                }
                // the tests, each with the tmax the earlier ones left.  any-hit: the first accepted hit that is not the
                // excluded triangle (bvh.cuh:243); closest-hit: bvh.cuh:227-231 (t <= tmax), ties by closest_hit_wins
                bool occluded = false;
                int occ_j = 0;  // which of the tests found the occluder
#pragma unroll
                for (int j = 0; j < kTriPerStep; j++) {
                    if (act[j] && !occluded) {
                        float t, u, v;
                        const bool hit = tri_intersect(tr[j], o, d, tmax, t, u, v);
                        occluded = hit && is_any && ks[j] != tri;
                        occ_j = occluded ? j : occ_j;
                        bool better = hit && !is_any;
                        if (VERIFY) {
                            // an exact tie is the reference's tree order to decide: the ray is re-traced literally in the ADV block
                            // (the mark is the sign bit of hv; v >= 0 for an accepted hit), so which of the two stays until then
                            // does not matter -- no branch, no look at the caller order
                            const bool tie = better && t == tmax && tri >= 0;
                            v = __uint_as_float(__float_as_uint(v) | (tie ? 0x80000000u : 0u));
                        } else if (better && t == tmax && tri >= 0) {  // (RT_FLAG_WATERTIGHT: ties go to the larger caller index)
                            better = sc.order[(unsigned)ks[j]] > sc.order[(unsigned)tri];
                        }
                        tmax = better ? t : tmax;
                        hu = occluded ? 1.f : (better ? u : hu);
                        hv = better ? v : hv;
                        tri = better ? ks[j] : tri;
                    }
                }
                pend = occluded ? kEntryDone : pd;
                cur = occluded ? kEntryDone : cu;
                // VERIFY: an occluder only counts if the reference's walk can see its triangle (2 % of the shadow rays get here;
                // ONE branch behind both tests: inside each test it cost the block's straight-line shape, 2 % of the frame).  An
                // occluder it cannot see -- ~1 in 10^7 -- says nothing about the rest of the ray: the ray ends here and is
                // re-traced through the reference's own tree in the finished-rays section (hu = 2 marks it)
                if (VERIFY && occluded) {
                    static_assert(kTriPerStep == 2, "the occluder is picked from two records");
                    Tri tq;
                    tq.p0 = occ_j ? tr[1].p0 : tr[0].p0;
                    tq.e1 = occ_j ? tr[1].e1 : tr[0].e1;
                    tq.e2 = occ_j ? tr[1].e2 : tr[0].e2;
                    tq.n = tq.p0;  // (not looked at)
                    if (!ref_visible(sc, o, d, tq, occ_j ? ks[1] : ks[0], vstat)) hu = 2.f;
                }
            }
#ifdef RT_TRACE_PROFILE
            pf[10] += __builtin_readcyclecounter() - pf_tt;
#endif
            RT_MARK("tri.end");
        };
        // Which of the two: the more popular block -- and when that is the node block, the triangle block right behind it
        // for the lanes that hold a leaf BY THEN (at least `tri_follow` of them): a lane that reached a leaf in the node
        // block has its triangles tested in this scheduling round instead of the next one.  Measured on C2: +6.6 % at
        // tri_follow = 1, +5.3 % at 12, +0.4 % at 40; the mirror image (a node block behind a triangle block) buys nothing on
        // top and loses 5 % alone.  (ONE copy of the triangle block in the code: the block behind a node block and the block
        // on its own are the same instructions for different lanes.)
        {
            const bool run_node = n_node > 0 && n_node >= n_tri;
            bool w = want_tri;
            int nw = n_tri;
            if (run_node) {
                node_block(want_node, n_node);
                w = tri_follow > 0 && trav && ((cur != kEntryDone && cur < 0) || (kSpeculate && pend != kEntryDone));
                nw = wave_count(w);
                nw = (tri_follow > 0 && nw >= tri_follow) ? nw : 0;
            }
            if (nw > 0) tri_block(w, nw);
        }
        // ---------------- finished rays
        RT_MARK("fin.begin");
        const bool fin = trav && cur == kEntryDone && (!kSpeculate || pend == kEntryDone);
#ifdef RT_TRACE_PROFILE
        const unsigned long long pf_tf = __builtin_readcyclecounter();
        pf_fin_lanes += wave_count(fin);
        pf_fin_iters += wave_ballot(fin) != 0 ? 1 : 0;
#endif
        if (VERIFY) {  // the shadow rays whose occluder the reference cannot see (triangle block): the literal walk decides
            const bool lit = fin && is_any && hu == 2.f;
            if (wave_ballot(lit)) {
                if (lit) {
                    atomicAdd(&vstat[V_LITERAL], 1ull);
                    float tm = tmax, no_v = 0.f;
                    int excluded = tri;
                    hu = 0.f;
                    reference_walk<true>(sc, o, d, tm, excluded, hu, no_v, stack, over, stack_cap);
                }
            }
        }
        n_deposit += wave_count((fin && is_any && hu == 0.f));
        if (fin) {
            if (is_any) {
                if (hu == 0.f && !debug_no_deposit)  // unoccluded: render.cuh:291-293
                    acc_add(acc, park[6 * kBlock], park[7 * kBlock], park[8 * kBlock]);
                // now the slot's path ray
                o = mk(park[0 * kBlock], park[1 * kBlock], park[2 * kBlock]);
                d = mk(park[3 * kBlock], park[4 * kBlock], park[5 * kBlock]);
                phase = PH_CLOSEST;
                inv = inv_dir(d);
                tmax = kFltMax;
                tri = -1;
                cur = 0;
                sp = 0;
            } else {
                // (tri, hu, hv, d) carry the hit to the ADV block; a path that missed, or has no bounce left (and is not
                // at bounce 0, where a hit light still emits: render.cuh:98-109), can only generate
                const int b = cold[0 * kBlock];
                phase = (SPLIT_GEN && (tri < 0 || (b >= ap_max_bounces && b > 0))) ? PH_GEN : PH_ADV;
            }
        }
#ifdef RT_TRACE_PROFILE
        pf_fin_cycles += __builtin_readcyclecounter() - pf_tf;
        pf_last_work = phase != PH_IDLE ? pf_tf - pf_t0 : pf_last_work;
#endif
    }
#ifdef RT_TRACE_PROFILE
    if (prof && lane_id() == 0) { atomicAdd(&prof[17], pf_fin_cycles); atomicAdd(&prof[18], pf_fin_lanes); atomicAdd(&prof[19], pf_fin_iters); }
    // the lane-idle tail: lane-cycles between each lane's last work and the wave's exit, and the longest of the 64 tails
    // (= from the first lane going idle for good to the exit)
    const unsigned long long pf_life = __builtin_readcyclecounter() - pf_t0;
    unsigned long long pf_idle = pf_life - pf_last_work, pf_idle_max = pf_idle;
    for (int off = 32; off > 0; off >>= 1) {
        pf_idle += __shfl_xor(pf_idle, off);
        const unsigned long long other = __shfl_xor(pf_idle_max, off);
        pf_idle_max = other > pf_idle_max ? other : pf_idle_max;
    }
    if (prof && lane_id() == 0)
        { pf[11] = pf_life; for (int k = 0; k < 16; k++) atomicAdd(&prof[k], pf[k]); atomicMax(&prof[13], pf[11]); atomicAdd(&prof[14], 1ull); atomicAdd(&prof[16], pf_gen_cycles);
          atomicAdd(&prof[20], pf_idle); atomicAdd(&prof[21], pf_idle_max);
          atomicAdd(&prof[22], pf_handovers); atomicAdd(&prof[23], pf_handover_blocks);
          atomicAdd(&prof[24], pf_rr_turns); atomicAdd(&prof[25], pf_rr_blocks);
          // per-wave record: where it ran and for how long
          unsigned long long *rec = prof + kProfHead + kProfRec * (size_t)((blockIdx.x * kBlock + threadIdx.x) >> 6);
          rec[0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
          rec[1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
          rec[2] = pf[11];
          rec[3] = pf[0] + pf[2] + pf[4];
          rec[4] = pf_idle;
          rec[5] = pf_idle_max; }
#endif
    if constexpr (BUILD::kBg && SPLIT_GEN) {
        unsigned long long bg = n_bg_lane;
        for (int off = 32; off > 0; off >>= 1) bg += __shfl_xor(bg, off);
        n_gen += bg;
        n_traced += bg;
    }
    unsigned long long v[C_COUNT] = {n_gen, n_shade, n_traced, n_shadow, n_emit, n_deposit, n_rr, 0ull};
    row_add(rows, v);
}
