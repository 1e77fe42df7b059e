// rtcuda_amd.hip -- HIP kernels and the C-ABI of the MI355X-native render path (gfx950 only).
// The root of the one translation unit.  Here: the constants, the device structures and wave helpers, RNG and pool initialisation,
// the table builders, gen_core / advance_core, the k_paths knobs, the post-process kernels and the C-ABI.  Included, in this order:
//   rt_walk.inc            box test, traversal stack, inner_step; reference_walk; VERIFY (ref_visible); leaf_hits, verify_closest
//   rt_stream_kernels.inc  k_trace (the pools of a round); the query prepasses; stream_walk, the persistent loop of every dense ray
//                          array, under k_query (queries and trace hooks), k_aov and k_motion; k_aov_resolve
//   rt_frame_kernels.inc   k_advance<SRC> and k_paths<BUILD>: templates over the source of camera rays and the build tag
//   rt_build_kernels.inc   device BVH: the leaf-order arrays, the refit (k_refit_*), the build (k_ploc_*)
//   rt_host_scene.inc      rt_scene and the one way a tree gets into it: build (host SAH, device PLOC), emit, adopt; the entry
//                          points on top of it (create, update, rebuild, the edits); what the ray entry points share
//   rt_host_render.inc     Context and the cached output buffers (and their release, rt_shutdown), kernel selection, one shard of a
//                          frame (render_shard_impl), queries and their host-pointer form (the trace hooks), ray tables, AOVs
//   rt_host_frame.inc      whole frames: shards side by side on host threads (run_shard_jobs: RT_SPLIT, rt_render_multi), their
//                          stats merged (rt_stats_merge.h), the post-process, finish_frame, rt_render and rt_render_multi
//   rt_denoise_kernels.inc the denoisers' kernels: one tap loop (dn_filter_pixel) and two pass bodies (dn_pass_direct, dn_pass_lds) under
//                          k_atrous* / k_atrous_var*; prepare, finish, k_dn_var_blur (arithmetic: rt_denoise.h, shared with the CPU twin)
//   rt_host_denoise.inc    rt_denoise_fixed, rt_denoise_dual_fixed and rt_denoise_variance_fixed: one set of checks (dn_check), one pass
//                          launcher, one run (dn_run); rt_upsample_fixed and rt_upsample_rgb behind the same checks (upsample_impl)
//   rt_temporal_kernels.inc k_temporal_accumulate_moments, k_temporal_accumulate: one pixel body with its features and without (arithmetic: rt_temporal.h, shared with k_motion and the CPU twins)
//   rt_upsample_kernels.inc k_upsample<F, kRgb>: AOV-guided upsampling, a tile of full pixels from its low-resolution footprint in LDS (arithmetic: rt_upsample.h, shared with the CPU twin)
//   rt_host_temporal.inc   rt_temporal_accumulate_moments_fixed, and rt_temporal_accumulate_fixed as that with the features off: the checks and the launch
// The C-ABI below them only checks arguments and forwards, and calls none of its own entry points.  Two bodies stay in it:
// rt_camera_make (host arithmetic, nothing shared) and rt_xorwow_states (a test hook around k_rng_init / k_test_draw).
//
// The hot path of lashhw/rtcuda (render.cuh:61-457) re-designed for CDNA4:
//
//   * Path state lives in structure-of-arrays pools indexed by path SLOT (the reference keeps
//     28-byte AoS rays and pointer-chasing payloads: render.cuh:5-23).
//   * Slot s owns RNG stream s and serves exactly the camera rays c with c % W == s
//     (W = 1048576): in the reference every slot regenerates in lockstep (bounces is incremented
//     unconditionally, render.cuh:126, and reset only by gen, :268), so the rank of a slot in the
//     compacted gen queue is always the slot id itself.  A slot's history therefore never depends
//     on any other slot, and a slot may start its next camera ray as soon as its current path can
//     do nothing more.  That removes the reference's idle iterations (the
//     active fraction decays 100 % -> 2 % inside every 11-iteration generation) without changing
//     one random number, and makes the image invariant under any partition of the slots -- which
//     is how the work is sharded over GPUs.
//   * One global condition remains -- the host loop stops at the first iteration in which nothing
//     shades (render.cuh:436) -- and it can only bite in the final generation, which is therefore
//     run in lockstep (one init() per slot per round; the stop rule is evaluated on the device).
//
// Kernels:
//   k_paths      everything before the final generation, ONE persistent launch per frame.  A lane
//                owns a slot (then its next one); init+mat, gen, the shadow ray and the path ray are
//                PHASES of the lane; the wave issues, per iteration, the one block most of its lanes
//                wait for.  Rays, hit records and queues never leave registers / LDS; a camera
//                ray's contributions are summed in LDS and reach the framebuffer as one atomic triple;
//                traversal is speculative (a leaf reached inside a node block is set aside).
//   k_advance    init() + mat() + gen() for all slots of a round (render.cuh:84-275), state in the
//   k_trace      SoA pools; ch() + ah() of a round (render.cuh:278-328) with persistent waves, ballot +
//                mbcnt compaction into a per-wave LDS queue instead of flag arrays + CUB select
//                (render.cuh:348-364), while-while traversal, LDS stack.  Used for the lockstep final
//                generation and (RT_PERSISTENT=0) for whole frames: it walks pools and nothing else.
//   advance_core / inner_step / tri_intersect / box_hit are the shared device functions: one copy of
//   the estimator and of the traversal for both pipelines.
//   k_query      the caller's rays from device buffers (rt_query_*_device, and rt_trace_* with host pointers), and the first-hit
//   k_aov        feature buffers: two pairs of ends on one persistent loop over a stream of ray ids (stream_walk,
//                rt_stream_kernels.inc), the walker of every dense ray array.
//   * BVH: 64-byte node records with full-precision padded boxes -- a 4-wide node as two consecutive
//     records (default), or 2-wide nodes of one record (RT_BVH_WIDE=0) --
//     and 48-byte {p0,e1,e2,n} triangle records in leaf order (rt_bvh.h: SAH sweep + insertion-based
//     optimisation + collapse to 4-wide).
//   * Two results that depend, in the reference, on the shape of its own tree are defined by the triangle
//     list alone here: an accepted hit is never culled (conservative box test), and hits at exactly equal
//     t go to the larger caller index (closest_hit_wins).  Traversal ORDER therefore never matters.
//   * There are no host read-backs inside a frame (the reference does four blocking 4-byte read-backs per
//     iteration: render.cuh:433-434,444-445): the persistent kernel needs none, and the lockstep rounds of the
//     final generation carry their stop rule on the device (k_advance: `lock_shades`).
//
// No MFMA anywhere: there is no dense contraction on this path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <string>
#include <vector>

#include "../../include/rtcuda_amd.h"
#include "rt_background.h"
#include "rt_bvh.h"
#include "rt_denoise.h"
#include "rt_device.h"
#include "rt_launch_plan.h"
#include "rt_ploc.h"
#include "rt_ref_tree.h"
#include "rt_slot_chunks.h"
#include "rt_stats_merge.h"
#include "rt_temporal.h"
#include "rt_upsample.h"

using namespace rt;

// ============================================================================ error handling
namespace {
thread_local std::string g_last_error;
std::string g_peer_log;  // rt_render_multi: what became of peer access, pair by pair (rt_peer_access_log)
int fail(const std::string &msg) {
    g_last_error = msg;
    return 1;
}
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return fail(std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ ":" + \
                        std::to_string(__LINE__) + ")");                                       \
    } while (0)

using rtbvh::knob;  // (experiment knobs are read only under RTCUDA_EXPERIMENTAL=1: rt_bvh.h)

constexpr int kW = RT_NUM_WORKING_PATHS;
constexpr uint32_t kFlagFixedFb = 0x200u;  // internal: d_sum points to int64 fixed-point sums
constexpr int kBlock = 256;       // 4 waves per workgroup
static_assert(rtplan::kBlock == kBlock && rtplan::kSlots == kW, "rt_launch_plan.h plans for this workgroup and this pool");
constexpr int kLdsStack = 16;          // traversal stack entries kept in LDS per lane (k_trace)
constexpr int kPathsLdsStack = 10;     // ... by k_paths: 10 + 1 + 26 rows = 37 KB per workgroup, four workgroups per CU; with 10 the
                                       // step without overflow handling (inner_step<WIDE, SHALLOW>) serves 95 % of the node steps
constexpr int kOverStride = 1 << 20;   // lanes of the overflow stack (>= lanes of the largest grid that traverses)
constexpr int kMaxStackBound = 160;    // deepest traversal stack a scene may need (3 per level + 1)
constexpr int kLockChunk = 16;         // lockstep rounds of the final generation enqueued between two looks at the stop rule's counters
}  // namespace

// ============================================================================ device structures
struct DScene {
    const float4 *nodes;   // 64-byte records (4 x float4): two per 4-wide node, one per 2-wide node (rt_bvh.h)
    const float4 *tris;    // 3 x float4 per triangle, leaf order
    const int2 *tri_info;  // leaf order: {material index, light index or -1}
    const float4 *tri_shade;  // leaf order: what mat() needs of a hit triangle besides the point -- the flipped unit
                              // normal -normalize(n) (render.cuh:153) and the packed ids (material | light + 1 << 16)
    const int *order;         // leaf order -> the caller's triangle index (closest-hit tie rule, test output)
    const Material *mats;
    const Light *lights;
    int num_lights;
    int num_mats;
    // shading tables in one block of dwords: [materials 5/each][lights 8/each][light triangle
    // records 12/each][per-light precomputed {1/area, unit normal} 4/each]
    const float *tables;
    int tab_dwords;
    // RT_FLAG_REFERENCE_WALK only (null otherwise; no other kernel reads them): the reference's own binary tree
    // (rt_ref_tree.h) as 32-byte nodes {bounds[6], count, link} = 2 x float4, and its primitive order mapped to this
    // scene's leaf-order triangle indices
    const float4 *ref_nodes;
    const int *ref_prims;
    int ref_n_prims;
    // default kernels (VERIFY; null with RT_FLAG_WATERTIGHT): leaf-order triangle index -> the node of its leaf in the
    // reference's tree, node -> parent node (root: -1), and whether that tree's root is a leaf (ref_visible)
    const int *ref_leaf_of;
    const int *ref_parent;
    int ref_root_leaf;
};
__device__ __host__ inline int tab_off_lights(int n_mats) { return 5 * n_mats; }
__device__ __host__ inline int tab_off_ltri(int n_mats, int n_lights) { return 5 * n_mats + 8 * n_lights; }
__device__ __host__ inline int tab_off_lpre(int n_mats, int n_lights) { return 5 * n_mats + 20 * n_lights; }
constexpr int kTabPerMat = 5, kTabPerLight = 8 + 12 + 4;  // dwords of the block per material and per light
inline int tab_dwords(int n_mats, int n_lights) { return kTabPerMat * n_mats + kTabPerLight * n_lights; }

// Structure-of-arrays path state for the slots of one shard (n slots each)
// Structure-of-arrays path state for the slots of one shard: A_COUNT arrays of n dwords in ONE
// allocation, array k at base + k * n.  A kernel therefore carries one base pointer (2 SGPRs)
// instead of 36 array pointers -- the persistent kernel otherwise spends VGPRs and scratch on
// addresses.
//   ox..dz            current path ray
//   hit_info          -1 = miss, else material | (light index + 1) << 16
//   hpx..hpz          Triangle::p(u, v) of the last closest hit              (render.cuh:152)
//   hnx..hnz          -d_triangle->n.unit_vector()                           (render.cuh:153)
//   br, bg, bb        beta
//   bounces           as PathRayPayload::bounces; kDone / kParked are sentinels
//   pixel, gen        pixel of the current camera ray; index of the slot's NEXT generation
//   rd, r0..r4        XORWOW state
//   sox..slb, starget shadow ray of the slot for this round (stmax < 0: none) + radiance + excluded triangle
enum { A_OX, A_OY, A_OZ, A_DX, A_DY, A_DZ, A_HPX, A_HPY, A_HPZ, A_HNX, A_HNY, A_HNZ, A_BR, A_BG, A_BB, A_SOX, A_SOY, A_SOZ, A_SDX, A_SDY, A_SDZ, A_STMAX, A_SLR, A_SLG, A_SLB, A_HIT_INFO, A_BOUNCES, A_PIXEL, A_GEN, A_STARGET, A_RD, A_R0, A_R1, A_R2, A_R3, A_R4, A_COUNT };
struct DPools {
    float *base;
    int n;
    __device__ __forceinline__ float &ox(int i) const { return base[(unsigned)(A_OX * n + i)]; }
    __device__ __forceinline__ float &oy(int i) const { return base[(unsigned)(A_OY * n + i)]; }
    __device__ __forceinline__ float &oz(int i) const { return base[(unsigned)(A_OZ * n + i)]; }
    __device__ __forceinline__ float &dx(int i) const { return base[(unsigned)(A_DX * n + i)]; }
    __device__ __forceinline__ float &dy(int i) const { return base[(unsigned)(A_DY * n + i)]; }
    __device__ __forceinline__ float &dz(int i) const { return base[(unsigned)(A_DZ * n + i)]; }
    __device__ __forceinline__ float &hpx(int i) const { return base[(unsigned)(A_HPX * n + i)]; }
    __device__ __forceinline__ float &hpy(int i) const { return base[(unsigned)(A_HPY * n + i)]; }
    __device__ __forceinline__ float &hpz(int i) const { return base[(unsigned)(A_HPZ * n + i)]; }
    __device__ __forceinline__ float &hnx(int i) const { return base[(unsigned)(A_HNX * n + i)]; }
    __device__ __forceinline__ float &hny(int i) const { return base[(unsigned)(A_HNY * n + i)]; }
    __device__ __forceinline__ float &hnz(int i) const { return base[(unsigned)(A_HNZ * n + i)]; }
    __device__ __forceinline__ float &br(int i) const { return base[(unsigned)(A_BR * n + i)]; }
    __device__ __forceinline__ float &bg(int i) const { return base[(unsigned)(A_BG * n + i)]; }
    __device__ __forceinline__ float &bb(int i) const { return base[(unsigned)(A_BB * n + i)]; }
    __device__ __forceinline__ float &sox(int i) const { return base[(unsigned)(A_SOX * n + i)]; }
    __device__ __forceinline__ float &soy(int i) const { return base[(unsigned)(A_SOY * n + i)]; }
    __device__ __forceinline__ float &soz(int i) const { return base[(unsigned)(A_SOZ * n + i)]; }
    __device__ __forceinline__ float &sdx(int i) const { return base[(unsigned)(A_SDX * n + i)]; }
    __device__ __forceinline__ float &sdy(int i) const { return base[(unsigned)(A_SDY * n + i)]; }
    __device__ __forceinline__ float &sdz(int i) const { return base[(unsigned)(A_SDZ * n + i)]; }
    __device__ __forceinline__ float &stmax(int i) const { return base[(unsigned)(A_STMAX * n + i)]; }
    __device__ __forceinline__ float &slr(int i) const { return base[(unsigned)(A_SLR * n + i)]; }
    __device__ __forceinline__ float &slg(int i) const { return base[(unsigned)(A_SLG * n + i)]; }
    __device__ __forceinline__ float &slb(int i) const { return base[(unsigned)(A_SLB * n + i)]; }
    __device__ __forceinline__ int &hit_info(int i) const { return ((int *)base)[(unsigned)(A_HIT_INFO * n + i)]; }
    __device__ __forceinline__ int &bounces(int i) const { return ((int *)base)[(unsigned)(A_BOUNCES * n + i)]; }
    __device__ __forceinline__ int &pixel(int i) const { return ((int *)base)[(unsigned)(A_PIXEL * n + i)]; }
    __device__ __forceinline__ int &gen(int i) const { return ((int *)base)[(unsigned)(A_GEN * n + i)]; }
    __device__ __forceinline__ int &starget(int i) const { return ((int *)base)[(unsigned)(A_STARGET * n + i)]; }
    __device__ __forceinline__ uint32_t &rd(int i) const { return ((uint32_t *)base)[(unsigned)(A_RD * n + i)]; }
    __device__ __forceinline__ uint32_t &r0(int i) const { return ((uint32_t *)base)[(unsigned)(A_R0 * n + i)]; }
    __device__ __forceinline__ uint32_t &r1(int i) const { return ((uint32_t *)base)[(unsigned)(A_R1 * n + i)]; }
    __device__ __forceinline__ uint32_t &r2(int i) const { return ((uint32_t *)base)[(unsigned)(A_R2 * n + i)]; }
    __device__ __forceinline__ uint32_t &r3(int i) const { return ((uint32_t *)base)[(unsigned)(A_R3 * n + i)]; }
    __device__ __forceinline__ uint32_t &r4(int i) const { return ((uint32_t *)base)[(unsigned)(A_R4 * n + i)]; }
    // host-side address of array k
    float *array(int k) const { return base + (size_t)k * n; }
};

// Global words that need atomics / host polling.  Event counters are NOT here: they live in
// per-wave rows (DWaveRow) that only their owner wave updates, with plain loads and stores --
// 16384 waves hitting eight shared words with atomics every round was the single largest cost of
// the first version of k_advance.
struct DCounters {
    int last_live_round;         // highest batch-closing round in which some slot still traced a ray
    unsigned int unused0;        // (round 3: the lockstep rounds' shade count, now per round in Context::d_lock)
    unsigned int pad2[2];
    // VERIFY builds (rare events, global atomics): [0] accepted hits whose OWN box fails the reference's slab test,
    // [1] ... whose reference leaf box (or, for a ray with a -0.0 direction component, some ancestor box) fails it too =
    // hits the reference's walk loses, [2] closest hits with an exact tie at the final distance, [3] literal re-traces
    unsigned long long vstat[4];
};
enum { V_OWN_FAIL = 0, V_LOST = 1, V_TIE = 2, V_LITERAL = 3 };
enum { C_CAMERA = 0, C_SHADE, C_CLOSEST, C_ANY, C_EMIT, C_SHADOW_ADD, C_RR, C_UNUSED, C_COUNT };
struct DWaveRow {
    unsigned long long c[C_COUNT];  // one 64-byte line per wave
};

constexpr int kDone = -0x7fffffff;    // slot has no camera ray left
constexpr int kParked = -0x7ffffffe;  // slot waits for the lockstep rounds of the final generation
constexpr int kChunkFresh = 0x7ffffffe;  // k_paths<PathsChunked>, in the lane's LDS copy of `bounces` only: the lane has taken the slot and made no ray of it yet

// ============================================================================ wave helpers
__device__ __forceinline__ unsigned lane_id() {
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}
// number of set bits of `mask` below this lane
__device__ __forceinline__ unsigned prefix_popc(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}
// Wave votes straight from the condition's compare (HIP's wave_ballot(int) first materialises the predicate as 0 / 1 in
// a VGPR and compares that with zero again: two more VALU instructions per vote, a dozen votes per scheduling decision).
__device__ __forceinline__ unsigned long long wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ int wave_count(bool p) { return (int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(p)); }
__device__ __forceinline__ unsigned wave_index() { return (blockIdx.x * blockDim.x + threadIdx.x) >> 6; }
// lanes 0..7 of the wave add v[lane] to the wave's own row: one 64-byte load + one 64-byte store
__device__ __forceinline__ void row_add(DWaveRow *rows, const unsigned long long (&v)[C_COUNT]) {
    unsigned l = lane_id();
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < C_COUNT; k++) mine = (l == (unsigned)k) ? v[k] : mine;
    // no-return atomics on a line only this wave touches: fire-and-forget, no load round trip
    if (l < C_COUNT && mine != 0) atomicAdd(&rows[wave_index()].c[l], mine);
}

// ============================================================================ RNG init kernel
// curand_init(seed, slot, 0) (render.cuh:68-73): the seed-scrambled state advanced by slot * 2^67
// draws.  The 2^67-draw jump is the GF(2)-linear map J on the 160 state bits; jump_pow holds
// J^(2^k), k = 0..19, as 160 rows x 5 words each (row b = image of basis bit b), so J^slot is at
// most 20 mat-vecs selected by the bits of the slot id.
__global__ void k_rng_init(DPools p, int n, int slot_lo, Rng seed_state, const uint32_t *__restrict__ jump_pow) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t slot = (uint32_t)(slot_lo + i);
    uint32_t v[5] = {seed_state.v0, seed_state.v1, seed_state.v2, seed_state.v3, seed_state.v4};
    for (int k = 0; k < 20; k++) {
        if (!((slot >> k) & 1u)) continue;
        const uint32_t *m = jump_pow + (size_t)k * 160 * 5;
        uint32_t r[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < 5; w++) {
            uint32_t bits = v[w];
            for (int b = 0; b < 32; b++) {
                uint32_t sel = 0u - ((bits >> b) & 1u);
                const uint32_t *row = m + (w * 32 + b) * 5;
                r[0] ^= row[0] & sel;
                r[1] ^= row[1] & sel;
                r[2] ^= row[2] & sel;
                r[3] ^= row[3] & sel;
                r[4] ^= row[4] & sel;
            }
        }
#pragma unroll
        for (int w = 0; w < 5; w++) v[w] = r[w];
    }
    p.rd(i) = seed_state.d;
    p.r0(i) = v[0];
    p.r1(i) = v[1];
    p.r2(i) = v[2];
    p.r3(i) = v[3];
    p.r4(i) = v[4];
}

// init_path_ray_payload (render.cuh:75-82): every slot starts "finished" so the first round
// routes it to gen.  (The reference stores INT_MAX and relies on INT_MAX+1 wrapping; any value
// >= max_bounces has the same effect on the first init().)
__global__ void k_pool_init(DPools p, int n, int max_bounces) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    p.hit_info(i) = -1;
    p.bounces(i) = max_bounces;
    p.gen(i) = 0;
    p.pixel(i) = 0;
}

// ============================================================================ k_advance
struct AdvanceParams {
    int n;        // slots in this shard
    int slot_lo;  // global id of local slot 0
    int width, height, spp, max_bounces;
    long long cam_end;  // width*height*spp
    int round;
    int batch_mask;      // rounds with (round & batch_mask) == batch_mask close a host-polled batch
    int last_gen;        // index of the final camera-ray generation
    int lockstep;        // != 0: final generation, one init() per slot per round (literal reference schedule); 1 + the index of
                         // the lockstep round (0 = the round that generates)
    int fb_fixed;        // framebuffer holds 64-bit fixed-point sums (see deposit())
    int w_over_spp;      // W / spp when spp divides W (then pixel = gen * w_over_spp + slot / spp: no 64-bit divide), else 0
    int dpx, dpy;        // w_over_spp = dpy * width + dpx: how a slot's pixel moves per generation; dpy < 0: not usable
    // RT_FLAG_RNG_PER_SAMPLE: every camera ray starts its own stream, keyed by its GLOBAL id = local id * key_mul + key_add
    // (rank `key_add` of `key_mul` renders the frame at spp / key_mul with the full slot pool); no slot parks
    int per_sample, key_mul, key_add;
    uint32_t seed_lo, seed_hi;
    // The pixels [bg_x0, bg_x0 + bg_w) x [bg_y0, bg_y0 + bg_h) outside which no camera ray of the frame can hit the scene
    // (rt_background.h; the whole frame where nothing is known, bg_w = 0 where nothing can be hit).  Read by k_paths<PathsBg> /
    // k_paths<PathsChunkedBg> only, which a frame runs if the rectangle is smaller than it: they make no ray for a pixel outside it
    // (gen_background).
    int bg_x0, bg_y0, bg_w, bg_h;
};

constexpr int kLdsTable = 64;                   // materials / lights staged in LDS per workgroup
constexpr int kTabDwordsMax = kLdsTable * (kTabPerMat + kTabPerLight);  // tab_dwords(kLdsTable, kLdsTable)

// Per-light values that depend on the light triangle only, computed once per scene on the device
// with the same operations mat() would redo per shade: 1 / Triangle::area() (triangle.cuh:79,84-86)
// and d_triangle->n.unit_vector() (light.cuh:46).
// Per-triangle shading record, computed once per scene with the operations mat() would redo at every shade
// (isect_unit_n = -d_triangle->n.unit_vector(), render.cuh:153; vec3.cuh:131-134).
__global__ void k_build_tri_shade(const float4 *__restrict__ tris, const int2 *__restrict__ tri_info, int n,
                                  float4 *__restrict__ out) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    Tri tr = load_tri(tris, k);
    V3 un = neg(unit(tr.n));
    int2 ml = tri_info[k];
    out[k] = make_float4(un.x, un.y, un.z, __int_as_float((ml.x & 0xffff) | ((ml.y + 1) << 16)));
}

__global__ void k_build_tables(const Material *mats, int n_mats, const Light *lights, int n_lights,
                               const float4 *tris, float *tab) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_mats) {
        const float *src = (const float *)&mats[t];
        for (int k = 0; k < 5; k++) tab[5 * t + k] = src[k];
    }
    if (t < n_lights) {
        const float *src = (const float *)&lights[t];
        float *dl = tab + tab_off_lights(n_mats) + 8 * t;
        for (int k = 0; k < 8; k++) dl[k] = src[k];
        float *dt = tab + tab_off_ltri(n_mats, n_lights) + 12 * t;
        float *dp = tab + tab_off_lpre(n_mats, n_lights) + 4 * t;
        Light l = lights[t];
        if (l.type == 1) {
            Tri lt = load_tri(tris, l.tri);
            const float *q = (const float *)(tris + 3 * (size_t)l.tri);
            for (int k = 0; k < 12; k++) dt[k] = q[k];
            V3 un = unit(lt.n);
            dp[0] = 1.f / tri_area(lt);
            dp[1] = un.x;
            dp[2] = un.y;
            dp[3] = un.z;
        } else {
            for (int k = 0; k < 12; k++) dt[k] = 0.f;
            dp[0] = dp[1] = dp[2] = dp[3] = 0.f;
        }
    }
}

__device__ __forceinline__ Material tab_material(const float *tab, int i) {
    const float *q = tab + 5 * i;
    Material m;
    m.ax = q[0];
    m.ay = q[1];
    m.az = q[2];
    m.ior = q[3];
    m.type = __float_as_int(q[4]);
    return m;
}
__device__ __forceinline__ Light tab_light(const float *tab, int n_mats, int i) {
    const float *q = tab + tab_off_lights(n_mats) + 8 * i;
    Light l;
    l.type = __float_as_int(q[0]);
    l.px = q[1];
    l.py = q[2];
    l.pz = q[3];
    l.tri = __float_as_int(q[4]);
    l.lx = q[5];
    l.ly = q[6];
    l.lz = q[7];
    return l;
}

// ---------------------------------------------------------------------------------------------
// advance_core: init() + mat() + gen() for ONE slot (render.cuh:84-275), on register state.
// Shared by k_advance (state loaded from / stored to the pools) and k_paths (state lives in
// registers for the whole frame).
// Framebuffer deposit.  Default: three float atomics, as the reference's Vec3::atomic_add
// (vec3.cuh:149-153) -- the summation order, and with it the last bits of a pixel, vary from run to
// run.  Fixed mode (RT_FLAG_DETERMINISTIC / rt_render_shard_fixed): the buffer holds 64-bit
// fixed-point sums (scale 2^30); integer adds commute, so the image is bit-reproducible and the sum of
// the shards of a multi-GPU render is EXACTLY the single-GPU sum.  Non-finite contributions (none
// occur in any test scene) are dropped and magnitudes are clamped to 2^31 in that mode.
constexpr float kFixedScale = 1073741824.f;  // 2^30
__device__ __forceinline__ long long to_fixed(float x) {
    if (!(fabsf(x) <= 2147483648.f)) x = (x == x) ? copysignf(2147483648.f, x) : 0.f;
    return __float2ll_rn(x * kFixedScale);
}
__device__ __forceinline__ void deposit(float *__restrict__ fb, int fixed, int pixel, float r, float g, float b) {
    const unsigned k = (unsigned)(3 * pixel);
    if (fixed) {
        unsigned long long *f = (unsigned long long *)fb;
        atomicAdd(&f[k + 0], (unsigned long long)to_fixed(r));
        atomicAdd(&f[k + 1], (unsigned long long)to_fixed(g));
        atomicAdd(&f[k + 2], (unsigned long long)to_fixed(b));
    } else {
        atomicAdd(&fb[k + 0], r);
        atomicAdd(&fb[k + 1], g);
        atomicAdd(&fb[k + 2], b);
    }
}

// Per-lane sample accumulator of k_paths (3 floats in the lane's LDS column, element k at acc[k * kBlock]): the
// contributions of ONE camera ray -- bounce-0 emission, then the unoccluded shadow rays in path order -- are summed here
// and reach the framebuffer as one atomic triple when the slot starts its next camera ray (the reference issues one
// atomic triple per contribution, in an order that differs from run to run: vec3.cuh:149-153).  A float atomic is a
// fabric transaction whose acknowledgement a wave's later loads queue behind (vmcnt is in order), so the frame has
// 0.5 G of them instead of 1.0 G and they sit in the GEN block instead of the traversal loop: +4 %.
__device__ __forceinline__ void acc_add(float *acc, float r, float g, float b) {
    acc[0 * kBlock] += r;
    acc[1 * kBlock] += g;
    acc[2 * kBlock] += b;
}
__device__ __forceinline__ void acc_flush(float *acc, float *__restrict__ fb, int fixed, int pixel) {
    const float r = acc[0 * kBlock], g = acc[1 * kBlock], b = acc[2 * kBlock];
    if (r != 0.f || g != 0.f || b != 0.f) {  // (a NaN contribution compares unequal to 0: it is deposited)
        deposit(fb, fixed, pixel, r, g, b);
        acc[0 * kBlock] = 0.f;
        acc[1 * kBlock] = 0.f;
        acc[2 * kBlock] = 0.f;
    }
}

struct SlotState {
    int bounces, hit_info, pixel, gen;
    Rng rs;
    V3 beta, wo, isect_p, isect_n;
};
struct AdvanceOut {
    bool did_gen, did_shade, has_shadow, did_emit, new_ray;
    bool wants_gen;             // advance_core<DEFER_GEN = true> only: the slot's next step is gen()
    int rr_draws;
    int bg_skipped;             // advance_core of k_paths' 2-waves-per-SIMD camera builds only: background camera rays gen() passed over
    V3 ray_o, ray_d;            // next path ray (valid when new_ray)
    V3 s_o, s_d, s_L;           // shadow ray + radiance to deposit if unoccluded (valid when has_shadow)
    float s_tmax;
    int s_target;
};

// The camera rays of a ray-table frame (rt_render_rays_device / rt_render_rays_fixed_device): row c is camera ray c.
struct RayTable {
    const float *o3, *d3;  // origins and directions, AoS triples
    const int *pixel;      // the pixel a ray deposits into; null: c / AdvanceParams::spp
};
// The camera rays of a KEYED ray-table frame (rt_render_rays_keyed_device / rt_render_rays_keyed_fixed_device): row c is the
// camera ray with the 64-bit key K = key_first + c * key_stride, and its stream is rng_sample_stream(seed, K) -- camera ray
// G = K of an RT_FLAG_RNG_PER_SAMPLE frame.  Without a pixel array the ray lands on pixel K / rays_per_pixel (by the key, not
// by the row), which the host hands over as pix_first + (rem_first + c * key_stride) / rays_per_pixel with
// pix_first = key_first / rays_per_pixel and rem_first = key_first % rays_per_pixel: the same quotient, and its dividend
// fits 32 bits for every chunk of a stride-1 table (then the divide is the 32-bit one).
// Travels in k_paths<PathsKeyed>'s uniforms where the camera builds keep the Camera: no larger than it.
struct KeyedRayTable {
    const float *o3, *d3;  // origins and directions, AoS triples
    const int *pixel;      // the pixel a ray deposits into; null: K / rays_per_pixel
    unsigned long long key_first;
    uint32_t key_stride, rays_per_pixel;
    int pix_first;
    uint32_t rem_first;
};
static_assert(sizeof(KeyedRayTable) <= sizeof(Camera), "k_paths' dynamic LDS is sized for a Camera in the uniforms");
// The camera rays of a COUNTED frame (rt_render_counts_fixed): pixel p renders the samples first[p] .. first[p] + count[p] - 1
// of the RT_FLAG_RNG_PER_SAMPLE frame with `stride` samples per pixel.  Camera ray c of the call, 0 <= c < sum of the counts,
// belongs to the pixel p with offset[p] <= c < offset[p + 1] (offset: the exclusive prefix sum of the counts, n_pixels + 1
// words, made by the prepass k_counts_*), is that pixel's sample k = first[p] + c - offset[p], and has the 64-bit key
// p * stride + k: the stream, the jitter and the ray of camera ray G = key of the whole frame.
// Larger than a Camera: k_paths<PathsCounts>' launch sizes the dynamic LDS for it (FrameRun::run_persistent).
struct CountsCamera {
    Camera cam;
    const uint32_t *offset;
    const int32_t *first;  // null: all 0
    uint32_t stride;
    int n_pixels;
};
__device__ __forceinline__ void camera_get_ray(const CountsCamera &s, float x, float y, V3 &o, V3 &d) { camera_get_ray(s.cam, x, y, o, d); }
// the largest p in [lo, hi] with offset[p] <= c, given offset[lo] <= c: the pixel of camera ray c if that pixel is at most hi.
// Runs of pixels without samples repeat an offset, and the LAST pixel of such a run is the one that holds the ray.
__device__ __forceinline__ int counts_find(const uint32_t *__restrict__ offset, int lo, int hi, unsigned c) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);  // (lo < mid <= hi)
        const bool below = offset[mid] <= c;
        lo = below ? mid : lo;
        hi = below ? hi : mid - 1;
    }
    return lo;
}
// counts_find for a whole wave that looks for ONE c (lo, hi and c are wave-uniform, every lane of the wave is here): the 64 lanes
// probe 64 evenly spaced pixels of the range at once -- the offsets do not decrease, so the lanes that find offset <= c are the
// first ones, and the last of them names the next range -- and 2^21 pixels take 4 rounds of one load where a lane alone makes 21
// loads one after the other.
__device__ __forceinline__ int counts_find_wave(const uint32_t *__restrict__ offset, int lo, int hi, unsigned c) {
    const int lane = (int)lane_id();
    while (true) {
        const int step = (hi - lo) / 64 + 1;  // (the 64 probes lo + j * step cover [lo, hi]; step = 1: every pixel of it)
        const int probe = min(lo + lane * step, hi);  // (lo + 63 * step <= lo + 63 * (hi - lo) / 64 + 63: no overflow, hi < 2^30)
        const unsigned long long below = wave_ballot(offset[probe] <= c);  // (lane 0: offset[lo] <= c)
        const int j = (int)__popcll(below) - 1;
        const int at = min(lo + j * step, hi);
        if (step == 1) return at;
        hi = min(at + step - 1, hi);
        lo = at;
    }
}
// camera ray c of a counted frame, its pixel known to lie in [lo, hi]: the pixel, its coordinates and the ray's key
__device__ __forceinline__ void counts_locate(const CountsCamera &s, unsigned c, int lo, int hi, int width, int &pixel, int &px, int &py,
                                              unsigned long long &key) {
    const uint32_t *offset = s.offset;
    const int32_t *first = s.first;
    pixel = counts_find(offset, lo, hi, c);
    const unsigned k = (first ? (unsigned)first[pixel] : 0u) + (c - offset[pixel]);  // (below stride: the prepass has checked)
    key = (unsigned long long)(unsigned)pixel * s.stride + k;
    py = (int)((unsigned)pixel / (unsigned)width);
    px = pixel - py * width;
}
#ifndef RT_RAYS_NONTEMPORAL
#define RT_RAYS_NONTEMPORAL 1
#endif
template <class T>
__device__ __forceinline__ T table_load(const T *q) {
    return RT_RAYS_NONTEMPORAL ? __builtin_nontemporal_load(q) : *q;
}

// gen() (render.cuh:250-275) for one slot.  Camera ray id = generation * W + slot (see file header).  Leaves
// st.bounces = kDone (no camera ray left) / kParked (the final generation runs in lockstep) or a new path.
// `pxy` (optional): the slot's previous pixel as (x | y << 16), or -1.  A slot's pixel index grows by W / spp per
// generation, so with it the pixel coordinates follow by an add and a carry instead of two integer divisions.
// NEVER_LOCKSTEP: the caller (k_paths) only ever runs with ap.lockstep == 0 -- known at compile time there, a value read
// from LDS (and so a divergent branch with its merges, as far as the compiler can tell) otherwise.
// `cid_given` >= 0 (per-sample streams on the persistent kernel only): the camera ray is not the slot's next one but the one
// the wave drew from the frame's counter -- with a stream of its own per camera ray, any lane can take any camera ray.
// SRC: where camera ray `cid` comes from -- Camera: gen()'s pinhole; RayTable: the caller's table (rt_render_rays_*).  A
// property of the kernel build (a type, so a compile-time choice): the camera builds carry nothing of the table.
// The pieces of gen()'s pinhole, in the order gen_core runs them (k_paths' GEN block runs them itself, as a wave-level loop
// that passes over background pixels).
// gen_begin: the end tests, then the slot's generation counter moves on.  false: no ray (st.bounces = kDone / kParked).
template <bool NEVER_LOCKSTEP>
__device__ __forceinline__ bool gen_begin(const AdvanceParams &ap, int slot_global, SlotState &st, long long cid_given, long long &cid) {
    const bool lockstep = NEVER_LOCKSTEP ? false : (ap.lockstep != 0);
    cid = cid_given >= 0 ? cid_given : (long long)st.gen * kW + slot_global;
    if (cid >= ap.cam_end) {
        st.bounces = kDone;
        return false;
    }
    if (!lockstep && st.gen == ap.last_gen) {
        st.bounces = kParked;
        return false;
    }
    st.gen = st.gen + 1;
    return true;
}
// gen_pixel: the pixel of camera ray `cid` (st.gen already counts it) into st.pixel and (px, py); *pxy follows.
__device__ __forceinline__ void gen_pixel(const AdvanceParams &ap, int slot_global, SlotState &st, int *pxy, long long cid_given,
                                          long long cid, int &px, int &py) {
    // pixel = camera_ray_id / spp (render.cuh:254-256).  cid = gen * W + slot, so when spp divides W the quotient
    // splits exactly into two 32-bit terms; the general case keeps the 64-bit division.
    if (cid_given >= 0) {
        st.pixel = (int)((unsigned)cid / (unsigned)ap.spp);  // (camera-ray ids stay below 2^31: rt_render_shard checks)
        py = (int)((unsigned)st.pixel / (unsigned)ap.width);
        px = st.pixel - py * ap.width;
    } else if (pxy && ap.dpy >= 0 && *pxy >= 0) {
        px = (*pxy & 0xffff) + ap.dpx;
        py = (*pxy >> 16) + ap.dpy;
        if (px >= ap.width) {
            px -= ap.width;
            py++;
        }
        st.pixel = py * ap.width + px;
    } else {
        if (ap.w_over_spp) st.pixel = (st.gen - 1) * ap.w_over_spp + (int)((unsigned)slot_global / (unsigned)ap.spp);  // (gen already counts this ray)
        else st.pixel = (int)(cid / ap.spp);
        py = (int)((unsigned)st.pixel / (unsigned)ap.width);  // (both non-negative: the unsigned divide is the cheaper one)
        px = st.pixel - py * ap.width;
    }
    if (pxy) *pxy = px | (py << 16);
}
// gen_background (k_paths' camera builds): no ray through this pixel can hit the scene (AdvanceParams::bg_*, rt_background.h).
// Such a camera ray is counted and its two jitter draws are made -- the slot's stream stays where the reference's is -- but
// no ray is made or walked: it would miss, deposit nothing and use no further draw.
__device__ __forceinline__ bool gen_background(const AdvanceParams &ap, int px, int py) {
    return (unsigned)(px - ap.bg_x0) >= (unsigned)ap.bg_w || (unsigned)(py - ap.bg_y0) >= (unsigned)ap.bg_h;
}
// gen_new_path: what every gen() that has made a ray leaves: the slot starts a new path.
__device__ __forceinline__ void gen_new_path(SlotState &st, AdvanceOut &out) {
    out.new_ray = true;
    st.bounces = 0;
    st.beta = mk(1.f, 1.f, 1.f);
    out.did_gen = true;
}
// gen_table_ray: row c of a ray table (RayTable, KeyedRayTable) as the new path ray.  The lanes of a wave serve consecutive slots
// (or hold consecutive ranks of a drawn chunk), so their rows are consecutive: 768 contiguous bytes per array and wave, read once
// per frame -- streamed past the caches the BVH lives in (RT_RAYS_NONTEMPORAL).
template <class TABLE>
__device__ __forceinline__ void gen_table_ray(const TABLE &tab, unsigned c, AdvanceOut &out) {
    const float *o3 = tab.o3 + 3 * (size_t)c, *d3 = tab.d3 + 3 * (size_t)c;
    out.ray_o = mk(table_load(o3), table_load(o3 + 1), table_load(o3 + 2));
    out.ray_d = mk(table_load(d3), table_load(d3 + 1), table_load(d3 + 2));
}
// gen_camera_ray: the stream (per-sample mode), the two jitter draws, camera.get_ray; the slot starts a new path.
__device__ __forceinline__ void gen_camera_ray(const Camera &cam, const AdvanceParams &ap, long long cid, int px, int py, SlotState &st,
                                               AdvanceOut &out) {
    if (ap.per_sample) st.rs = rng_sample_stream(ap.seed_lo, ap.seed_hi, (unsigned long long)cid * (unsigned)ap.key_mul + (unsigned)ap.key_add);
    float jx = rng_uniform(st.rs);  // x first, then y (Appendix A.7)
    float jy = rng_uniform(st.rs);
    camera_get_ray(cam, (px + jx) / ap.width, (py + jy) / ap.height, out.ray_o, out.ray_d);
    gen_new_path(st, out);
}

// BG_SKIP (advance_core of k_paths<PathsBg>'s 2-waves-per-SIMD builds, where gen() stays inside the ADV block): a background
// camera ray (gen_background) is passed over on the spot -- counted in out.bg_skipped, its two draws made unless every
// camera ray starts a stream of its own -- and the lane takes its slot's next generation.
template <bool NEVER_LOCKSTEP = false, bool BG_SKIP = false, class SRC>
__device__ __forceinline__ void gen_core(const SRC &cam, const AdvanceParams &ap, int slot_global, SlotState &st,
                                         AdvanceOut &out, int *pxy = nullptr, long long cid_given = -1) {
    long long cid;
    if constexpr (BG_SKIP && std::is_same<SRC, Camera>::value) {
        int px, py;
        while (true) {
            if (!gen_begin<NEVER_LOCKSTEP>(ap, slot_global, st, cid_given, cid)) return;
            gen_pixel(ap, slot_global, st, pxy, cid_given, cid, px, py);
            if (!gen_background(ap, px, py)) break;
            if (!ap.per_sample) {
                rng_next(st.rs);
                rng_next(st.rs);
            }
            out.bg_skipped++;
        }
        gen_camera_ray(cam, ap, cid, px, py, st, out);
    } else if constexpr (std::is_same<SRC, CountsCamera>::value) {
        // Counted frames (k_paths<PathsCounts>' 2-waves-per-SIMD builds, where ids are tied to slots): camera ray `cid` of the call is
        // found in the prefix sum over the whole image; a background pixel's ray is counted and passed over without a stream
        // or a ray, as in the per-sample camera path; then the stream of the ray's 64-bit key, the two draws, the pinhole.
        int px, py;
        unsigned long long key;
        while (true) {
            if (!gen_begin<NEVER_LOCKSTEP>(ap, slot_global, st, cid_given, cid)) return;
            counts_locate(cam, (unsigned)cid, 0, cam.n_pixels - 1, ap.width, st.pixel, px, py, key);  // (cid < cam_end < 2^31)
            if (!BG_SKIP || !gen_background(ap, px, py)) break;
            out.bg_skipped++;
        }
        st.rs = rng_sample_stream(ap.seed_lo, ap.seed_hi, key);
        const float jx = rng_uniform(st.rs);  // x first, then y (Appendix A.7)
        const float jy = rng_uniform(st.rs);
        camera_get_ray(cam.cam, (px + jx) / ap.width, (py + jy) / ap.height, out.ray_o, out.ray_d);
        gen_new_path(st, out);
    } else {
        if (!gen_begin<NEVER_LOCKSTEP>(ap, slot_global, st, cid_given, cid)) return;
        if constexpr (std::is_same<SRC, KeyedRayTable>::value) {
            // Keyed ray-table frames: row `cid` starts the per-sample stream of its key (whatever stream the lane held), gen()'s
            // two jitter draws are made and dropped -- a pinhole's own table reproduces the RT_FLAG_RNG_PER_SAMPLE frame draw for
            // draw --, the ray is the row.
            const unsigned c = (unsigned)cid;  // (below 2^31: the host checks the frame)
            const unsigned long long ck = (unsigned long long)c * cam.key_stride;  // (no wrap: c < 2^31, key_stride < 2^32)
            st.rs = rng_sample_stream(ap.seed_lo, ap.seed_hi, cam.key_first + ck);  // (the host refuses keys that wrap)
            rng_next(st.rs);  // x first, then y (Appendix A.7)
            rng_next(st.rs);
            gen_table_ray(cam, c, out);
            if (cam.pixel) {
                st.pixel = table_load(cam.pixel + c);
            } else {
                const unsigned long long t = cam.rem_first + ck;  // K / rays_per_pixel = pix_first + t / rays_per_pixel
                const unsigned q = (t >> 32) ? (unsigned)(t / cam.rays_per_pixel) : (unsigned)t / cam.rays_per_pixel;
                st.pixel = cam.pix_first + (int)q;  // (below n_pixels: the host checks the last key)
            }
            gen_new_path(st, out);
        } else if constexpr (std::is_same<SRC, RayTable>::value) {
            // Ray-table frames: gen()'s two jitter draws are made and dropped (the slot's stream stays where the reference's
            // is), the ray and its pixel are row `cid` of the table.  No pixel coordinates, no stepping (`pxy` is left alone).
            const unsigned c = (unsigned)cid;  // (below 2^31: the host checks the frame)
            rng_next(st.rs);  // x first, then y (Appendix A.7)
            rng_next(st.rs);
            gen_table_ray(cam, c, out);
            st.pixel = cam.pixel ? table_load(cam.pixel + c) : (int)(c / (unsigned)ap.spp);  // (render.cuh:254-256)
            gen_new_path(st, out);
        } else {
            int px, py;
            gen_pixel(ap, slot_global, st, pxy, cid_given, cid, px, py);
            gen_camera_ray(cam, ap, cid, px, py, st, out);
        }
    }
}

// `acc` (USE_ACC, k_paths only): the lane's sample accumulator; otherwise contributions go straight into the framebuffer.
template <bool DEFER_GEN, bool NEVER_LOCKSTEP = false, bool USE_ACC = false, bool BG_SKIP = false, class SRC>
__device__ __forceinline__ void advance_core(const DScene &sc, const float *tab, const SRC &cam,
                                             const AdvanceParams &ap, int slot_global, SlotState &st, AdvanceOut &out,
                                             float *__restrict__ fb, float *acc = nullptr) {
    const bool lockstep = NEVER_LOCKSTEP ? false : (ap.lockstep != 0);
    const int off_ltri = tab_off_ltri(sc.num_mats, sc.num_lights);
    const int off_lpre = tab_off_lpre(sc.num_mats, sc.num_lights);
    out.did_gen = out.did_shade = out.has_shadow = out.did_emit = out.new_ray = out.wants_gen = false;
    out.rr_draws = 0;
    out.bg_skipped = 0;
    const bool hit = st.hit_info >= 0;
    const int light_of_hit = hit ? ((st.hit_info >> 16) & 0xffff) - 1 : -1;
    // Emulate consecutive init() calls (render.cuh:84-137) until one of them ends in mat() or gen(): a slot whose
    // path missed idles (no RNG use) until bounces reaches max_bounces; a slot that Russian roulette "killed" is
    // re-rolled by every following init() (Appendix A.1) -- beta, and with it the kill probability, does not change
    // along such a chain, so the chain is a tight loop of draws.  `lockstep`: exactly one init() per call.
    RT_MARK("adv.init");
    if (st.bounces == 0 && hit && light_of_hit >= 0) {  // :98-103 emission only at bounce 0
        Light l = tab_light(tab, sc.num_mats, light_of_hit);
        if (USE_ACC) acc_add(acc, l.lx, l.ly, l.lz);  // (k_paths; a compile-time choice: `if (acc)` is a per-lane pointer test)
        else deposit(fb, ap.fb_fixed, st.pixel, l.lx, l.ly, l.lz);
        out.did_emit = true;
    }
    const bool cont = st.bounces < ap.max_bounces;  // :109
    if (cont && hit) {
        bool shade = true;
        if (st.bounces > kRrStart && max3(st.beta) < kRrThreshold) {  // :112-124
            // The chain is a lane's own loop inside a whole-wave block: a turn is paid by the wave for as long as its longest
            // lane rolls, so the turn holds only the draw and ONE stop test.  The rolls a lane may make are known before the
            // loop (`cont` holds: at least one); bounces, rr_draws, the survivor bit and the survivor's beta follow from the
            // number of rolls behind it.  beta is neither read nor written in the loop.
            const float pt = fmaxf(0.05f, 1 - max3(st.beta));
            const int limit = lockstep ? 1 : ap.max_bounces - st.bounces;
            int n = 0;
            uint32_t draw;
            bool kill;
            RT_MARK("adv.rr.begin");
            do {
                n++;  // :126
                rng_step(st.rs);
                st.rs.d += kRngWeyl;
                draw = st.rs.v4 + st.rs.d;  // (rng_next)
                kill = rng_to_uniform(draw) < pt;  // (a draw equal to pt survives)
            } while (kill & (n < limit));
            RT_MARK("adv.rr.end");
            // (the test again, on the lane's last draw: carried out of the loop, the bit is kept every turn for the lanes
            // already through -- see gen.loop.end.  The empty statement emits nothing.)
            __asm__ volatile("" : "+v"(draw));
            shade = !(rng_to_uniform(draw) < pt);
            st.bounces = st.bounces + n;
            out.rr_draws = n;
            if (shade) st.beta = divf(st.beta, 1 - pt);
        } else {
            st.bounces = st.bounces + 1;  // :126
        }
        if (shade) out.did_shade = true;
        else if (lockstep) return;  // killed this round; the next round rolls again
    } else {
        if (cont && lockstep) {  // a miss idles: nothing but the counter moves (Appendix A.2)
            st.bounces = st.bounces + 1;
            return;
        }
    }
    if (!out.did_shade) {
        // ---- gen() :250-275 (the init() that finds no bounce left; its own increment of `bounces` is overwritten)
        if (DEFER_GEN) {  // k_paths: camera rays are generated by the (much shorter) GEN block
            out.wants_gen = true;
            return;
        }
        if (USE_ACC) acc_flush(acc, fb, ap.fb_fixed, st.pixel);  // the camera ray that ends here: its sum -> its pixel
        gen_core<NEVER_LOCKSTEP, BG_SKIP>(cam, ap, slot_global, st, out);
        return;
    }
    // ---- mat() :139-248
    RT_MARK("adv.mat.sample_f");
    Material m = tab_material(tab, st.hit_info & 0xffff);
    V3 multiplier = scale(st.beta, (float)sc.num_lights);  // taken BEFORE the beta update (:150)
    int again_draws;
    {
        V3 n = st.isect_n, wi;
        float pdf;
        V3 f = mat_sample_f(m, st.wo, st.rs, n, wi, pdf, again_draws);
        out.ray_o = offset_ray_origin(st.isect_p, n);
        out.ray_d = wi;
        out.new_ray = true;
        st.beta = mul(st.beta, divf(scale(f, dot(wi, n)), pdf));  // :166
    }
    RT_MARK("adv.mat.light_sample");
    if (sc.num_lights > 0) {
        int light_idx = min((int)(rng_uniform(st.rs) * sc.num_lights), sc.num_lights - 1);  // :178
        Light light = tab_light(tab, sc.num_mats, light_idx);
        V3 wi, Li;
        float lt, lpdf;
        // Light::sample_Li light.cuh:29-48
        if (light.type == 0) {
            wi = sub(mk(light.px, light.py, light.pz), st.isect_p);
            lt = len(wi);
            Li = divf(mk(light.lx, light.ly, light.lz), lt * lt);
            wi = divf(wi, lt);
            lpdf = 1.f;
        } else {
            const float *q = tab + off_ltri + 12 * light_idx;
            const float *pre = tab + off_lpre + 4 * light_idx;
            Tri lt_tri;
            lt_tri.p0 = mk(q[0], q[1], q[2]);
            lt_tri.e1 = mk(q[3], q[4], q[5]);
            lt_tri.e2 = mk(q[6], q[7], q[8]);
            lt_tri.n = mk(q[9], q[10], q[11]);
            lpdf = pre[0];                        // 1 / area
            V3 lun = mk(pre[1], pre[2], pre[3]);   // unit normal of the light triangle
            float a = sqrtf(rng_uniform(st.rs));   // Triangle::sample_p triangle.cuh:78-82
            float u2 = rng_uniform(st.rs);
            V3 tp = tri_point(lt_tri, 1 - a, u2 * a);
            wi = sub(tp, st.isect_p);
            lt = len(wi);
            wi = divf(wi, lt);
            Li = mk(light.lx, light.ly, light.lz);
            lpdf *= len2(sub(tp, st.isect_p)) / fabsf(dot(lun, wi));
        }
        RT_MARK("adv.mat.nee");
        V3 n = dot(st.isect_n, wi) > 0.f ? st.isect_n : neg(st.isect_n);  // :187
        V3 f;
        float spdf;
        if (mat_get_f(m, st.wo, wi, n, f, spdf)) {
            f = scale(f, dot(wi, n));
            out.s_o = offset_ray_origin(st.isect_p, n);
            out.s_d = wi;
            out.s_tmax = lt;
            out.s_target = light.type == 1 ? light.tri : -1;
            if (light.type == 0) {
                out.s_L = divf(mul(mul(multiplier, f), Li), lpdf);  // :199
            } else {
                float weight = power_heuristic(lpdf, spdf);  // :201 (int-truncating)
                out.s_L = divf(scale(mul(mul(multiplier, f), Li), weight), lpdf);  // :202
            }
            out.has_shadow = true;
        }
        // "sample BSDF with MIS" block :213-245: its ray cannot contribute; keep its draws
        RT_MARK("adv.mat.burn");
        if (light.type != 0) {  // (the first call already knows how many: see mat_sample_f)
            if (again_draws >= 1) rng_next(st.rs);
            if (again_draws >= 2) rng_next(st.rs);
        }
    }
    RT_MARK("adv.mat.end");
}

// k_advance (init() + mat() + gen() for all slots of a round) is defined with k_paths in rt_frame_kernels.inc.

#include "rt_walk.inc"            // traversal: box test, stack, inner_step; reference_walk; VERIFY (ref_visible)
#include "rt_stream_kernels.inc"  // k_trace, the query prepasses, k_query, k_aov, k_motion, k_aov_resolve

// ============================================================================ k_paths
// The whole asynchronous part of a frame in ONE launch.  A lane owns one path slot for the entire
// render and keeps its state in registers; the reference's stage kernels become PHASES of the lane:
//     ADV      init() + mat()                (advance_core; + gen() on small shards)
//     GEN      gen()                         (gen_core)
//     ANY      ah():  the slot's shadow ray  (any hit, deposit if unoccluded)
//     CLOSEST  ch():  the slot's path ray    (closest hit -> hit record for the next ADV)
// Because a slot never depends on another slot (see the file header) there is no barrier of any
// kind between rounds: a wave simply keeps all 64 of its slots moving until each has run out of
// camera rays (or parks for the lockstep final generation).  That removes what dominated the
// per-round design -- every k_trace launch ended in a drain where a wave waited for its longest
// ray with ~10 of 64 lanes active, 1 700 times per frame -- together with the per-round state
// traffic (rays, hit records and shadow rays never leave registers) and 3 400 kernel launches.
// Divergence between phases is handled by wave-level scheduling: each iteration the wave issues ONE
// block for all its lanes -- the expensive ADV block when at least `adv_batch` lanes wait for it (or
// nothing else can run), the short GEN block (gen() alone, for paths that certainly ended) when
// `gen_batch` lanes wait for it, otherwise the more popular of a node block (up to 8 node steps) and a
// triangle block (up to 2 tests).
enum { PH_ADV = 0, PH_ANY = 1, PH_CLOSEST = 2, PH_IDLE = 3, PH_GEN = 4 };
#ifndef RT_TRI_PER_STEP
#define RT_TRI_PER_STEP 2
#endif
constexpr int kCidChunk = 512;  // camera-ray ids a wave draws at a time in the per-sample RNG mode
constexpr int kTriPerStep = RT_TRI_PER_STEP;  // triangle tests a lane makes per scheduled triangle block
#ifndef RT_NODE_PER_STEP
#define RT_NODE_PER_STEP 8
#endif
constexpr int kNodePerStep = RT_NODE_PER_STEP;  // node steps a lane makes per scheduled node block (2-wide records)
#ifndef RT_NODE_PER_STEP_WIDE
#define RT_NODE_PER_STEP_WIDE 2
#endif
constexpr int kNodePerStepWide = RT_NODE_PER_STEP_WIDE;  // ... with 4-wide nodes (measured: 3 649 / 3 620 / 3 539 / 3 391 Msamples/s at 2 / 3 / 4 / 5)
// 4-wide node blocks are adaptive: kNodePerStepWide steps for every lane that has one to make, then -- if at least
// kNodeCont lanes of the wave still do -- up to kNodeExtra more (a wave-uniform branch).  Measured on the four BASELINE
// scenes against fixed 2 / 3 / 4 / 5 steps: fixed 4 is 8 % faster on the sixteen-light scene (its shadow rays make
// 4.8 node steps against 2.2 in C2) and 5 % slower on the matte scene; 2 + 2 at >= 36 lanes is at least as fast as
// fixed 2 on all four.  A `do ... while (enough lanes)` loop that is not unrolled loses 1 %.
#ifndef RT_NODE_CONT
#define RT_NODE_CONT 36
#endif
#ifndef RT_NODE_EXTRA
#define RT_NODE_EXTRA 2
#endif
constexpr int kNodeCont = RT_NODE_CONT, kNodeExtra = RT_NODE_EXTRA;
#ifndef RT_SPECULATE
#define RT_SPECULATE 1
#endif

constexpr bool kSpeculate = RT_SPECULATE != 0;  // k_paths: postpone a leaf reached inside a node block (see `pend` there)

// Register diet: across loop iterations a lane carries only ONE ray (o, d, 1/d, tmax) and the
// traversal cursor (cur, sp, tri, hu, hv).  The slot's persistent state (bounces, pixel, gen, RNG,
// beta = 12 dwords) lives in the lane's LDS column and is only in registers inside the ADV block;
// while a shadow ray is traced, the slot's path ray and the radiance to deposit wait in 9 more
// dwords of LDS; the hit record is rebuilt from (tri, hu, hv) inside the ADV block.
// LDS layout (dynamic): [stack: (stack_cap + 1) x kBlock (push_if)][parked ray: 9 x kBlock][slot state: 12 + 1 x kBlock][sample sum: 3 x kBlock][tables]
// LITERAL (RT_FLAG_REFERENCE_WALK): the node block is a lane's WHOLE ray through reference_walk -- the reference's tree,
// box test, order and tie rule; no triangle blocks, no speculation.  Everything around it (phases, ADV / GEN blocks, the
// sample accumulator) is the same code.  Opt-in and never timed.
// VERIFY (the default build; off with RT_FLAG_WATERTIGHT): the reference's decisions on this kernel's own walk (see
// ref_visible): a shadow ray's accepted hit counts only if the reference's walk can see its triangle (triangle block); a
// path ray's closest hit is checked once, at the top of the ADV block that shades it -- visible, and no exact tie at the
// final distance -- and the ~2 rays in 10^7 that fail are re-traced there by reference_walk.
#ifdef RT_TRACE_PROFILE
constexpr int kProfHead = 26;  // qwords of k_paths' totals
constexpr int kProfRec = 6;    // qwords of k_paths' per-wave record (behind the totals)
#endif
// The two kernels of a frame are templates (rt_frame_kernels.inc): k_advance<SRC, LDS_TABLES> over the source of camera rays (see
// gen_core) and k_paths<BUILD, ...> over a build tag.  A tag names the source type and the axes that are compiled in or out:
// kChunks (the chunked deal, rt_slot_chunks.h), kBg (gen() passes over background pixels: rt_background.h, gen_background) and
// kCounts (a counted frame's ids: the prefix sum of the count map).  One NAMED tag per build that is launched, so that a
// profile's or a resource remark's kernel name says which build it is (k_paths<PathsChunkedBg, ...>); a new source or a new axis
// is one more tag here and one more line in the host's selection (FrameRun::run_persistent).  An axis is a compile-time
// constant and not a kernel argument so that a build carries nothing of what it does not run, instruction for instruction:
// tools/device_code_diff.py on two builds' assembly is the check.
// k_advance exists for the sources whose frames can run on the round pipeline: Camera and RayTable.  Per-sample streams (keyed
// tables, counted frames) run on the persistent kernel only.
struct PathsCamera {  // the camera's frame, static deal, nothing to skip: every frame that no other tag takes
    using Src = Camera;
    static constexpr bool kChunks = false, kBg = false, kCounts = false;
};
struct PathsRays {  // rt_render_rays_*: camera ray c is row c of the caller's table.  Tables keep the static deal: no table frame has
    using Src = RayTable;  // been timed with the chunked one
    static constexpr bool kChunks = false, kBg = false, kCounts = false;
};
struct PathsKeyed {  // rt_render_rays_keyed_*: a table with a per-sample stream per row
    using Src = KeyedRayTable;
    static constexpr bool kChunks = false, kBg = false, kCounts = false;
};
// The camera with the chunked deal compiled in: launched instead of the 4-waves-per-SIMD reference-mode PathsCamera builds when the
// launch plan picks a chunk, and only those instances exist.  A tag of its own so that the static deal keeps its code: with the
// deal's code in it the static deal was 2.5 % slower (see s_task in k_paths).
struct PathsChunked {
    using Src = Camera;
    static constexpr bool kChunks = true, kBg = false, kCounts = false;
};
// Both camera builds with the background skip compiled into gen(): launched instead of PathsCamera / PathsChunked when the frame's
// rectangle (AdvanceParams::bg_*) is smaller than the frame.  A frame with nothing to skip keeps a kernel of its own because the
// skipping GEN block with a whole-frame rectangle cost C2 3 %.
struct PathsBg {
    using Src = Camera;
    static constexpr bool kChunks = false, kBg = true, kCounts = false;
};
struct PathsChunkedBg {
    using Src = Camera;
    static constexpr bool kChunks = true, kBg = true, kCounts = false;
};
// rt_render_counts_fixed: the skipping text, whose GEN block finds a drawn id's pixel and sample in the prefix sum of the count
// map.  Per-sample streams, so of it the two per-sample builds per table placement.
struct PathsCounts {
    using Src = CountsCamera;
    static constexpr bool kChunks = false, kBg = true, kCounts = true;
};
#include "rt_frame_kernels.inc"

// The prepass of a counted frame, three kernels on the caller's stream.  A workgroup serves kCountsTile consecutive pixels, a lane
// kCountsItems consecutive ones of them.  words[0]: pixels whose (first, count) the call refuses; words[1]: the sum of the counts;
// words[2 + b]: the sum over tile b, then (k_counts_scan) the sum over the tiles before b.
// k_counts_sums writes the words only; the host reads words[0 .. 1] and decides; k_counts_offsets then writes the prefix sum the
// frame kernel searches and makes the caller's d_samples add.
constexpr int kCountsItems = 4, kCountsTile = kCountsItems * 256;
__global__ void __launch_bounds__(256)
k_counts_sums(const int32_t *__restrict__ first, const int32_t *__restrict__ count, int n, uint32_t stride, unsigned long long *__restrict__ words) {
    __shared__ unsigned long long s_sum[4];
    __shared__ unsigned s_bad[4];
    const unsigned base = (blockIdx.x * 256u + threadIdx.x) * (unsigned)kCountsItems;  // (n + kCountsTile < 2^31)
    unsigned long long sum = 0;
    unsigned bad = 0;
    for (unsigned k = 0; k < (unsigned)kCountsItems; k++) {
        const unsigned p = base + k;
        if (p < (unsigned)n) {
            const long long c = count[p], f = first ? first[p] : 0;
            const bool b = c < 0 || f < 0 || f + c > (long long)stride;  // (64-bit: no int32 overflow)
            bad += b ? 1u : 0u;
            sum += b ? 0ull : (unsigned long long)c;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off);
        bad += __shfl_xor(bad, off);
    }
    if ((threadIdx.x & 63u) == 0u) {
        s_sum[threadIdx.x >> 6] = sum;
        s_bad[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        words[2 + blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        const unsigned b = s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
        if (b) atomicAdd(&words[0], (unsigned long long)b);
    }
}
// an inclusive scan over the 256 values of a workgroup, one per lane, through `s` (256 words)
template <class T>
__device__ __forceinline__ T counts_block_scan(T *s, T v) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (unsigned off = 1; off < 256u; off <<= 1) {
        const T t = threadIdx.x >= off ? s[threadIdx.x - off] : (T)0;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    return s[threadIdx.x];
}
// one workgroup: the tiles' sums -> the sums before each tile, and the total
__global__ void __launch_bounds__(256) k_counts_scan(unsigned long long *__restrict__ words, int n_tiles) {
    __shared__ unsigned long long s[256];
    unsigned long long carry = 0;
    for (int base = 0; base < n_tiles; base += 256) {
        const int i = base + (int)threadIdx.x;
        const unsigned long long v = i < n_tiles ? words[2 + i] : 0ull;
        const unsigned long long incl = counts_block_scan(s, v);
        const unsigned long long tile_total = s[255];
        if (i < n_tiles) words[2 + i] = carry + incl - v;
        carry += tile_total;
        __syncthreads();  // (s is written again in the next turn)
    }
    if (threadIdx.x == 0) words[1] = carry;
}
// (every (first, count) has passed and the total is below 2^31: the host has looked)
__global__ void __launch_bounds__(256)
k_counts_offsets(const int32_t *__restrict__ count, int n, const unsigned long long *__restrict__ words, uint32_t *__restrict__ offset,
                 int32_t *__restrict__ samples) {
    __shared__ unsigned s[256];
    const unsigned base = (blockIdx.x * 256u + threadIdx.x) * (unsigned)kCountsItems;
    unsigned c[kCountsItems], mine = 0;
    for (unsigned k = 0; k < (unsigned)kCountsItems; k++) {
        c[k] = base + k < (unsigned)n ? (unsigned)count[base + k] : 0u;
        mine += c[k];
    }
    unsigned at = (unsigned)words[2 + blockIdx.x] + (counts_block_scan(s, mine) - mine);
    for (unsigned k = 0; k < (unsigned)kCountsItems; k++) {
        const unsigned p = base + k;
        if (p < (unsigned)n) {
            offset[p] = at;
            if (samples && c[k]) samples[p] += (int32_t)c[k];
        }
        at += c[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) offset[n] = (unsigned)words[1];
}

// rt_normalize_counts_fixed: sums with a per-pixel divisor -> sums of ONE sample of the mean, sign(s) * ((|s| + (n >> 1)) / n) in
// 64-bit integers; n == 0 gives 0.  k_counts_negative counts the pixels with a negative divisor first (nothing is written then).
__global__ void k_counts_negative(const int32_t *__restrict__ samples, int n, unsigned long long *__restrict__ words) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long m = wave_ballot(i < n && samples[i] < 0);
    if (m != 0ull && lane_id() == 0) atomicAdd(&words[0], (unsigned long long)__popcll(m));
}
__global__ void k_normalize_counts(const long long *__restrict__ sums, const int32_t *__restrict__ samples, int n_values, long long *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_values) return;
    const long long s = sums[i];
    const unsigned long long n = (unsigned long long)samples[(unsigned)i / 3u];
    long long r = 0;
    if (n) {
        const unsigned long long a = s < 0 ? 0ull - (unsigned long long)s : (unsigned long long)s;
        const long long q = (long long)((a + (n >> 1)) / n);
        r = s < 0 ? -q : q;
    }
    out[i] = r;
}
// rt_post_process_counts_fixed: k_post_process_fixed with the pixel's own count; n == 0 gives 0
__global__ void k_post_process_counts(const long long *__restrict__ sums, const int32_t *__restrict__ samples, float *__restrict__ out, int n_values) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_values) return;
    const int n = samples[(unsigned)i / 3u];
    out[i] = n > 0 ? sqrtf((float)((double)sums[i] * (1.0 / 1073741824.0)) * (1.f / (float)n)) : 0.f;
}

// rt_sample_allocate.  The quantised weight: 0 unless w > 0 (NaN, zero, negatives), else floor(min(w, 4096) * 2^20), every step
// exact in fp32 and at most 2^32.  k_allocate_total: words[0] = T, the sum of the quantised weights (64-bit integer adds: any order).
// k_allocate_counts: count = min(max_count, min_count + (T ? extra * q / T : extra / n)) and words[1] = the sum of the counts.
__device__ __forceinline__ unsigned long long allocate_weight(float w) {
    return w > 0.f ? (unsigned long long)floorf(fminf(w, 4096.f) * 1048576.f) : 0ull;
}
__device__ __forceinline__ void allocate_wave_add(unsigned long long v, unsigned long long *word) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (v != 0ull && lane_id() == 0) atomicAdd(word, v);
}
__global__ void k_allocate_total(const float *__restrict__ weight, int n, unsigned long long *__restrict__ words) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    allocate_wave_add(i < n ? allocate_weight(weight[i]) : 0ull, &words[0]);
}
__global__ void k_allocate_counts(const float *__restrict__ weight, int n, int min_count, int max_count, unsigned long long extra,
                                  unsigned long long *__restrict__ words, int32_t *__restrict__ count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long total = words[0];
    unsigned long long c = 0;
    if (i < n) {
        const unsigned long long more = total ? extra * allocate_weight(weight[i]) / total : extra / (unsigned long long)n;  // (extra < 2^31, q <= 2^32)
        c = min((unsigned long long)max_count, (unsigned long long)min_count + more);
        count[i] = (int32_t)c;
    }
    allocate_wave_add(c, &words[1]);
}

// post_process_framebuffer (render.cuh:330-338): c = sqrt(c * (1/spp))
__global__ void k_post_process(float *fb, int n_values, float inv_spp) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_values) fb[i] = sqrtf(fb[i] * inv_spp);
}

// fixed-point sums -> post-processed image: c = sqrt(float(sum * 2^-30) * (1/spp))
__global__ void k_post_process_fixed(const long long *__restrict__ sums, float *__restrict__ out, int n_values, float inv_spp) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_values) out[i] = sqrtf((float)((double)sums[i] * (1.0 / 1073741824.0)) * inv_spp);
}

// rt_render_multi: dst += src over the raw sums of two shards (fp32 sums, or the int64 fixed-point sums of RT_FLAG_DETERMINISTIC)
__global__ void k_accumulate_f32(float *__restrict__ dst, const float *__restrict__ src, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}
__global__ void k_accumulate_i64(long long *__restrict__ dst, const long long *__restrict__ src, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

// ---- stage-level test kernels
__global__ void k_test_draw(DPools p, int n, int draws, uint32_t *__restrict__ state6, float *__restrict__ uni) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng rs{p.rd(i), p.r0(i), p.r1(i), p.r2(i), p.r3(i), p.r4(i)};
    for (int k = 0; k < draws; k++) uni[(size_t)i * draws + k] = rng_uniform(rs);
    state6[6 * (size_t)i + 0] = rs.d;
    state6[6 * (size_t)i + 1] = rs.v0;
    state6[6 * (size_t)i + 2] = rs.v1;
    state6[6 * (size_t)i + 3] = rs.v2;
    state6[6 * (size_t)i + 4] = rs.v3;
    state6[6 * (size_t)i + 5] = rs.v4;
}
#include "rt_build_kernels.inc"   // device BVH: the leaf-order arrays, refit (k_refit_*), build (k_ploc_*)
#include "rt_denoise_kernels.inc"  // dn_filter_pixel under k_atrous* and k_atrous_var*; k_dn_prepare*, k_dn_var_blur, k_dn_finish*
#include "rt_temporal_kernels.inc"  // k_temporal_accumulate_moments, k_temporal_accumulate
#include "rt_upsample_kernels.inc"  // k_upsample<F, kRgb>: a tile of full pixels from its low-resolution footprint in LDS

#include "rt_host_scene.inc"   // (opens the anonymous namespace that is closed below) rt_scene: reference tree, checks, build / emit / adopt, create, update, rebuild, edits; what the ray entry points share
#include "rt_host_render.inc"  // Context, cached output buffers, kernel selection, one shard of a frame, queries and trace hooks, ray tables, AOVs
#include "rt_host_frame.inc"   // whole frames: the shard fan-out (RT_SPLIT, rt_render_multi), finish_frame, rt_render, rt_render_multi
#include "rt_host_denoise.inc"  // rt_denoise_fixed, rt_denoise_dual_fixed, rt_denoise_variance_fixed, rt_upsample_fixed / rt_upsample_rgb
#include "rt_host_temporal.inc"  // rt_temporal_accumulate_fixed, rt_temporal_accumulate_moments_fixed
#include "rt_host_counts.inc"  // rt_normalize_counts_fixed, rt_post_process_counts_fixed, rt_sample_allocate
}  // namespace

// ============================================================================ C-ABI
extern "C" {

const char *rt_last_error(void) { return g_last_error.c_str(); }
const char *rt_peer_access_log(void) { return g_peer_log.c_str(); }
const char *rt_version(void) { return "rtcuda_amd 0.1 (gfx950)"; }
#ifndef RT_BUILD_ID
#define RT_BUILD_ID "unknown"
#endif
const char *rt_build_id(void) { return RT_BUILD_ID; }

int rt_scene_create(const float *tri_p0p1p2, int n_tris, const int32_t *tri_material, const int32_t *tri_light,
                    const rt_material *materials, int n_materials, const rt_light *lights, int n_lights,
                    rt_scene **out_scene) {
    return scene_create_impl(tri_p0p1p2, n_tris, tri_material, tri_light, materials, n_materials, lights, n_lights, 0u, out_scene);
}

int rt_scene_create_flags(const float *tri_p0p1p2, int n_tris, const int32_t *tri_material, const int32_t *tri_light,
                          const rt_material *materials, int n_materials, const rt_light *lights, int n_lights,
                          uint32_t scene_flags, rt_scene **out_scene) {
    return scene_create_impl(tri_p0p1p2, n_tris, tri_material, tri_light, materials, n_materials, lights, n_lights, scene_flags, out_scene);
}

void rt_scene_destroy(rt_scene *scene) { delete scene; }  // (~rt_scene frees the device arrays)

int rt_scene_info(const rt_scene *scene, int64_t out[4]) {
    if (!scene || !out) return fail("rt_scene_info: null argument");
    out[0] = scene->n_nodes;
    out[1] = scene->n_tris;
    out[2] = scene->max_depth;
    out[3] = scene->n_leaves;
    return 0;
}

int rt_scene_build_info(const rt_scene *scene, int *builder, double *seconds) {
    if (!scene || !builder || !seconds) return fail("rt_scene_build_info: null argument");
    *builder = scene->builder;
    *seconds = scene->build_seconds;
    return 0;
}

int rt_scene_update(rt_scene *scene, const float *tri_p0p1p2, int n_tris) {
    return scene_update_impl(scene, tri_p0p1p2, n_tris, false, nullptr, "rt_scene_update");
}

int rt_scene_update_device(rt_scene *scene, const float *d_tri_p0p1p2, int n_tris, void *stream) {
    return scene_update_impl(scene, d_tri_p0p1p2, n_tris, true, (hipStream_t)stream, "rt_scene_update_device");
}

int rt_scene_rebuild(rt_scene *scene, const float *tri_p0p1p2, int n_tris) {
    return scene_rebuild_impl(scene, tri_p0p1p2, n_tris, false, nullptr, "rt_scene_rebuild");
}

int rt_scene_rebuild_device(rt_scene *scene, const float *d_tri_p0p1p2, int n_tris, void *stream) {
    return scene_rebuild_impl(scene, d_tri_p0p1p2, n_tris, true, (hipStream_t)stream, "rt_scene_rebuild_device");
}

int rt_scene_set_materials(rt_scene *scene, const rt_material *materials, int n_materials) {
    return scene_set_materials_impl(scene, materials, n_materials);
}

int rt_scene_set_lights(rt_scene *scene, const rt_light *lights, int n_lights, const int32_t *tri_light) {
    return scene_set_lights_impl(scene, lights, n_lights, tri_light);
}

int rt_scene_set_triangles(rt_scene *scene, const float *tri_p0p1p2, int n_tris, const int32_t *tri_material, const int32_t *tri_light,
                           const rt_material *materials, int n_materials, const rt_light *lights, int n_lights) {
    return scene_set_triangles_impl(scene, tri_p0p1p2, n_tris, tri_material, tri_light, materials, n_materials, lights, n_lights, false,
                                    nullptr, "rt_scene_set_triangles");
}

int rt_scene_set_triangles_device(rt_scene *scene, const float *d_tri_p0p1p2, int n_tris, const int32_t *d_tri_material,
                                  const int32_t *d_tri_light, const rt_material *materials, int n_materials, const rt_light *lights,
                                  int n_lights, void *stream) {
    return scene_set_triangles_impl(scene, d_tri_p0p1p2, n_tris, d_tri_material, d_tri_light, materials, n_materials, lights, n_lights,
                                    true, (hipStream_t)stream, "rt_scene_set_triangles_device");
}

int rt_scene_create_device(const float *d_tri_p0p1p2, int n_tris, const int32_t *d_tri_material, const int32_t *d_tri_light,
                           const rt_material *materials, int n_materials, const rt_light *lights, int n_lights, void *stream,
                           rt_scene **out_scene) {
    return scene_create_device_impl(d_tri_p0p1p2, n_tris, d_tri_material, d_tri_light, materials, n_materials, lights, n_lights,
                                    (hipStream_t)stream, out_scene);
}

int rt_scene_refit_info(const rt_scene *scene, int64_t *refits, double *seconds_last, double *sah_ratio) {
    if (!scene || !refits || !seconds_last || !sah_ratio) return fail("rt_scene_refit_info: null argument");
    *refits = scene->refits;
    *seconds_last = scene->refit_seconds;
    *sah_ratio = scene->sah_build > 0.0 ? scene->sah_now / scene->sah_build : 1.0;
    return 0;
}

int rt_camera_make(const float lookfrom[3], const float lookat[3], const float up[3], float vfov_deg,
                   float aspect_ratio, rt_camera *out) {
    if (!lookfrom || !lookat || !up || !out) return fail("rt_camera_make: null argument");
    // camera.cuh:15-29, host fp32 (tanf from the host libm, as in the reference)
    const float pi = 3.14159265358979323846f;
    float vfov_rad = vfov_deg * (pi / 180.f);
    float vh = 2.f * tanf(vfov_rad * 0.5f);
    float vw = vh * aspect_ratio;
    auto sub3 = [](const float *a, const float *b, float *r) { r[0] = a[0] - b[0]; r[1] = a[1] - b[1]; r[2] = a[2] - b[2]; };
    auto dot3 = [](const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    auto unit3 = [&](float *a) {
        float inv = 1.f / sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        a[0] *= inv; a[1] *= inv; a[2] *= inv;
    };
    float w[3], v[3], u[3];
    sub3(lookfrom, lookat, w);
    unit3(w);
    float duw = dot3(up, w);
    v[0] = up[0] - duw * w[0];
    v[1] = up[1] - duw * w[1];
    v[2] = up[2] - duw * w[2];
    unit3(v);
    u[0] = v[1] * w[2] - v[2] * w[1];
    u[1] = v[2] * w[0] - v[0] * w[2];
    u[2] = v[0] * w[1] - v[1] * w[0];
    for (int a = 0; a < 3; a++) {
        out->lookfrom[a] = lookfrom[a];
        out->horizontal[a] = vw * u[a];
        out->vertical[a] = -vh * v[a];
    }
    for (int a = 0; a < 3; a++)
        out->upper_left[a] = ((lookfrom[a] - w[a]) - 0.5f * out->horizontal[a]) - 0.5f * out->vertical[a];
    return 0;
}

int rt_render_shard(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples,
                    int max_bounces, uint64_t seed, int shard_index, int shard_count, uint32_t flags,
                    float *d_sum_rgb, void *stream, rt_stats *stats) {
    return render_overlapped(scene, camera, width, height, num_samples, max_bounces, seed, shard_index, shard_count,
                             flags & ~kFlagFixedFb, d_sum_rgb, (hipStream_t)stream, stats);
}

int rt_render_shard_fixed(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples,
                          int max_bounces, uint64_t seed, int shard_index, int shard_count, uint32_t flags,
                          int64_t *d_sum_fixed, void *stream, rt_stats *stats) {
    return render_overlapped(scene, camera, width, height, num_samples, max_bounces, seed, shard_index, shard_count,
                             (flags & ~kFlagFixedFb) | kFlagFixedFb, (float *)d_sum_fixed, (hipStream_t)stream, stats);
}

int rt_render_rays_device(const rt_scene *scene, int64_t n_rays, const float *d_origin_xyz, const float *d_dir_xyz, const int32_t *d_pixel,
                          int rays_per_pixel, int n_pixels, int max_bounces, uint64_t seed, uint32_t flags, float *d_sum_rgb, void *stream,
                          rt_stats *stats) {
    if (flags & kFlagFixedFb) return fail("rt_render_rays_device: unknown flag 0x200");
    return render_rays_impl(scene, n_rays, d_origin_xyz, d_dir_xyz, d_pixel, rays_per_pixel, n_pixels, max_bounces, seed, flags, d_sum_rgb,
                            (hipStream_t)stream, stats);
}

int rt_render_rays_keyed_device(const rt_scene *scene, int64_t n_rays, const float *d_origin_xyz, const float *d_dir_xyz,
                                const int32_t *d_pixel, int rays_per_pixel, int n_pixels, int max_bounces, uint64_t seed,
                                uint64_t key_first, uint32_t key_stride, uint32_t flags, float *d_sum_rgb, void *stream, rt_stats *stats) {
    if (flags & kFlagFixedFb) return fail("rt_render_rays_keyed_device: unknown flag 0x200");
    return render_rays_keyed_impl(scene, n_rays, d_origin_xyz, d_dir_xyz, d_pixel, rays_per_pixel, n_pixels, max_bounces, seed, key_first,
                                  key_stride, flags, d_sum_rgb, (hipStream_t)stream, stats);
}

int rt_render_rays_keyed_fixed_device(const rt_scene *scene, int64_t n_rays, const float *d_origin_xyz, const float *d_dir_xyz,
                                      const int32_t *d_pixel, int rays_per_pixel, int n_pixels, int max_bounces, uint64_t seed,
                                      uint64_t key_first, uint32_t key_stride, uint32_t flags, int64_t *d_sum_fixed, void *stream,
                                      rt_stats *stats) {
    if (flags & kFlagFixedFb) return fail("rt_render_rays_keyed_fixed_device: unknown flag 0x200");
    return render_rays_keyed_impl(scene, n_rays, d_origin_xyz, d_dir_xyz, d_pixel, rays_per_pixel, n_pixels, max_bounces, seed, key_first,
                                  key_stride, flags | kFlagFixedFb, (float *)d_sum_fixed, (hipStream_t)stream, stats);
}

int rt_render_rays_fixed_device(const rt_scene *scene, int64_t n_rays, const float *d_origin_xyz, const float *d_dir_xyz,
                                const int32_t *d_pixel, int rays_per_pixel, int n_pixels, int max_bounces, uint64_t seed, uint32_t flags,
                                int64_t *d_sum_fixed, void *stream, rt_stats *stats) {
    if (flags & kFlagFixedFb) return fail("rt_render_rays_fixed_device: unknown flag 0x200");
    return render_rays_impl(scene, n_rays, d_origin_xyz, d_dir_xyz, d_pixel, rays_per_pixel, n_pixels, max_bounces, seed, flags | kFlagFixedFb,
                            (float *)d_sum_fixed, (hipStream_t)stream, stats);
}

int rt_render_counts_fixed(const rt_scene *scene, const rt_camera *camera, int width, int height, int sample_stride, const int32_t *d_first,
                           const int32_t *d_count, int max_bounces, uint64_t seed, uint32_t flags, int64_t *d_sum_fixed, int32_t *d_samples,
                           void *stream, rt_stats *stats) {
    if (flags & kFlagFixedFb) return fail("rt_render_counts_fixed: unknown flag 0x200");
    return render_counts_impl(scene, camera, width, height, sample_stride, d_first, d_count, max_bounces, seed, flags, d_sum_fixed, d_samples,
                              (hipStream_t)stream, stats);
}

int rt_normalize_counts_fixed(const int64_t *d_sum_fixed, const int32_t *d_samples, int num_pixels, int64_t *d_out_fixed, void *stream) {
    return normalize_counts_impl(d_sum_fixed, d_samples, num_pixels, d_out_fixed, (hipStream_t)stream);
}

int rt_post_process_counts_fixed(const int64_t *d_sum_fixed, const int32_t *d_samples, int num_pixels, float *d_rgb_out, void *stream) {
    return post_process_counts_impl(d_sum_fixed, d_samples, num_pixels, d_rgb_out, (hipStream_t)stream);
}

int rt_sample_allocate(const float *d_weight, int num_pixels, int min_count, int max_count, int64_t budget, int32_t *d_count_out,
                       int64_t *total_out, void *stream) {
    return sample_allocate_impl(d_weight, num_pixels, min_count, max_count, budget, d_count_out, total_out, (hipStream_t)stream);
}

int rt_post_process_fixed(const int64_t *d_sum_fixed, float *d_rgb_out, int num_pixels, int num_samples, void *stream) {
    if (!d_sum_fixed || !d_rgb_out || num_pixels <= 0 || num_samples <= 0) return fail("rt_post_process_fixed: bad argument");
    if (num_pixels > 0x7fffffff / 3) return fail("rt_post_process_fixed: more than 715827882 pixels");
    return post_process_impl((const long long *)d_sum_fixed, d_rgb_out, num_pixels, num_samples, (hipStream_t)stream);
}

int rt_render_aov_fixed(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples, uint64_t seed,
                        int shard_index, int shard_count, uint32_t flags, int64_t *d_aov_fixed, int32_t *d_ids, void *stream,
                        rt_stats *stats) {
    return render_aov_impl("rt_render_aov_fixed", scene, camera, width, height, num_samples, seed, shard_index, shard_count, flags, 0,
                           d_aov_fixed, d_ids, (hipStream_t)stream, stats);
}
int rt_render_aov_follow_fixed(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples, uint64_t seed,
                               int shard_index, int shard_count, uint32_t flags, int max_specular, int64_t *d_aov_fixed,
                               int32_t *d_ids, void *stream, rt_stats *stats) {
    return render_aov_impl("rt_render_aov_follow_fixed", scene, camera, width, height, num_samples, seed, shard_index, shard_count,
                           flags, max_specular, d_aov_fixed, d_ids, (hipStream_t)stream, stats);
}

int rt_render_aov_rays_fixed_device(const rt_scene *scene, int64_t n_rays, const float *d_origin_xyz, const float *d_dir_xyz,
                                    const int32_t *d_pixel, int rays_per_pixel, int n_pixels, uint64_t key_first,
                                    uint32_t key_stride, uint32_t flags, int64_t *d_aov_fixed, int32_t *d_ids, void *stream,
                                    rt_stats *stats) {
    return render_aov_rays_impl("rt_render_aov_rays_fixed_device", scene, n_rays, d_origin_xyz, d_dir_xyz, d_pixel, rays_per_pixel,
                                n_pixels, 0, key_first, key_stride, flags, 0, d_aov_fixed, d_ids, (hipStream_t)stream, stats);
}
int rt_render_aov_follow_rays_fixed_device(const rt_scene *scene, int64_t n_rays, const float *d_origin_xyz, const float *d_dir_xyz,
                                           const int32_t *d_pixel, int rays_per_pixel, int n_pixels, uint64_t seed,
                                           uint64_t key_first, uint32_t key_stride, uint32_t flags, int max_specular,
                                           int64_t *d_aov_fixed, int32_t *d_ids, void *stream, rt_stats *stats) {
    return render_aov_rays_impl("rt_render_aov_follow_rays_fixed_device", scene, n_rays, d_origin_xyz, d_dir_xyz, d_pixel,
                                rays_per_pixel, n_pixels, seed, key_first, key_stride, flags, max_specular, d_aov_fixed, d_ids,
                                (hipStream_t)stream, stats);
}

int rt_aov_resolve(const int64_t *d_aov_fixed, float *d_out, int n_pixels, int num_samples, void *stream) {
    if (!d_aov_fixed || !d_out) return fail(std::string("rt_aov_resolve: null ") + (!d_aov_fixed ? "d_aov_fixed" : "d_out"));
    if (n_pixels < 1 || num_samples < 1) return fail("rt_aov_resolve: n_pixels and num_samples must be at least 1");
    const long long nv = (long long)n_pixels * RT_AOV_CHANNELS;
    const float inv = 1.f / (float)num_samples;
    hipLaunchKernelGGL(k_aov_resolve, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const long long *)d_aov_fixed, d_out, nv, inv);
    HIP_TRY(hipGetLastError());
    return 0;
}

int64_t rt_denoise_scratch_bytes(int width, int height) { return denoise_scratch_bytes(width, height); }

int rt_denoise_default_params(rt_denoise_params *out) {
    if (!out) return fail("rt_denoise_default_params: null out");
    *out = denoise_defaults();
    return 0;
}

int rt_denoise_fixed(const int64_t *d_sum_fixed, int num_samples, const int64_t *d_aov_fixed, int aov_samples, int width, int height,
                     const rt_denoise_params *params, void *d_scratch, float *d_rgb_out, void *stream) {
    return denoise_impl(d_sum_fixed, num_samples, d_aov_fixed, aov_samples, width, height, params, d_scratch, d_rgb_out,
                        (hipStream_t)stream);
}

int64_t rt_denoise_dual_scratch_bytes(int width, int height) { return denoise_dual_scratch_bytes(width, height); }

int rt_denoise_dual_default_params(rt_denoise_dual_params *out) {
    if (!out) return fail("rt_denoise_dual_default_params: null out");
    *out = denoise_dual_defaults();
    return 0;
}

int rt_denoise_dual_fixed(const int64_t *d_sum_a, int samples_a, const int64_t *d_sum_b, int samples_b, const int64_t *d_aov_fixed,
                          int aov_samples, int width, int height, const rt_denoise_dual_params *params, void *d_scratch,
                          float *d_rgb_out, void *stream) {
    return denoise_dual_impl(d_sum_a, samples_a, d_sum_b, samples_b, d_aov_fixed, aov_samples, width, height, params, d_scratch,
                             d_rgb_out, (hipStream_t)stream);
}

int rt_upsample_default_params(rt_upsample_params *out) {
    if (!out) return fail("rt_upsample_default_params: null out");
    *out = upsample_defaults();
    return 0;
}

int rt_upsample_fixed(const int64_t *d_sum_lo, int num_samples, const int64_t *d_aov_lo, int aov_samples_lo, int low_width, int low_height,
                      int factor, const int64_t *d_aov_hi, int aov_samples_hi, const rt_upsample_params *params, float *d_rgb_out,
                      int64_t *d_out_fixed, void *stream) {
    return upsample_impl("rt_upsample_fixed: ", false, d_sum_lo, "d_sum_lo", num_samples, d_aov_lo, aov_samples_lo, low_width, low_height, factor,
                         d_aov_hi, aov_samples_hi, params, d_rgb_out, d_out_fixed, (hipStream_t)stream);
}

int rt_upsample_rgb(const float *d_rgb_lo, const int64_t *d_aov_lo, int aov_samples_lo, int low_width, int low_height, int factor,
                    const int64_t *d_aov_hi, int aov_samples_hi, const rt_upsample_params *params, float *d_rgb_out, int64_t *d_out_fixed,
                    void *stream) {
    return upsample_impl("rt_upsample_rgb: ", true, d_rgb_lo, "d_rgb_lo", 1, d_aov_lo, aov_samples_lo, low_width, low_height, factor, d_aov_hi,
                         aov_samples_hi, params, d_rgb_out, d_out_fixed, (hipStream_t)stream);
}

int rt_render_motion(const rt_scene *scene, const rt_camera *camera, int width, int height, const rt_camera *prev_camera,
                     const float *d_prev_tri_p0p1p2, uint32_t flags, float *d_motion, void *stream, rt_stats *stats) {
    return render_motion_impl(scene, camera, width, height, prev_camera, d_prev_tri_p0p1p2, flags, d_motion, (hipStream_t)stream, stats);
}

int rt_temporal_default_params(rt_temporal_params *out) {
    if (!out) return fail("rt_temporal_default_params: null out");
    *out = temporal_defaults();
    return 0;
}

int rt_temporal_accumulate_fixed(const int64_t *d_sum_a, int samples_a, const int64_t *d_sum_b, int samples_b, const int64_t *d_aov_fixed,
                                 int aov_samples, const float *d_motion, const int64_t *d_hist_a_in, const int64_t *d_hist_b_in,
                                 const int32_t *d_len_in, const int64_t *d_prev_aov_fixed, int prev_aov_samples, int width, int height,
                                 const rt_temporal_params *params, int64_t *d_hist_a_out, int64_t *d_hist_b_out, int32_t *d_len_out,
                                 void *stream) {
    // The accumulator with the newer features off, on the instantiation that has them compiled out.  Of temporal_run's checks those
    // this entry point never had cannot fire: the four pointers are null (together, and 16-byte aligned), +inf >= 0 and 1 >= 1; the
    // others are its own, in its order.
    const rt_temporal_params old = params ? *params : temporal_defaults();
    rt_temporal_moments_params prm{};
    prm.max_history = old.max_history;
    prm.alpha_min = old.alpha_min;
    prm.depth_tolerance = old.depth_tolerance;
    prm.normal_cos_min = old.normal_cos_min;
    prm.emission_tolerance = INFINITY;
    prm.variance_min_history = 1;
    prm.flags = old.flags;
    return temporal_run("rt_temporal_accumulate_fixed: ", k_temporal_accumulate, d_sum_a, samples_a, d_sum_b, samples_b, d_aov_fixed, aov_samples,
                        d_motion, d_hist_a_in, d_hist_b_in, d_len_in, d_prev_aov_fixed, prev_aov_samples, nullptr, nullptr, width, height, &prm,
                        d_hist_a_out, d_hist_b_out, d_len_out, nullptr, nullptr, (hipStream_t)stream);
}

int rt_temporal_moments_default_params(rt_temporal_moments_params *out) {
    if (!out) return fail("rt_temporal_moments_default_params: null out");
    *out = temporal_moments_defaults();
    return 0;
}

int rt_temporal_accumulate_moments_fixed(const int64_t *d_sum_a, int samples_a, const int64_t *d_sum_b, int samples_b, const int64_t *d_aov_fixed,
                                         int aov_samples, const float *d_motion, const int64_t *d_hist_a_in, const int64_t *d_hist_b_in,
                                         const int32_t *d_len_in, const int64_t *d_prev_aov_fixed, int prev_aov_samples, const float *d_prev_motion,
                                         const float *d_moments_in, int width, int height, const rt_temporal_moments_params *params,
                                         int64_t *d_hist_a_out, int64_t *d_hist_b_out, int32_t *d_len_out, float *d_moments_out,
                                         float *d_variance_out, void *stream) {
    return temporal_run("rt_temporal_accumulate_moments_fixed: ", k_temporal_accumulate_moments, d_sum_a, samples_a, d_sum_b, samples_b, d_aov_fixed,
                        aov_samples, d_motion, d_hist_a_in, d_hist_b_in, d_len_in, d_prev_aov_fixed, prev_aov_samples, d_prev_motion, d_moments_in,
                        width, height, params, d_hist_a_out, d_hist_b_out, d_len_out, d_moments_out, d_variance_out, (hipStream_t)stream);
}

int rt_denoise_variance_fixed(const int64_t *d_sum_fixed, int num_samples, const float *d_variance, const int64_t *d_aov_fixed, int aov_samples,
                              int width, int height, const rt_denoise_dual_params *params, void *d_scratch, float *d_rgb_out, void *stream) {
    return denoise_variance_impl(d_sum_fixed, num_samples, d_variance, d_aov_fixed, aov_samples, width, height, params, d_scratch, d_rgb_out,
                                 (hipStream_t)stream);
}

int rt_post_process(float *d_rgb, int num_pixels, int num_samples, void *stream) {
    if (!d_rgb || num_pixels <= 0 || num_samples <= 0) return fail("rt_post_process: bad argument");
    if (num_pixels > 0x7fffffff / 3) return fail("rt_post_process: more than 715827882 pixels");
    return post_process_impl(nullptr, d_rgb, num_pixels, num_samples, (hipStream_t)stream);
}

int rt_render(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples,
              int max_bounces, uint64_t seed, uint32_t flags, float *out_rgb, rt_stats *stats) {
    return render_impl(scene, camera, width, height, num_samples, max_bounces, seed, flags, out_rgb, stats);
}

void rt_shutdown(void) { shutdown_impl(); }

int rt_render_multi(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples,
                    int max_bounces, uint64_t seed, uint32_t flags, const int *devices, int n_devices, float *out_rgb,
                    rt_stats *stats) {
    return render_multi_impl(scene, camera, width, height, num_samples, max_bounces, seed, flags, devices, n_devices, out_rgb, stats);
}

int rt_trace_closest(const rt_scene *scene, int n, const float *origin_xyz, const float *dir_xyz, const float *tmax,
                     int32_t *hit_tri, float *t, float *u, float *v) {
    return trace_closest_impl(scene, 0u, n, origin_xyz, dir_xyz, tmax, hit_tri, t, u, v);
}

int rt_trace_closest_flags(const rt_scene *scene, uint32_t flags, int n, const float *origin_xyz, const float *dir_xyz,
                           const float *tmax, int32_t *hit_tri, float *t, float *u, float *v) {
    return trace_closest_impl(scene, flags, n, origin_xyz, dir_xyz, tmax, hit_tri, t, u, v);
}

int rt_trace_any(const rt_scene *scene, int n, const float *origin_xyz, const float *dir_xyz, const float *tmax,
                 const int32_t *excluded_tri, int32_t *occluded) {
    return trace_any_impl(scene, 0u, n, origin_xyz, dir_xyz, tmax, excluded_tri, occluded);
}

int rt_trace_any_flags(const rt_scene *scene, uint32_t flags, int n, const float *origin_xyz, const float *dir_xyz,
                       const float *tmax, const int32_t *excluded_tri, int32_t *occluded) {
    return trace_any_impl(scene, flags, n, origin_xyz, dir_xyz, tmax, excluded_tri, occluded);
}

int rt_query_closest_device(const rt_scene *scene, uint32_t flags, int n, const float *d_origin_xyz, const float *d_dir_xyz,
                            const float *d_tmax, int32_t *d_hit_tri, float *d_t, float *d_u, float *d_v, void *stream) {
    return query_impl<Q_CLOSEST>(scene, flags, n, d_origin_xyz, d_dir_xyz, d_tmax, nullptr, d_hit_tri, d_t, d_u, d_v, (hipStream_t)stream);
}

int rt_query_any_device(const rt_scene *scene, uint32_t flags, int n, const float *d_origin_xyz, const float *d_dir_xyz,
                        const float *d_tmax, const int32_t *d_excluded_tri, int32_t *d_occluded, void *stream) {
    return query_impl<Q_ANY>(scene, flags, n, d_origin_xyz, d_dir_xyz, d_tmax, d_excluded_tri, d_occluded, nullptr, nullptr, nullptr,
                             (hipStream_t)stream);
}

int rt_query_last_counters(const rt_scene *scene, int64_t out[3]) {
    if (!scene || !out) return fail("rt_query_last_counters: null argument");
    std::lock_guard<std::mutex> lock(scene->query.mutex);
    for (int k = 0; k < 3; k++) out[k] = scene->query.counters[k];
    return 0;
}

int rt_xorwow_states(uint64_t seed, uint32_t first, uint32_t count, int draws, uint32_t *state6, float *uniforms) {
    if (count == 0) return 0;
    if (!state6 || draws < 0 || (draws > 0 && !uniforms)) return fail("rt_xorwow_states: bad argument");
    if ((uint64_t)first + count > (uint64_t)kW) return fail("rt_xorwow_states: subsequence range exceeds W");
    DPools p{};
    uint32_t *buf = nullptr, *d_state = nullptr, *d_jump = nullptr;
    float *d_uni = nullptr;
    DevScope tmp;
    if (tmp.alloc(buf, 6 * (size_t)count) || tmp.alloc(d_state, 6 * (size_t)count) || tmp.alloc(d_uni, (size_t)count * draws) ||
        tmp.alloc(d_jump, (size_t)20 * 800))
        return 1;
    p.n = (int)count;  // only the six RNG arrays are touched: place array A_RD at buf
    p.base = (float *)buf - (size_t)A_RD * count;
    HIP_TRY(hipMemcpy(d_jump, jump_powers().data(), sizeof(uint32_t) * 20 * 800, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_rng_init, dim3(grid_for((int)count)), dim3(kBlock), 0, nullptr, p, (int)count, (int)first,
                       xorwow_seed(seed), d_jump);
    hipLaunchKernelGGL(k_test_draw, dim3(grid_for((int)count)), dim3(kBlock), 0, nullptr, p, (int)count, draws, d_state,
                       d_uni);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(state6, d_state, sizeof(uint32_t) * 6 * (size_t)count, hipMemcpyDeviceToHost));
    if (draws > 0) HIP_TRY(hipMemcpy(uniforms, d_uni, sizeof(float) * (size_t)count * draws, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
