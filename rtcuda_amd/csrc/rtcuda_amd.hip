// rtcuda_amd.hip -- HIP kernels and the C-ABI of the MI355X-native render path (gfx950 only).
// The root of the one translation unit: kernels and C-ABI; the host side between them is rt_host_scene.inc + rt_host_render.inc.
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
//                generation, by the stage-level test entry points, and (RT_PERSISTENT=0) for whole frames.
//   advance_core / inner_step / tri_intersect / box_hit are the shared device functions: one copy of
//   the estimator and of the traversal for both pipelines.
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
#include "rt_bvh.h"
#include "rt_device.h"
#include "rt_launch_plan.h"
#include "rt_ploc.h"
#include "rt_ref_tree.h"

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
};

constexpr int kLdsTable = 64;                   // materials / lights staged in LDS per workgroup
constexpr int kTabDwordsMax = kLdsTable * 29;   // 5 + 8 + 12 + 4 dwords per (material, light)

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
// Travels in k_paths_keyed's uniforms where the camera builds keep the Camera: no larger than it.
struct KeyedRayTable {
    const float *o3, *d3;  // origins and directions, AoS triples
    const int *pixel;      // the pixel a ray deposits into; null: K / rays_per_pixel
    unsigned long long key_first;
    uint32_t key_stride, rays_per_pixel;
    int pix_first;
    uint32_t rem_first;
};
static_assert(sizeof(KeyedRayTable) <= sizeof(Camera), "k_paths' dynamic LDS is sized for a Camera in the uniforms");
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
template <bool NEVER_LOCKSTEP = false, class SRC>
__device__ __forceinline__ void gen_core(const SRC &cam, const AdvanceParams &ap, int slot_global, SlotState &st,
                                         AdvanceOut &out, int *pxy = nullptr, long long cid_given = -1) {
    const bool lockstep = NEVER_LOCKSTEP ? false : (ap.lockstep != 0);
    long long cid = cid_given >= 0 ? cid_given : (long long)st.gen * kW + slot_global;
    if (cid >= ap.cam_end) {
        st.bounces = kDone;
        return;
    }
    if (!lockstep && st.gen == ap.last_gen) {
        st.bounces = kParked;
        return;
    }
    st.gen = st.gen + 1;
    if constexpr (std::is_same<SRC, KeyedRayTable>::value) {
        // Keyed ray-table frames: row `cid` starts the per-sample stream of its key (whatever stream the lane held), gen()'s
        // two jitter draws are made and dropped -- a pinhole's own table reproduces the RT_FLAG_RNG_PER_SAMPLE frame draw for
        // draw --, the ray is the row.  Rows are read as in the RayTable branch below: the lanes of a wave hold consecutive
        // ranks of a drawn chunk (or consecutive slots), so consecutive rows.
        const unsigned c = (unsigned)cid;  // (below 2^31: the host checks the frame)
        const unsigned long long ck = (unsigned long long)c * cam.key_stride;  // (no wrap: c < 2^31, key_stride < 2^32)
        st.rs = rng_sample_stream(ap.seed_lo, ap.seed_hi, cam.key_first + ck);  // (the host refuses keys that wrap)
        rng_next(st.rs);  // x first, then y (Appendix A.7)
        rng_next(st.rs);
        const float *o3 = cam.o3 + 3 * (size_t)c, *d3 = cam.d3 + 3 * (size_t)c;
        out.ray_o = mk(table_load(o3), table_load(o3 + 1), table_load(o3 + 2));
        out.ray_d = mk(table_load(d3), table_load(d3 + 1), table_load(d3 + 2));
        if (cam.pixel) {
            st.pixel = table_load(cam.pixel + c);
        } else {
            const unsigned long long t = cam.rem_first + ck;  // K / rays_per_pixel = pix_first + t / rays_per_pixel
            const unsigned q = (t >> 32) ? (unsigned)(t / cam.rays_per_pixel) : (unsigned)t / cam.rays_per_pixel;
            st.pixel = cam.pix_first + (int)q;  // (below n_pixels: the host checks the last key)
        }
        out.new_ray = true;
        st.bounces = 0;
        st.beta = mk(1.f, 1.f, 1.f);
        out.did_gen = true;
        return;
    } else if constexpr (std::is_same<SRC, RayTable>::value) {
        // Ray-table frames: gen()'s two jitter draws are made and dropped (the slot's stream stays where the reference's
        // is), the ray and its pixel are row `cid` of the table.  No pixel coordinates, no stepping (`pxy` is left alone).
        // The lanes of a wave serve consecutive slots, so their rows are consecutive: 768 contiguous bytes per array and
        // wave, read once per frame -- streamed past the caches the BVH lives in (RT_RAYS_NONTEMPORAL).
        const unsigned c = (unsigned)cid;  // (below 2^31: the host checks the frame)
        rng_next(st.rs);  // x first, then y (Appendix A.7)
        rng_next(st.rs);
        const float *o3 = cam.o3 + 3 * (size_t)c, *d3 = cam.d3 + 3 * (size_t)c;
        out.ray_o = mk(table_load(o3), table_load(o3 + 1), table_load(o3 + 2));
        out.ray_d = mk(table_load(d3), table_load(d3 + 1), table_load(d3 + 2));
        st.pixel = cam.pixel ? table_load(cam.pixel + c) : (int)(c / (unsigned)ap.spp);  // (render.cuh:254-256)
        out.new_ray = true;
        st.bounces = 0;
        st.beta = mk(1.f, 1.f, 1.f);
        out.did_gen = true;
        return;
    } else {
    // pixel = camera_ray_id / spp (render.cuh:254-256).  cid = gen * W + slot, so when spp divides W the quotient
    // splits exactly into two 32-bit terms; the general case keeps the 64-bit division.
    int px, py;
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
    if (ap.per_sample) st.rs = rng_sample_stream(ap.seed_lo, ap.seed_hi, (unsigned long long)cid * (unsigned)ap.key_mul + (unsigned)ap.key_add);
    float jx = rng_uniform(st.rs);  // x first, then y (Appendix A.7)
    float jy = rng_uniform(st.rs);
    camera_get_ray(cam, (px + jx) / ap.width, (py + jy) / ap.height, out.ray_o, out.ray_d);
    out.new_ray = true;
    st.bounces = 0;
    st.beta = mk(1.f, 1.f, 1.f);
    out.did_gen = true;
    }
}

// `acc` (USE_ACC, k_paths only): the lane's sample accumulator; otherwise contributions go straight into the framebuffer.
template <bool DEFER_GEN, bool NEVER_LOCKSTEP = false, bool USE_ACC = false, class SRC>
__device__ __forceinline__ void advance_core(const DScene &sc, const float *tab, const SRC &cam,
                                             const AdvanceParams &ap, int slot_global, SlotState &st, AdvanceOut &out,
                                             float *__restrict__ fb, float *acc = nullptr) {
    const bool lockstep = NEVER_LOCKSTEP ? false : (ap.lockstep != 0);
    const int off_ltri = tab_off_ltri(sc.num_mats, sc.num_lights);
    const int off_lpre = tab_off_lpre(sc.num_mats, sc.num_lights);
    out.did_gen = out.did_shade = out.has_shadow = out.did_emit = out.new_ray = out.wants_gen = false;
    out.rr_draws = 0;
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
            const float pt = fmaxf(0.05f, 1 - max3(st.beta));
            shade = false;
            while (true) {
                out.rr_draws++;
                const bool kill = rng_uniform(st.rs) < pt;
                st.bounces = st.bounces + 1;  // :126
                if (!kill) {
                    st.beta = divf(st.beta, 1 - pt);
                    shade = true;
                    break;
                }
                if (lockstep || !(st.bounces < ap.max_bounces)) break;
            }
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
        gen_core<NEVER_LOCKSTEP>(cam, ap, slot_global, st, out);
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

// ============================================================================ traversal
// One wave-wide traversal engine serves the four trace entry points (closest-hit over the path
// pools = ch(), render.cuh:297-328; any-hit over the shadow queue = ah(), :278-294; and the two
// stage-level test hooks), so the parity tests exercise exactly the code the renderer runs.
//
// Structure (wave64, persistent):
//   * every wave owns 64 lanes = 64 rays in flight and keeps pulling ray indices from a global
//     head counter in chunks of kChunk (one atomic per 256 rays); finished lanes are finalised and
//     re-filled together once fewer than kRefillAt lanes are still traversing, so the wave does not
//     idle on its longest ray;
//   * "while-while": all lanes first step through inner pair records until each holds a leaf (or
//     is finished), then all lanes test their leaf's triangles -- node steps run beside node steps
//     and triangle tests beside triangle tests instead of serialising per lane;
//   * the traversal stack is a column of LDS per lane (replaces device_stack.cuh's int[29] in
//     scratch memory); entries are inner pair indices (>= 0) or leaf references (< 0).
//
// The box test only culls: it is conservative (boxes padded by the builder, exit distance widened
// by 8 ulp) and may use any arithmetic.  The triangle test is the reference's, bit for bit.
struct RayPrep {
    V3 o, d, inv;
};
__device__ __forceinline__ V3 inv_dir(V3 d) {
    // aabb_intersector.cuh:17-19 clamps |d| away from 0 the same way before inverting.  The reciprocal itself is the
    // hardware's v_rcp_f32 (1 ulp) rather than an IEEE division (11 instructions each, three per ray): 1 / d only feeds
    // the box test, which only culls -- box_hit / inner_step widen the exit distance by 8 ulps, which covers the 1 ulp
    // per axis this costs on top of the rounding of the slab arithmetic (the builder pads every box by 2 ulps)
    float ix = __builtin_amdgcn_rcpf((fabsf(d.x) < kFltEps) ? copysignf(kFltEps, d.x) : d.x);
    float iy = __builtin_amdgcn_rcpf((fabsf(d.y) < kFltEps) ? copysignf(kFltEps, d.y) : d.y);
    float iz = __builtin_amdgcn_rcpf((fabsf(d.z) < kFltEps) ? copysignf(kFltEps, d.z) : d.z);
    return mk(ix, iy, iz);
}
__device__ __forceinline__ bool box_hit(V3 o, V3 inv, float lox, float loy, float loz, float hix, float hiy,
                                        float hiz, float tmax, float &entry) {
    float ax = (lox - o.x) * inv.x, bx = (hix - o.x) * inv.x;
    float ay = (loy - o.y) * inv.y, by = (hiy - o.y) * inv.y;
    float az = (loz - o.z) * inv.z, bz = (hiz - o.z) * inv.z;
    float t_in = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
    float t_out = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
    entry = t_in;
    t_out = t_out * 1.000001f;
    return t_in <= t_out && t_out >= 0.f && t_in <= tmax * 1.000001f;  // (tmax widened like t_out: see inner_step)
}

typedef float v2f __attribute__((ext_vector_type(2)));  // packed fp32 (v_pk_*_f32 on gfx950)
constexpr int kEntryDone = (int)0x80000000;  // "nothing left to visit" marker for a lane (== rtbvh::kNoChild)
// Traversal stack: the first `cap` entries of a lane live in its LDS column, deeper ones (rare: the
// bound is 3 per tree level, the typical depth under 10) in a per-lane column of a global overflow
// buffer, so LDS use -- and with it occupancy -- is set by the common case, not the worst case.
__device__ __forceinline__ void stack_push(int *lds_col, int *over_col, int &sp, int cap, int v) {
    if (sp < cap) lds_col[sp * kBlock] = v;
    else over_col[(size_t)(sp - cap) * kOverStride] = v;
    sp++;
}
// Pushes without divergent branches: a value is ALWAYS stored one above the current top of the LDS part and the stack
// pointer moves only if the push is meant (what lies above the top is never read).  The LDS part has one row more than
// `cap` (callers allocate cap + 1 rows), which takes the stores of lanes whose LDS part is full; only such lanes,
// rarely, branch -- once per node step -- to the global overflow column.  Written as `if (push) ...`, each of the up
// to 3 pushes of a 4-wide node step cost an exec-mask save / restore pair, two jumps and a 64-bit overflow address:
// a third of the instructions of the step.
__device__ __forceinline__ void push_if(int *lds_col, int *over_col, int &sp, int cap, int v, bool push) {
    lds_col[min(sp, cap) * kBlock] = v;
    if (push && sp >= cap) {
        over_col[(size_t)(sp - cap) * kOverStride] = v;
        __asm__ volatile("" ::: "memory");
    }
    sp += push ? 1 : 0;
}
__device__ __forceinline__ void push_if4(int *lds_col, int *over_col, int &sp, int cap, int v0, bool p0, int v1, bool p1,
                                         int v2, bool p2, int v3, bool p3) {
    const int s0 = sp, s1 = s0 + (p0 ? 1 : 0), s2 = s1 + (p1 ? 1 : 0), s3 = s2 + (p2 ? 1 : 0), s4 = s3 + (p3 ? 1 : 0);
    lds_col[min(s0, cap) * kBlock] = v0;
    lds_col[min(s1, cap) * kBlock] = v1;
    lds_col[min(s2, cap) * kBlock] = v2;
    lds_col[min(s3, cap) * kBlock] = v3;
    if (s4 > cap) {  // rare: some of this lane's pushes belong in the overflow column
        if (p0 && s0 >= cap) over_col[(size_t)(s0 - cap) * kOverStride] = v0;
        if (p1 && s1 >= cap) over_col[(size_t)(s1 - cap) * kOverStride] = v1;
        if (p2 && s2 >= cap) over_col[(size_t)(s2 - cap) * kOverStride] = v2;
        if (p3 && s3 >= cap) over_col[(size_t)(s3 - cap) * kOverStride] = v3;
        __asm__ volatile("" ::: "memory");
    }
    sp = s4;
}
__device__ __forceinline__ int stack_pop(int *lds_col, int *over_col, int &sp, int cap) {
    sp--;
    // always read the LDS column (clamped) and patch from the overflow only when needed: written as a
    // select of two pointers, the compiler merges the paths into one FLAT load, which is slower
    int v = lds_col[min(sp, cap - 1) * kBlock];
    if (sp >= cap) {
        v = over_col[(size_t)(sp - cap) * kOverStride];
        __asm__ volatile("" ::: "memory");  // keeps this a branch: merged, the two loads become one FLAT load behind
                                            // a dozen instructions of 64-bit address selection, on every pop
    }
    return v;
}
// Closest hit among EQUAL distances.  The reference accepts `t <= tmax` (triangle.cuh:49), so of two triangles hit at
// exactly the same t (a shared edge) the one its BVH walk tests LAST wins -- a property of the
// reference's tree that no other tree can reproduce.  Here the tie goes to the triangle with the larger index in the
// CALLER's order, whatever the tree: the result is a function of the ray and the triangle list alone (the oracle's
// watertight mode applies the same rule; ties are ~1 in 10^7 rays).  `tri` / `tmax`: best hit so far.
__device__ __forceinline__ bool closest_hit_wins(const DScene &sc, float t, float tmax, int k, int tri) {
    if (t == tmax && tri >= 0) return sc.order[(unsigned)k] > sc.order[(unsigned)tri];
    return true;
}
constexpr int kRefillAt = 40;                // finalise + refill once <= this many lanes still traverse
__device__ __forceinline__ int leaf_ref(int first, int count) { return ~((first << 3) | count); }

// One node step of a lane whose current entry is an inner record (cur >= 0): test the children,
// continue with the nearest one that the ray may enter, push the others (far first).
// `top` / `top_n`: the first top_n records (the top of the tree, breadth-first: rt_bvh.h) may be staged
// in LDS by the caller; nullptr / 0 otherwise.
// SHALLOW (4-wide nodes, k_paths): the caller has established -- with one wave vote -- that every lane taking this step has at
// most stack_cap - 3 entries, so neither the pop nor the up to three pushes of the step can leave the LDS part of the stack:
// no clamps, no overflow branches (each of which costs the wave an exec-mask save / restore pair and a jump whether or not a
// lane takes it; the general step has four such rare regions).  95 % of the node steps of C2 qualify at stack_cap = 10.
template <bool WIDE, bool SHALLOW = false>
__device__ __forceinline__ void inner_step(const DScene &sc, V3 o, V3 inv, float tmax, int &cur, int &sp, int *stack,
                                           int *over, int stack_cap, const float4 *top = nullptr, int top_n = 0) {
    // (2-wide records) the top of the LDS part of the stack, in case this step ends in a pop: see below
    const int spec_top = SHALLOW ? stack[max(sp - 1, 0) * kBlock] : stack[max(min(sp - 1, stack_cap - 1), 0) * kBlock];
    // 2-wide: one 64-byte record, q0..q3.  4-wide: the node's 128 bytes are laid out BY PLANE (k_refit_emit): per axis a
    // 16-byte word with the four children's lower bounds and one with their upper bounds, then the four links.  Which of the two
    // is the NEAR plane of an axis depends on the sign of 1 / d alone, so each lane fetches near and far planes by address
    // (word index 2 * axis + sign, and the other one) and the slab test needs no min / max per axis: 24 instructions fewer per
    // node step than sorting each pair of distances.  n*: near planes, f*: far planes, q3: links.
    float4 q0, q1, q2, q3, nx, ny, nz, fx, fy, fz;
    if (WIDE) {
        const unsigned bx = (__float_as_uint(inv.x) >> 27) & 16u, by = (__float_as_uint(inv.y) >> 27) & 16u,
                       bz = (__float_as_uint(inv.z) >> 27) & 16u;  // 16 where 1 / d is negative: the upper bound is the near one
        if (top_n > 0 && cur < top_n) {
            const char *q = (const char *)(top + 4 * cur);
            nx = *(const float4 *)(q + bx);
            fx = *(const float4 *)(q + (bx ^ 16u));
            ny = *(const float4 *)(q + 32 + by);
            fy = *(const float4 *)(q + 32 + (by ^ 16u));
            nz = *(const float4 *)(q + 64 + bz);
            fz = *(const float4 *)(q + 64 + (bz ^ 16u));
            q3 = *(const float4 *)(q + 96);
            __asm__ volatile("" ::: "memory");  // (keeps the two branches apart: see below)
        } else {
            const char *q = (const char *)sc.nodes;
            const unsigned base = (unsigned)cur << 6;
            nx = *(const float4 *)(q + (base | bx));
            fx = *(const float4 *)(q + ((base | bx) ^ 16u));
            ny = *(const float4 *)(q + ((base | by) + 32u));
            fy = *(const float4 *)(q + (((base | by) ^ 16u) + 32u));
            nz = *(const float4 *)(q + ((base | bz) + 64u));
            fz = *(const float4 *)(q + (((base | bz) ^ 16u) + 64u));
            q3 = *(const float4 *)(q + (base + 96u));
        }
        q0 = q1 = q2 = q3;  // (unused in this form)
    } else if (top_n > 0 && cur < top_n) {
        const float4 *q = top + 4 * cur;
        q0 = q[0];
        q1 = q[1];
        q2 = q[2];
        q3 = q[3];
        // keeps the two branches apart: merged into a select of pointers they become FLAT loads, which go
        // through the texture addresser like any global load and make the LDS copy pointless
        __asm__ volatile("" ::: "memory");
        nx = ny = nz = fx = fy = fz = q0;
    } else {
        const float4 *q = (const float4 *)((const char *)sc.nodes + ((unsigned)cur << 6));
        q0 = q[0];
        q1 = q[1];
        q2 = q[2];
        q3 = q[3];
        nx = ny = nz = fx = fy = fz = q0;
    }
    if (!WIDE) {
        // 2-wide record: two exact boxes, near child first, far child onto the stack.  The bounds of the two
        // children are interleaved (rt_scene_create), so the 12 subtractions and 12 multiplications of the
        // slab test are 6 + 6 packed operations; each component is rounded exactly as in box_hit.
        int cl = __float_as_int(q3.x), cr = __float_as_int(q3.y);
        const v2f ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z};
        const v2f ix = {inv.x, inv.x}, iy = {inv.y, inv.y}, iz = {inv.z, inv.z};
        v2f ax = v2f{q0.x, q0.y} - ox, ay = v2f{q0.z, q0.w} - oy, az = v2f{q1.x, q1.y} - oz;
        v2f bx = v2f{q1.z, q1.w} - ox, by = v2f{q2.x, q2.y} - oy, bz = v2f{q2.z, q2.w} - oz;
        ax = ax * ix; ay = ay * iy; az = az * iz;
        bx = bx * ix; by = by * iy; bz = bz * iz;
        const float el = fmaxf(fmaxf(fminf(ax.x, bx.x), fminf(ay.x, by.x)), fminf(az.x, bz.x));
        const float er = fmaxf(fmaxf(fminf(ax.y, bx.y), fminf(ay.y, by.y)), fminf(az.y, bz.y));
        v2f t_out = {fminf(fminf(fmaxf(ax.x, bx.x), fmaxf(ay.x, by.x)), fmaxf(az.x, bz.x)),
                     fminf(fminf(fmaxf(ax.y, bx.y), fmaxf(ay.y, by.y)), fmaxf(az.y, bz.y))};
        t_out = t_out * v2f{1.000001f, 1.000001f};
        // (tmax is widened like the exit distance: the entry distance carries the same few ulps of rounding, and a
        // shadow ray that ends ON a triangle coplanar with an occluder -- light quads -- has entry = t = tmax to the
        // last bit; unwidened, the full-size audit of the sixteen-light scene lost 1 occluder in 9.8e8 shadow rays)
        const float tmax_w = tmax * 1.000001f;
        bool hl = el <= t_out.x && t_out.x >= 0.f && el <= tmax_w && cl != kEntryDone;
        bool hr = er <= t_out.y && t_out.y >= 0.f && er <= tmax_w && cr != kEntryDone;
        // What comes next, with as little divergent control flow as the three outcomes allow (every divergent branch
        // costs the wave an exec-mask save / restore pair and a jump, a dozen scalar instructions per step before):
        //   one child entered  -> it becomes the cursor;
        //   both               -> the nearer one, the farther one onto the stack (the only branch left, a single store);
        //   none               -> the top of the stack, read speculatively BEFORE the slab arithmetic (`spec_top`), so
        //                         that the LDS latency of a pop is never on the critical path of a step.
        const bool both = hl && hr, none = !(hl || hr);
        const bool left_first = !(el > er);
        int popped = sp > 0 ? spec_top : kEntryDone;
        if (none && sp > stack_cap) {  // rare: the entry lives in the global overflow part
            popped = over[(size_t)(sp - 1 - stack_cap) * kOverStride];
            __asm__ volatile("" ::: "memory");
        }
        const int entered = (hl && (!hr || left_first)) ? cl : cr;
        cur = none ? popped : entered;
        sp -= (none && sp > 0) ? 1 : 0;
        push_if(stack, over, sp, stack_cap, left_first ? cr : cl, both);
    }
    if (WIDE) {
        // 4-wide node = two pair-style records (children 0, 1 | children 2, 3) with full-precision boxes: half the
        // dependent fetches of the 2-wide walk for the same box arithmetic.  The nearest child the ray may enter becomes
        // the cursor, the others go onto the stack in record order (measured on the CPU walk: sorting them as well
        // saves 0.3 % of the steps), nothing entered -> the speculative top of the stack.
        const int c0 = __float_as_int(q3.x), c1 = __float_as_int(q3.y), c2 = __float_as_int(q3.z), c3 = __float_as_int(q3.w);
        const v2f ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z};
        const v2f ix = {inv.x, inv.x}, iy = {inv.y, inv.y}, iz = {inv.z, inv.z};
        // (clamped to a finite value: an absent child has an all-+inf box -- rt_bvh.h -- whose entry distance is +inf or
        // whose exit distance is -inf whatever the ray, so the one comparison below rejects it without a look at its link)
        const float tmax_w = fminf(tmax * 1.000001f, kFltMax);
        float e[4];
        bool h[4];
        // entered <=> entry <= exit, exit >= 0, entry <= tmax: max(entry, 0) <= min(exit, tmax) -- one comparison per child
        // instead of three and their scalar ANDs (tmax >= 0 always)
        // plane distance = b * (1 / d) + s, s = -o * (1 / d): ONE packed fma per pair of planes where (b - o) * (1 / d) takes
        // two instructions.  s is rounded on its own, which moves the planes of an axis by up to 2^-24 |o| as the ray sees
        // them: the records are padded for that (k_refit_emit, rt_bvh.h pad_quads_for_origins; ensure_origin_radius).
        // Near and far planes were picked by the sign of 1 / d when they were fetched: monotone rounding makes the near
        // plane's distance the smaller of the two, the very value min() would pick.
        const v2f sx = {-o.x * inv.x, -o.x * inv.x}, sy = {-o.y * inv.y, -o.y * inv.y}, sz = {-o.z * inv.z, -o.z * inv.z};
        (void)ox; (void)oy; (void)oz; (void)q0; (void)q1; (void)q2;
#define RT_SLAB(b, i, s_) __builtin_elementwise_fma((b), (i), (s_))
        {
            const v2f tnx = RT_SLAB((v2f{nx.x, nx.y}), ix, sx), tny = RT_SLAB((v2f{ny.x, ny.y}), iy, sy), tnz = RT_SLAB((v2f{nz.x, nz.y}), iz, sz);
            const v2f tfx = RT_SLAB((v2f{fx.x, fx.y}), ix, sx), tfy = RT_SLAB((v2f{fy.x, fy.y}), iy, sy), tfz = RT_SLAB((v2f{fz.x, fz.y}), iz, sz);
            e[0] = fmaxf(fmaxf(tnx.x, tny.x), tnz.x);
            e[1] = fmaxf(fmaxf(tnx.y, tny.y), tnz.y);
            v2f t_out = {fminf(fminf(tfx.x, tfy.x), tfz.x), fminf(fminf(tfx.y, tfy.y), tfz.y)};
            t_out = t_out * v2f{1.000001f, 1.000001f};
            h[0] = fmaxf(e[0], 0.f) <= fminf(t_out.x, tmax_w);
            h[1] = fmaxf(e[1], 0.f) <= fminf(t_out.y, tmax_w);
        }
        {
            const v2f tnx = RT_SLAB((v2f{nx.z, nx.w}), ix, sx), tny = RT_SLAB((v2f{ny.z, ny.w}), iy, sy), tnz = RT_SLAB((v2f{nz.z, nz.w}), iz, sz);
            const v2f tfx = RT_SLAB((v2f{fx.z, fx.w}), ix, sx), tfy = RT_SLAB((v2f{fy.z, fy.w}), iy, sy), tfz = RT_SLAB((v2f{fz.z, fz.w}), iz, sz);
            e[2] = fmaxf(fmaxf(tnx.x, tny.x), tnz.x);
            e[3] = fmaxf(fmaxf(tnx.y, tny.y), tnz.y);
            v2f t_out = {fminf(fminf(tfx.x, tfy.x), tfz.x), fminf(fminf(tfx.y, tfy.y), tfz.y)};
            t_out = t_out * v2f{1.000001f, 1.000001f};
            h[2] = fmaxf(e[2], 0.f) <= fminf(t_out.x, tmax_w);
            h[3] = fmaxf(e[3], 0.f) <= fminf(t_out.y, tmax_w);
        }
#undef RT_SLAB
        // nearest entered child (a child that is not entered counts as infinitely far)
        const float f0 = h[0] ? e[0] : kFltMax, f1 = h[1] ? e[1] : kFltMax, f2 = h[2] ? e[2] : kFltMax, f3 = h[3] ? e[3] : kFltMax;
        const bool a01 = !(f0 > f1), a23 = !(f2 > f3);       // winner of each record (ties: the lower index)
        const float g01 = a01 ? f0 : f1, g23 = a23 ? f2 : f3;
        const bool first = !(g01 > g23);
        const int near_k = first ? (a01 ? 0 : 1) : (a23 ? 2 : 3);
        const int near_link = first ? (a01 ? c0 : c1) : (a23 ? c2 : c3);
        const bool any_hit = h[0] || h[1] || h[2] || h[3];
        int spec = spec_top;
        __asm__ volatile("" : "+v"(spec));  // the read stays where it was issued: the compiler otherwise sinks it into a branch
        int popped = sp > 0 ? spec : kEntryDone;
        if (!SHALLOW && !any_hit && sp > stack_cap) {
            popped = over[(size_t)(sp - 1 - stack_cap) * kOverStride];
            __asm__ volatile("" ::: "memory");
        }
        cur = any_hit ? near_link : popped;
        sp -= (!any_hit && sp > 0) ? 1 : 0;
        if (SHALLOW) {  // (every value is stored one above the running top; the top moves only if the push is meant)
            const bool p0 = h[0] && near_k != 0, p1 = h[1] && near_k != 1, p2 = h[2] && near_k != 2, p3 = h[3] && near_k != 3;
            const int s0 = sp, s1 = s0 + (p0 ? 1 : 0), s2 = s1 + (p1 ? 1 : 0), s3 = s2 + (p2 ? 1 : 0);
            stack[s0 * kBlock] = c0;
            stack[s1 * kBlock] = c1;
            stack[s2 * kBlock] = c2;
            stack[s3 * kBlock] = c3;
            sp = s3 + (p3 ? 1 : 0);
        } else {
            push_if4(stack, over, sp, stack_cap, c0, h[0] && near_k != 0, c1, h[1] && near_k != 1, c2, h[2] && near_k != 2, c3,
                     h[3] && near_k != 3);
        }
    }
}

// ============================================================================ RT_FLAG_REFERENCE_WALK
// The reference's own traversal over its own tree (rt_ref_tree.h), decision for decision -- opt-in, never timed:
//   * AABBIntersector (aabb_intersector.cuh:14-36): octant from the sign of d, 1 / d as an IEEE division with |d|
//     clamped away from 0, scaled origin (-o) * (1 / d); per slab inv * bound + scaled_origin as a separately rounded
//     multiplication and addition (this file is built with -ffp-contract=off); hit iff entry <= exit -- on the exact,
//     unpadded boxes, with no clamp to [0, tmax].  This is the test that loses about one accepted hit in 10^7 rays;
//   * Bvh::traverse (bvh.cuh:251-303 / :306-357): the two children of a node are tested left then right, a leaf
//     child is intersected on the spot (left leaf before right leaf), of two inner children the one with the smaller
//     entry distance is descended first (ties: the left one) and the other one's children index is pushed;
//   * intersect_leaf (:222-236 / :239-248): triangles in the reference's primitive order; closest hit accepts
//     t <= tmax, so the LATER tested of two hits at equal t wins (triangle.cuh:49); any hit returns at the first
//     accepted triangle that is not the excluded one.
// A lane runs its whole ray here in one go (a plain per-lane loop with a private stack of 32 entries -- the
// reference's DeviceStack has 29, device_stack.cuh:4-11, for a tree of depth <= 30): no speculation, no reordering.
// `tri`: best hit so far / excluded triangle, as everywhere else (leaf-order index); ANY sets hu = 1 when occluded.
struct RefSlab {
    bool nx, ny, nz;  // octant: direction component negative
    V3 inv, so;
};
__device__ inline RefSlab ref_slab(V3 o, V3 d) {
    RefSlab s;
    s.nx = d.x < 0;
    s.ny = d.y < 0;
    s.nz = d.z < 0;
    s.inv = mk(1.f / ((fabsf(d.x) < kFltEps) ? copysignf(kFltEps, d.x) : d.x),
               1.f / ((fabsf(d.y) < kFltEps) ? copysignf(kFltEps, d.y) : d.y),
               1.f / ((fabsf(d.z) < kFltEps) ? copysignf(kFltEps, d.z) : d.z));
    s.so = mul(neg(o), s.inv);
    return s;
}
// node = {xmin, xmax, ymin, ymax | zmin, zmax, count, link}
__device__ inline bool ref_box(const RefSlab &s, float4 n0, float4 n1, float &entry) {
    const float ex = s.inv.x * (s.nx ? n0.y : n0.x) + s.so.x;
    const float ey = s.inv.y * (s.ny ? n0.w : n0.z) + s.so.y;
    const float ez = s.inv.z * (s.nz ? n1.y : n1.x) + s.so.z;
    entry = fmaxf(ex, fmaxf(ey, ez));
    const float xx = s.inv.x * (s.nx ? n0.x : n0.y) + s.so.x;
    const float xy = s.inv.y * (s.ny ? n0.z : n0.w) + s.so.y;
    const float xz = s.inv.z * (s.nz ? n1.x : n1.y) + s.so.z;
    const float exit = fminf(xx, fminf(xy, xz));
    return entry <= exit;
}
// `stack` / `over` / `cap`: the lane's own traversal stack (LDS column + global overflow column, stack_push / stack_pop) --
// free whenever this runs, since the lane's ray through the product's tree has ended or never started.  (Round 4 kept 32
// entries in a private array: the compiler promoted it to 32 VGPRs indexed through select chains -- 227 VGPRs unconstrained,
// 53 spilled at the 4-wave budget.)
template <bool ANY>
__device__ inline void reference_walk(const DScene &sc, V3 o, V3 d, float &tmax, int &tri, float &hu, float &hv, int *stack,
                                      int *over, int cap) {
    if (sc.ref_n_prims <= 0) return;
    const float4 *__restrict__ nodes = sc.ref_nodes;
    // true: the ray is finished (an occluder was found)
    auto leaf = [&](int first, int count) -> bool {
#pragma nounroll
        for (int i = first; i < first + count; i++) {
            const int k = sc.ref_prims[i];
            const Tri tr = load_tri(sc.tris, k);
            float t, u, v;
            if (tri_intersect(tr, o, d, tmax, t, u, v)) {
                if (ANY) {
                    if (k != tri) {
                        hu = 1.f;
                        return true;
                    }
                } else {
                    tmax = t;
                    hu = u;
                    hv = v;
                    tri = k;
                }
            }
        }
        return false;
    };
    {
        const float4 r1 = nodes[1];
        if (__float_as_int(r1.z) > 0) {  // the root is a leaf (:252 / :307)
            leaf(__float_as_int(r1.w), __float_as_int(r1.z));
            return;
        }
    }
    const RefSlab s = ref_slab(o, d);
    int sp = 0;
    int left = __float_as_int(nodes[1].w);
    // (a walk over a validated tree of n nodes ends after at most n / 2 pairs; the bound is a guard, not a schedule)
#pragma nounroll
    for (int guard = 0; guard < (1 << 24); guard++) {
        const float4 a0 = nodes[2 * left], a1 = nodes[2 * left + 1], b0 = nodes[2 * left + 2], b1 = nodes[2 * left + 3];
        const int lcount = __float_as_int(a1.z), llink = __float_as_int(a1.w);
        const int rcount = __float_as_int(b1.z), rlink = __float_as_int(b1.w);
        float el, er;
        bool go_l = ref_box(s, a0, a1, el);
        if (go_l && lcount > 0) {
            if (leaf(llink, lcount)) return;
            go_l = false;
        }
        bool go_r = ref_box(s, b0, b1, er);
        if (go_r && rcount > 0) {
            if (leaf(rlink, rcount)) return;
            go_r = false;
        }
        if (go_l && go_r) {
            const bool right_first = el > er;
            stack_push(stack, over, sp, cap, right_first ? llink : rlink);
            left = right_first ? rlink : llink;
        } else if (go_l) {
            left = llink;
        } else if (go_r) {
            left = rlink;
        } else {
            if (sp == 0) break;
            left = stack_pop(stack, over, sp, cap);
        }
    }
}

// ============================================================================ VERIFY: the reference's decisions on the product's walk
// What the reference's walk can SEE is a function of the ray alone: its box test does not look at tmax
// (aabb_intersector.cuh:35), so a leaf is reached iff every box on the way down to it passes `entry <= exit`, whatever has
// been hit before.  Its closest hit is therefore the nearest accepted triangle AMONG THE VISIBLE ONES (ties: the one its
// walk tests last, triangle.cuh:49), and a shadow ray is occluded iff a VISIBLE accepted triangle other than the target
// exists -- definitions that any search order over any acceleration structure can evaluate.  And visibility is cheap:
//   * the boxes along a root-to-leaf path are nested exactly (a node's box is the min / max of its triangles' boxes:
//     bvh.cuh:57-61,150-160); fp32 rounding is monotone, so each slab term inv * bound + scaled_origin is a monotone
//     function of the bound, non-decreasing for inv > 0 and non-increasing for inv < 0; with the octant chosen by the
//     sign of d (aabb_intersector.cuh:14-16) the near bound of a parent gives an entry distance <= its child's and the
//     far bound an exit distance >= its child's.  Hence: IF THE LEAF'S BOX PASSES, EVERY ANCESTOR'S PASSES -- a triangle
//     is visible iff its LEAF's box passes the reference's test (nothing is assumed about the size of any rounding error);
//   * the triangle's own box (triangle.cuh:22-37) lies inside its leaf's, so a pass on the own box -- computed from the
//     record that is in registers anyway -- is a pass on the leaf's: the common case costs no memory access.  Only when
//     the own box fails (flat boxes of axis-aligned triangles hit on their rim: ~1 hit in 10^7) is the leaf's box fetched;
//   * the one case in which octant and sign of 1 / d disagree is a direction component of exactly -0.0 (d < 0 is false,
//     1 / copysign(eps, -0.0) is negative): the nesting argument does not hold then and the ancestors are tested one by
//     one through the parent links.
// So the default kernels keep their own tree, node format, speculation and scheduling and still return the reference's
// answers: a shadow ray's accepted hit only counts if its triangle is visible (k_trace: the walk goes on past an unseen
// occluder; k_paths: the ray ends at its first occluder, and if the reference cannot see that one -- ~1 in 10^7 -- the
// literal walk decides), and a finished path ray's closest hit T is checked once, in the block that shades it anyway: T
// visible and no exact tie at the final distance  =>  T is the reference's closest hit (T is the nearest accepted triangle
// of ALL, so also of the visible ones).  The rest -- T invisible (the nearest VISIBLE hit is needed) or a tie (the
// reference's test order decides) -- is ~2 rays in 10^7 and is re-traced by reference_walk behind a rare branch.  tests/test_traversal_audit.py replays > 4 * 10^7 rays of literal oracle renders through the CPU twin of
// exactly this procedure (rt_host_check.cpp): equal on every ray; the GPU suite holds whole frames to the LITERAL
// oracle's fixed-point image bit for bit.
__device__ __forceinline__ bool neg_zero3(V3 d) {
    return __float_as_uint(d.x) == 0x80000000u || __float_as_uint(d.y) == 0x80000000u || __float_as_uint(d.z) == 0x80000000u;
}
__device__ __forceinline__ bool ref_visible(const DScene &sc, V3 o, V3 d, const Tri &tr, int k,
                                            unsigned long long *__restrict__ vstat) {
    // the reference's slab setup (aabb_intersector.cuh:17-21): 1 / d with |d| clamped away from 0 -- the operand is a
    // unit vector's component, FLT_EPSILON <= |x| <= 1, where rcp_exact_normal IS the IEEE quotient (rt_device.h) -- and
    // the scaled origin (-o) * (1 / d)
#ifndef RT_VERIFY_CLAMP
    // (a component below FLT_EPSILON in magnitude -- where the reference clamps, and where a -0.0 would sit -- is left to the
    // literal forms of the rare path: one min3 and one compare instead of three clamps and three sign tests)
    const bool tiny = fminf(fabsf(d.x), fminf(fabsf(d.y), fabsf(d.z))) < kFltEps;
    const V3 inv = mk(rcp_exact_normal(d.x), rcp_exact_normal(d.y), rcp_exact_normal(d.z));
#else
    const bool tiny = neg_zero3(d);
    const V3 inv = mk(rcp_exact_normal((fabsf(d.x) < kFltEps) ? copysignf(kFltEps, d.x) : d.x),
                      rcp_exact_normal((fabsf(d.y) < kFltEps) ? copysignf(kFltEps, d.y) : d.y),
                      rcp_exact_normal((fabsf(d.z) < kFltEps) ? copysignf(kFltEps, d.z) : d.z));
#endif
    const V3 so = mul(neg(o), inv);
    // the triangle's own box (triangle.cuh:9-10,22-37)
    const V3 p1 = sub(tr.p0, tr.e1), p2 = add(tr.p0, tr.e2);
    const float lox = fminf(tr.p0.x, fminf(p1.x, p2.x)), hix = fmaxf(tr.p0.x, fmaxf(p1.x, p2.x));
    const float loy = fminf(tr.p0.y, fminf(p1.y, p2.y)), hiy = fmaxf(tr.p0.y, fmaxf(p1.y, p2.y));
    const float loz = fminf(tr.p0.z, fminf(p1.z, p2.z)), hiz = fmaxf(tr.p0.z, fmaxf(p1.z, p2.z));
    // aabb_intersector.cuh:24-35: inv * bound + scaled_origin, a multiplication and an addition rounded one by one.  The
    // reference picks the near / far bound by the octant; with the octant consistent with the sign of 1 / d (no -0.0
    // component) the near bound's term is the smaller of the two (monotone rounding again), so min / max pick the same
    // values without the three compares and six selects
    const float tlx = inv.x * lox + so.x, thx = inv.x * hix + so.x;
    const float tly = inv.y * loy + so.y, thy = inv.y * hiy + so.y;
    const float tlz = inv.z * loz + so.z, thz = inv.z * hiz + so.z;
    const float entry = fmaxf(fminf(tlx, thx), fmaxf(fminf(tly, thy), fminf(tlz, thz)));
    const float exit = fminf(fmaxf(tlx, thx), fminf(fmaxf(tly, thy), fmaxf(tlz, thz)));
    bool vis = entry <= exit && !tiny;
    if (!vis) {  // rare (~1 hit in 10^7): the literal forms from here on
        vis = sc.ref_root_leaf != 0;  // bvh.cuh:252 / :307: a root that is a leaf is intersected without any box test
        if (!vis) {
            const RefSlab s = ref_slab(o, d);
            float e;
            // (the own box once more, literally: what the shortcut above could not decide -- a clamped or -0.0 component)
            vis = !neg_zero3(d) && ref_box(s, make_float4(lox, hix, loy, hiy), make_float4(loz, hiz, 0.f, 0.f), e);
        }
        if (!vis) {
            atomicAdd(&vstat[V_OWN_FAIL], 1ull);
            const RefSlab s = ref_slab(o, d);
            float e;
            int node = sc.ref_leaf_of[(unsigned)k];
            vis = ref_box(s, sc.ref_nodes[2 * node], sc.ref_nodes[2 * node + 1], e);
            if (vis && neg_zero3(d)) {  // no nesting argument for this ray: every ancestor below the root (the root's box is never tested)
#pragma nounroll
                for (int guard = 0; guard < 64 && vis; guard++) {
                    node = sc.ref_parent[(unsigned)node];
                    if (node <= 0) break;
                    vis = ref_box(s, sc.ref_nodes[2 * node], sc.ref_nodes[2 * node + 1], e);
                }
            }
            if (!vis) atomicAdd(&vstat[V_LOST], 1ull);
        }
        __asm__ volatile("" ::: "memory");
    }
    return vis;
}

enum { MODE_POOL = 0, MODE_TEST_CLOSEST = 2, MODE_TEST_ANY = 3 };

struct TraceParams {
    int total;             // number of slots (MODE_POOL) or test rays
    int debug_no_deposit;  // perf experiments only: skip the framebuffer atomics
    int fb_fixed;          // framebuffer holds 64-bit fixed-point sums (see deposit())
    float *fb;             // MODE_POOL: raw-sum framebuffer
    DWaveRow *rows;        // MODE_POOL: counter rows
    unsigned long long *prof;  // RT_TRACE_PROFILE builds only
    // lockstep rounds: nothing to trace in a round that shaded nothing (see k_advance); null / 0 otherwise
    const unsigned int *lock_shades;
    int lock_round;
    // test modes
    const float *o3, *d3, *tmax;
    const int *order, *excluded;
    int *out_i;
    float *out_t, *out_u, *out_v;
    unsigned long long *vstat;  // VERIFY builds: DCounters::vstat
};

// MODE_POOL traces BOTH ray kinds of a round in one launch: the path ray of every live slot
// (closest hit, ch()) and the shadow ray of every slot that spawned one (any hit, ah()).  A lane
// carries its kind with its ray, so closest-hit and any-hit rays share waves; the two kinds differ
// only in what a triangle hit does and in how the finished ray is finalised.
// LDS layout (dynamic): [stack: (stack_cap + 1) x kBlock ints (push_if)][pending: kBlock ints]
// MINW: minimum waves per SIMD the register budget is sized for (8 = 64 VGPRs: the renderer's build; the split probe
// also times the builds with 80 / 96 / 128 VGPRs).
// LITERAL (RT_FLAG_REFERENCE_WALK): a lane traverses its whole ray with reference_walk -- the scheduling around it
// (chunks, refill, finalisation) is unchanged, WIDE is not looked at.
// VERIFY (the default; off with RT_FLAG_WATERTIGHT): the product's walk with the reference's decisions -- see ref_visible.
template <int MODE, bool WIDE, int MINW = 8, bool LITERAL = false, bool VERIFY = false>
__global__ void __launch_bounds__(kBlock, MINW) k_trace(DScene sc, DPools p, TraceParams tp, int stack_cap, int *overflow) {
    if (MODE == MODE_POOL && tp.lock_shades != nullptr && tp.lock_round >= 1 && tp.lock_shades[tp.lock_round] == 0u) return;
    extern __shared__ int s_lds[];
    int *stack = s_lds + threadIdx.x;
    int *over = overflow + (blockIdx.x * kBlock + threadIdx.x);
    volatile int *pend = s_lds + (stack_cap + 1) * kBlock + (threadIdx.x & ~63);  // this wave's 64 entries
    const int total = tp.total;
    const int n_chunks = (total + 63) >> 6;                            // chunks per ray kind
    const int all_chunks = MODE == MODE_POOL ? 2 * n_chunks : n_chunks;  // [closest chunks][any chunks]
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
            const bool is_any = MODE == MODE_POOL ? (id & kAnyBit) != 0 : MODE == MODE_TEST_ANY;
            if (VERIFY && !LITERAL && fin && !is_any && tri >= 0) {
                // the closest hit stands if the reference's walk can see its triangle and nothing tied with it at the final
                // distance (the sign of hv: see the leaf phase); otherwise (~2 rays in 10^7) the ray is re-traced literally
                bool bad = (__float_as_uint(hv) >> 31) != 0u;
                if (bad) {
                    atomicAdd(&tp.vstat[V_TIE], 1ull);
                } else {
                    const Tri tr = load_tri(sc.tris, tri);
                    bad = !ref_visible(sc, o, d, tr, tri, tp.vstat);
                }
                if (bad) {
                    atomicAdd(&tp.vstat[V_LITERAL], 1ull);
                    tmax = MODE == MODE_POOL ? kFltMax : tp.tmax[id & (kAnyBit - 1)];
                    tri = -1;
                    hu = hv = 0.f;
                    reference_walk<false>(sc, o, d, tmax, tri, hu, hv, stack, over, stack_cap);
                }
            }
            if (MODE == MODE_POOL) deposits += wave_count((fin && is_any && hu == 0.f));
            if (fin) {
                const int slot = id & (kAnyBit - 1);
                if (MODE == MODE_POOL) {
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
                } else if (MODE == MODE_TEST_CLOSEST) {
                    tp.out_i[slot] = tri >= 0 ? tp.order[tri] : -1;
                    tp.out_t[slot] = tri >= 0 ? tmax : 0.f;
                    tp.out_u[slot] = hu;
                    tp.out_v[slot] = hv;
                } else {
                    tp.out_i[slot] = hu != 0.f ? 1 : 0;
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
                        const bool any_chunk = MODE == MODE_POOL && chunk >= n_chunks;
                        int cand = (any_chunk ? chunk - n_chunks : chunk) * 64 + (int)lane;
                        bool valid = cand < total;
                        if (MODE == MODE_POOL && valid)
                            valid = any_chunk ? p.stmax(cand) >= 0.f : (p.bounces(cand) != kDone && p.bounces(cand) != kParked);
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
                        if (MODE == MODE_POOL) {
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
                        } else {
                            o = mk(tp.o3[3 * slot], tp.o3[3 * slot + 1], tp.o3[3 * slot + 2]);
                            d = mk(tp.d3[3 * slot], tp.d3[3 * slot + 1], tp.d3[3 * slot + 2]);
                            tmax = tp.tmax[slot];
                            tri = MODE == MODE_TEST_ANY ? tp.excluded[slot] : -1;
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
                const bool is_any = MODE == MODE_POOL ? (id & kAnyBit) != 0 : MODE == MODE_TEST_ANY;
                if (is_any) reference_walk<true>(sc, o, d, tmax, tri, hu, hv, stack, over, stack_cap);
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
        // ---- leaf phase: every lane that holds a leaf tests its triangles (triangle.cuh:39-58)
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
            const bool is_any = MODE == MODE_POOL ? (id & kAnyBit) != 0 : MODE == MODE_TEST_ANY;
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
    if (MODE == MODE_POOL) {
        if (deposits != 0 && lane == 0) atomicAdd(&tp.rows[wave_index()].c[C_SHADOW_ADD], deposits);
    }
#ifdef RT_TRACE_PROFILE
    if (MODE == MODE_POOL && lane == 0 && tp.prof) {
        atomicAdd(&tp.prof[0], pf_outer); atomicAdd(&tp.prof[1], pf_refill); atomicAdd(&tp.prof[2], pf_inner_it);
        atomicAdd(&tp.prof[3], pf_inner_lanes); atomicAdd(&tp.prof[4], pf_leaf_it); atomicAdd(&tp.prof[5], pf_leaf_lanes);
        atomicAdd(&tp.prof[6], pf_tri_it); atomicAdd(&tp.prof[7], pf_tri_lanes); atomicAdd(&tp.prof[8], pf_act_at_top);
        atomicAdd(&tp.prof[9], pf_fin_lanes); atomicAdd(&tp.prof[10], 1ull);
    }
#endif
}

// ============================================================================ k_query: ray queries on device buffers
// rt_query_closest_device / rt_query_any_device: the caller's rays, from the caller's device buffers, through the same
// shared device functions as k_trace and k_paths (inv_dir, inner_step, tri_intersect, closest_hit_wins, ref_visible,
// reference_walk, the stack helpers) -- the hit decisions are theirs, only the way from a buffer to them and back is new.
enum { Q_CLOSEST = 0, Q_ANY = 1 };
struct QueryWords {           // the scratch of one query call (rt_scene::QueryState::d_words), zeroed before the prepass
    unsigned radius_bits[3];  // per axis: max |origin| over the finite origin components, as the bits of that float
    unsigned bad_dirs;        // rays with a direction component that is not finite or reaches 2^126
    unsigned bad_pixels;      // rt_render_rays_*: rays whose pixel index is outside the sum buffer (k_pixel_prepass)
    unsigned pad;
    unsigned long long vstat[4];  // V_OWN_FAIL, V_LOST, V_TIE, V_LITERAL of this call (rt_query_last_counters)
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
// products of the reference's box test stay finite).  A non-negative float orders like its bit pattern, so the maximum is
// an integer atomicMax: one per wave and axis after a wave reduction.
__global__ void __launch_bounds__(kBlock) k_query_prepass(const float *__restrict__ o3, const float *__restrict__ d3, int n,
                                                          QueryWords *__restrict__ words) {
    float mx = 0.f, my = 0.f, mz = 0.f;
    unsigned bad = 0;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < (size_t)n; i += stride) {
        const float ox = fabsf(o3[3 * i]), oy = fabsf(o3[3 * i + 1]), oz = fabsf(o3[3 * i + 2]);
        if (ox <= kFltMax) mx = fmaxf(mx, ox);  // (false for +inf and NaN)
        if (oy <= kFltMax) my = fmaxf(my, oy);
        if (oz <= kFltMax) mz = fmaxf(mz, oz);
        const float dm = fmaxf(fabsf(d3[3 * i]), fmaxf(fabsf(d3[3 * i + 1]), fabsf(d3[3 * i + 2])));
        const bool nan = d3[3 * i] != d3[3 * i] || d3[3 * i + 1] != d3[3 * i + 1] || d3[3 * i + 2] != d3[3 * i + 2];
        bad += (nan || !(dm < 0x1p126f)) ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, off));
        my = fmaxf(my, __shfl_xor(my, off));
        mz = fmaxf(mz, __shfl_xor(mz, off));
        bad += __shfl_xor(bad, off);
    }
    if (lane_id() == 0) {
        if (mx > 0.f) atomicMax(&words->radius_bits[0], __float_as_uint(mx));
        if (my > 0.f) atomicMax(&words->radius_bits[1], __float_as_uint(my));
        if (mz > 0.f) atomicMax(&words->radius_bits[2], __float_as_uint(mz));
        if (bad) atomicAdd(&words->bad_dirs, bad);
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

// The walk: one persistent launch per call, the grid sized from the device and not from n.  A wave takes chunks of 64
// consecutive rays round-robin (wave id + k x waves of the grid; no shared head counter, for the reason given in k_trace) and
// hands the rays of its current chunk to idle lanes by ballot + mbcnt: every ray of a chunk is wanted, so the pending rays are
// the id range [pend_lo, pend_hi) in two scalars where k_trace compacts slots into LDS.  Once at most kQueryRefillAt lanes
// still traverse, finished lanes write their result and take the next rays.
// LDS (dynamic): the stack columns, (stack_cap + 1) x kBlock ints (push_if).
// Registers: no pool, shading or camera state is carried, but the VERIFY finalisation (ref_visible + the literal re-trace)
// and the 4-wide node step with its seven 16-byte loads in flight want 71 VGPRs -- over the 64 of 8 waves per SIMD, where
// k_trace's test modes spill 26.  Measured on C2, 2^22 rays (tools/query_time.py, device time of the whole call): budget 8
// 0.689 / 0.912 / 0.703 ms for camera / bounce / shadow rays, budgets 4 to 7 (one and the same code: 71 VGPRs, 7 waves per SIMD,
// no spill, no scratch) 0.565 / 0.730 / 0.680 ms.  kQueryRefillAt: 24, 32, 48 and 56 all land within 1 % of each other on the
// three batches (the spread of one setting's repetitions is 2 %), so k_trace's 40 stays.
// KIND / WIDE / LITERAL / VERIFY: as k_trace's MODE_TEST_* / WIDE / LITERAL / VERIFY.
#ifndef RT_QUERY_MIN_WAVES
#define RT_QUERY_MIN_WAVES 4
#endif
#ifndef RT_QUERY_REFILL_AT
#define RT_QUERY_REFILL_AT 40
#endif
constexpr int kQueryMinWaves = RT_QUERY_MIN_WAVES;
constexpr int kQueryRefillAt = RT_QUERY_REFILL_AT;
template <int KIND, bool WIDE, bool LITERAL, bool VERIFY>
__global__ void __launch_bounds__(kBlock, kQueryMinWaves) k_query(DScene sc, QueryParams qp, int stack_cap, int *overflow) {
    extern __shared__ int s_lds[];
    int *stack = s_lds + threadIdx.x;
    int *over = overflow + (blockIdx.x * kBlock + threadIdx.x);
    const int n = qp.n;
    const int n_chunks = (int)(((unsigned)n + 63u) >> 6);
    const int grid_waves = (int)(gridDim.x * (kBlock / 64));
    int next_chunk = (int)wave_index();
    int pend_lo = 0, pend_hi = 0;  // wave-uniform: ray ids of the current chunk that no lane has taken yet
    // per-lane ray state, as in k_trace: `tri` is the best hit so far (closest) or the excluded triangle (any), leaf order;
    // `hu` doubles as the occluded flag of an any-hit ray
    int id = -1, cur = kEntryDone, sp = 0, tri = -1;
    V3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
    float tmax = 0.f, hu = 0.f, hv = 0.f;

    while (true) {
        unsigned long long act = wave_ballot(id >= 0 && cur != kEntryDone);
        if (__popcll(act) <= kQueryRefillAt) {
            // ---- finalise finished lanes
            const bool fin = id >= 0 && cur == kEntryDone;
            if (KIND == Q_CLOSEST && VERIFY && !LITERAL && fin && tri >= 0) {
                // k_trace's rule: the closest hit stands if the reference's walk can see its triangle and nothing tied with it
                // at the final distance (the sign of hv); otherwise (~2 rays in 10^7) the ray is re-traced literally
                bool bad = (__float_as_uint(hv) >> 31) != 0u;
                if (bad) {
                    atomicAdd(&qp.vstat[V_TIE], 1ull);
                } else {
                    const Tri tr = load_tri(sc.tris, tri);
                    bad = !ref_visible(sc, o, d, tr, tri, qp.vstat);
                }
                if (bad) {
                    atomicAdd(&qp.vstat[V_LITERAL], 1ull);
                    tmax = qp.tmax ? qp.tmax[id] : kFltMax;
                    tri = -1;
                    hu = hv = 0.f;
                    reference_walk<false>(sc, o, d, tmax, tri, hu, hv, stack, over, stack_cap);
                }
            }
            if (fin) {
                if (KIND == Q_CLOSEST) {
                    const bool hit = tri >= 0;
                    qp.out_i[id] = hit ? sc.order[(unsigned)tri] : -1;
                    if (qp.out_t) qp.out_t[id] = hit ? tmax : 0.f;
                    if (qp.out_u) qp.out_u[id] = hit ? hu : 0.f;
                    if (qp.out_v) qp.out_v[id] = hit ? hv : 0.f;
                } else {
                    qp.out_i[id] = hu != 0.f ? 1 : 0;
                }
                id = -1;
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
                    const size_t at = 3 * (size_t)id;
                    o = mk(qp.o3[at], qp.o3[at + 1], qp.o3[at + 2]);
                    d = mk(qp.d3[at], qp.d3[at + 1], qp.d3[at + 2]);
                    tmax = qp.tmax ? qp.tmax[id] : kFltMax;
                    tri = -1;
                    if (KIND == Q_ANY && qp.excluded) {
                        const int e = qp.excluded[id];
                        if (e >= 0 && e < qp.n_tris) tri = qp.inverse[e];
                    }
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
                reference_walk<KIND == Q_ANY>(sc, o, d, tmax, tri, hu, hv, stack, over, stack_cap);
                cur = kEntryDone;
            }
            continue;
        }
        // ---- inner phase: step through node records until no lane holds an inner entry
        while (wave_ballot(cur >= 0) != 0) {
            if (cur >= 0) inner_step<WIDE>(sc, o, inv, tmax, cur, sp, stack, over, stack_cap);
        }
        // ---- leaf phase: every lane that holds a leaf tests its triangles (triangle.cuh:39-58)
        if (cur != kEntryDone && cur < 0) {
            const int ref = ~cur, first = ref >> 3, count = ref & 7;
            bool stop = false;
            for (int k = first; k < first + count; k++) {
                const Tri tr = load_tri(sc.tris, k);
                float t, u, v;
                if (tri_intersect(tr, o, d, tmax, t, u, v)) {
                    if (KIND == Q_ANY) {
                        // bvh.cuh:243: first accepted hit that is not the excluded triangle (VERIFY: and that the reference's
                        // walk can see at all)
                        if (k != tri && (!VERIFY || ref_visible(sc, o, d, tr, k, qp.vstat))) {
                            hu = 1.f;
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
                        // VERIFY: an exact tie is marked in the sign of hv for the finalisation (see k_trace)
                        if (VERIFY && tie) hv = __uint_as_float(__float_as_uint(hv) | 0x80000000u);
                    }
                }
            }
            cur = (!stop && sp > 0) ? stack_pop(stack, over, sp, stack_cap) : kEntryDone;
        }
    }
}

// ============================================================================ k_aov: first-hit feature buffers
// rt_render_aov_fixed / rt_render_aov_rays_fixed_device: per pixel the albedo, the normal, the emission,
// the depth and the hit count of the FIRST hit of every sample, as int64 fixed-point sums, and optionally the ids of a pixel's
// first sample.  k_query's scheme -- one persistent launch, chunks of 64 consecutive sample ids per wave, idle lanes refilled
// by ballot, the shared walk (inv_dir, inner_step, tri_intersect, closest_hit_wins, ref_visible, reference_walk, the stack
// helpers) -- with the two ends replaced: a lane MAKES its ray (SRC = AovCamera: camera ray G of an RT_FLAG_RNG_PER_SAMPLE
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
__device__ __forceinline__ void aov_ray(const AovCamera &s, int id, V3 &o, V3 &d) {
    // gen_core, per-sample streams: pixel = id / spp, the stream of the global id, jitter x then y, camera.get_ray
    const int pixel = (int)((unsigned)id / s.spp);
    const int py = (int)((unsigned)pixel / (unsigned)s.width);
    const int px = pixel - py * s.width;
    Rng rs = rng_sample_stream(s.seed_lo, s.seed_hi, (unsigned long long)id * s.key_mul + s.key_add);
    const float jx = rng_uniform(rs);  // x first, then y (Appendix A.7)
    const float jy = rng_uniform(rs);
    camera_get_ray(s.cam, (px + jx) / s.width, (py + jy) / s.height, o, d);
}
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
__device__ __forceinline__ void aov_deposit(const AovParams &ap, bool dep, int pixel, long long (&val)[RT_AOV_HITS]) {
#ifdef RT_AOV_NO_DEPOSIT
    if (ap.n != 0x7fffffff) return;  // measurement build (tools/aov_time.py): always taken, the host refuses such a frame
#endif
    int hits = dep ? 1 : 0;
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
template <class SRC, bool WIDE, bool LITERAL, bool VERIFY>
__global__ void __launch_bounds__(kBlock, kQueryMinWaves) k_aov(DScene sc, SRC src, AovParams ap, int stack_cap, int *overflow) {
    extern __shared__ int s_lds[];
    int *stack = s_lds + threadIdx.x;
    int *over = overflow + (blockIdx.x * kBlock + threadIdx.x);
    const int n = ap.n;
    const int n_chunks = (int)(((unsigned)n + 63u) >> 6);
    const int grid_waves = (int)(gridDim.x * (kBlock / 64));
    int next_chunk = (int)wave_index();
    int pend_lo = 0, pend_hi = 0;  // wave-uniform: sample ids of the current chunk that no lane has taken yet
    int id = -1, cur = kEntryDone, sp = 0, tri = -1;  // per-lane state, as in k_query
    V3 o = mk(0, 0, 0), d = mk(0, 0, 0), inv = mk(0, 0, 0);
    float tmax = 0.f, hu = 0.f, hv = 0.f;

    while (true) {
        unsigned long long act = wave_ballot(id >= 0 && cur != kEntryDone);
        if (__popcll(act) <= kQueryRefillAt) {
            // ---- finalise finished lanes: the reference's decisions first (k_query's rule, k_trace's)
            const bool fin = id >= 0 && cur == kEntryDone;
            if (VERIFY && !LITERAL && fin && tri >= 0) {
                bool bad = (__float_as_uint(hv) >> 31) != 0u;
                if (bad) {
                    atomicAdd(&ap.vstat[V_TIE], 1ull);
                } else {
                    const Tri tr = load_tri(sc.tris, tri);
                    bad = !ref_visible(sc, o, d, tr, tri, ap.vstat);
                }
                if (bad) {
                    atomicAdd(&ap.vstat[V_LITERAL], 1ull);
                    tmax = kFltMax;
                    tri = -1;
                    hu = hv = 0.f;
                    reference_walk<false>(sc, o, d, tmax, tri, hu, hv, stack, over, stack_cap);
                }
            }
            // ---- deposit: what mat() would shade with (tri_shade, the material) and what init() deposits at bounce 0
            {
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
                if (fin) id = -1;
                aov_deposit(ap, dep, dep ? pixel : -1, val);
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
                    aov_ray(src, id, o, d);
                    tmax = kFltMax;
                    tri = -1;
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
                reference_walk<false>(sc, o, d, tmax, tri, hu, hv, stack, over, stack_cap);
                cur = kEntryDone;
            }
            continue;
        }
        // ---- inner phase: step through node records until no lane holds an inner entry
        while (wave_ballot(cur >= 0) != 0) {
            if (cur >= 0) inner_step<WIDE>(sc, o, inv, tmax, cur, sp, stack, over, stack_cap);
        }
        // ---- leaf phase: every lane that holds a leaf tests its triangles (triangle.cuh:39-58)
        if (cur != kEntryDone && cur < 0) {
            const int ref = ~cur, first = ref >> 3, count = ref & 7;
            for (int k = first; k < first + count; k++) {
                const Tri tr = load_tri(sc.tris, k);
                float t, u, v;
                if (tri_intersect(tr, o, d, tmax, t, u, v)) {
                    const bool tie = t == tmax && tri >= 0;
                    if (closest_hit_wins(sc, t, tmax, k, tri)) {  // bvh.cuh:227-231 (t <= tmax)
                        tmax = t;
                        hu = u;
                        hv = v;
                        tri = k;
                    }
                    // VERIFY: an exact tie is marked in the sign of hv for the finalisation (see k_trace)
                    if (VERIFY && tie) hv = __uint_as_float(__float_as_uint(hv) | 0x80000000u);
                }
            }
            cur = sp > 0 ? stack_pop(stack, over, sp, stack_cap) : kEntryDone;
        }
    }
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
// The two kernels of a frame, once per source of camera rays (see gen_core): the text of rt_frame_kernels.inc compiled with
// RT_FRAME_SRC = Camera as k_advance / k_paths and with RT_FRAME_SRC = RayTable (rt_render_rays_*) as k_advance_rays /
// k_paths_rays.  Two compilations of one text rather than a template parameter or a shared device function: the camera
// builds keep their symbols, their arguments and -- instruction for instruction -- their code.
#define RT_FRAME_SRC Camera
#define RT_K_ADVANCE k_advance
#define RT_K_PATHS k_paths
#include "rt_frame_kernels.inc"
#undef RT_FRAME_SRC
#undef RT_K_ADVANCE
#undef RT_K_PATHS
#define RT_FRAME_SRC RayTable
#define RT_K_ADVANCE k_advance_rays
#define RT_K_PATHS k_paths_rays
#include "rt_frame_kernels.inc"
#undef RT_FRAME_SRC
#undef RT_K_ADVANCE
#undef RT_K_PATHS
// and with RT_FRAME_SRC = KeyedRayTable (rt_render_rays_keyed_*) as k_paths_keyed: per-sample streams, so the persistent kernel
// only (k_advance_keyed is never instantiated)
#define RT_FRAME_SRC KeyedRayTable
#define RT_K_ADVANCE k_advance_keyed
#define RT_K_PATHS k_paths_keyed
#include "rt_frame_kernels.inc"
#undef RT_FRAME_SRC
#undef RT_K_ADVANCE
#undef RT_K_PATHS

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
// ============================================================================ device BVH: refit and build
__device__ __forceinline__ float pad_ulps2(float v, int dir) {  // 2 ulps outward, as the host builder pads
    v = nextafterf(v, dir < 0 ? -kFltMax : kFltMax);
    return nextafterf(v, dir < 0 ? -kFltMax : kFltMax);
}
// one compare-exchange step of a bitonic sort of n_pad (a power of 2) keys
__global__ void k_bitonic_step(unsigned long long *__restrict__ keys, int n_pad, int j, int k) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    int partner = i ^ j;
    if (partner > i) {
        unsigned long long a = keys[i], b = keys[partner];
        bool ascending = (i & k) == 0;
        if ((a > b) == ascending) {
            keys[i] = b;
            keys[partner] = a;
        }
    }
}

// ---- the scene's arrays in leaf order (emit_scene: rt_scene_create, rt_scene_update, rt_scene_rebuild)
// Triangle records: e1 = p0 - p1, e2 = p2 - p0, n = e1 x e2 (triangle.cuh:6-7), each operation rounded once in fp32 (this
// file is built with -ffp-contract=off).
__global__ void k_leaf_tris(const float *__restrict__ verts, const int *__restrict__ order, int n, float4 *__restrict__ tris) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float *q = verts + 9 * (size_t)order[k];
    const float e1x = q[0] - q[3], e1y = q[1] - q[4], e1z = q[2] - q[5];
    const float e2x = q[6] - q[0], e2y = q[7] - q[1], e2z = q[8] - q[2];
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    tris[3 * (size_t)k] = make_float4(q[0], q[1], q[2], e1x);
    tris[3 * (size_t)k + 1] = make_float4(e1y, e1z, e2x, e2y);
    tris[3 * (size_t)k + 2] = make_float4(e2z, nx, ny, nz);
}
// ---- refit (rt_scene_update): new vertex positions for the same tree.  Topology, leaf order, materials and lights stay;
// triangle records, boxes and the tables derived from the light triangles are recomputed on the scene's device.
// One level of the 4-wide tree (launched deepest level first, so a launch boundary orders every hand-off between levels).
// A node's child boxes, EXACT: a leaf child's from the caller's vertices p0, p1, p2 (as rtbvh::build_binary), an inner
// child's the union the deeper launch left in `exact`.  They are written into the node's two builder records padded by
// 2 ulps -- once, on write, as rtbvh::build pads the exact unions -- and their union stays exact for the parent.  With the
// vertices of creation the records are the builder's, bit for bit (min / max are exact; the padding erases the sign of a
// zero).
__global__ void k_refit_level(const float *__restrict__ verts, const int *__restrict__ order, const int *__restrict__ nodes,
                              int count, rtbvh::Pair *__restrict__ recs, float *__restrict__ exact) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int j = nodes[i];
    float u[6] = {kFltMax, kFltMax, kFltMax, -kFltMax, -kFltMax, -kFltMax};
    for (int k = 0; k < 4; k++) {
        rtbvh::Pair &rec = recs[2 * (size_t)j + (k >> 1)];
        const int32_t link = (k & 1) ? rec.rlink : rec.llink;
        if (link == rtbvh::kNoChild) continue;  // (absent: keeps its all-+inf box)
        float b[6] = {kFltMax, kFltMax, kFltMax, -kFltMax, -kFltMax, -kFltMax};
        if (link < 0) {
            const int ref = ~link, first = ref >> 3, cnt = ref & 7;
            for (int t = first; t < first + cnt; t++) {
                const float *v = verts + 9 * (size_t)order[t];
                for (int a = 0; a < 3; a++) {
                    b[a] = fminf(b[a], fminf(v[a], fminf(v[3 + a], v[6 + a])));
                    b[3 + a] = fmaxf(b[3 + a], fmaxf(v[a], fmaxf(v[3 + a], v[6 + a])));
                }
            }
        } else {
            const float *c = exact + 6 * (size_t)(link >> 1);  // (inner links are record indices: 2 x node)
            for (int a = 0; a < 6; a++) b[a] = c[a];
        }
        float *dst = (k & 1) ? rec.rbox : rec.lbox;
        for (int a = 0; a < 3; a++) {
            dst[a] = pad_ulps2(b[a], -1);
            dst[3 + a] = pad_ulps2(b[3 + a], +1);
            u[a] = fminf(u[a], b[a]);
            u[3 + a] = fmaxf(u[3 + a], b[3 + a]);
        }
    }
    for (int a = 0; a < 6; a++) exact[6 * (size_t)j + a] = u[a];
}
// The 4-wide records as the kernels read them, the only writer of that layout (emit_nodes: creation, refit, rebuild and the
// re-padding for far ray origins).  The builder's unpadded records are padded for ray origins within the radius -- the same
// arithmetic as rtbvh::pad_quads_for_origins, its host reference -- and laid out BY PLANE, 128 bytes per node: node j =
// builder records 2j (children 0, 1) and 2j + 1 (children 2, 3) -> word 2a: the four children's lower bounds of axis a,
// word 2a + 1: their upper bounds (a = x, y, z), word 6: the four links, word 7: spare.  A node step loads seven 16-byte
// words (a divergent wave-wide load occupies the CU's texture addresser for about a cycle per active lane:
// profiles/r05_gather_rate.txt) and picks near and far planes by address instead of by min / max (inner_step).  The radius
// is the one asked for, grown to the records' bounds (rtbvh::quads_abs_bounds): those of the root's children, which contain
// every box below them.  Node 0's thread reports it.
__global__ void k_refit_emit(const rtbvh::Pair *__restrict__ recs, int n_nodes, float r0, float r1, float r2,
                             float *__restrict__ out, float *__restrict__ radius_out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_nodes) return;
    float m[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 4; k++) {
        const rtbvh::Pair &p = recs[k >> 1];
        if (((k & 1) ? p.rlink : p.llink) == rtbvh::kNoChild) continue;
        const float *b = (k & 1) ? p.rbox : p.lbox;
        for (int a = 0; a < 3; a++) m[a] = fmaxf(m[a], fmaxf(fabsf(b[a]), fabsf(b[3 + a])));
    }
    const float radius[3] = {fmaxf(r0, m[0] * 1.001f), fmaxf(r1, m[1] * 1.001f), fmaxf(r2, m[2] * 1.001f)};
    if (j == 0)
        for (int a = 0; a < 3; a++) radius_out[a] = radius[a];
    const rtbvh::Pair &p0 = recs[2 * (size_t)j], &p1 = recs[2 * (size_t)j + 1];
    const float *box[4] = {p0.lbox, p0.rbox, p1.lbox, p1.rbox};
    const int32_t link[4] = {p0.llink, p0.rlink, p1.llink, p1.rlink};
    float *r = out + 32 * (size_t)j;
    for (int c = 0; c < 4; c++)
        for (int a = 0; a < 3; a++) {
            float lo = box[c][a], hi = box[c][3 + a];
            if (link[c] != rtbvh::kNoChild) {
                const double pad = (double)radius[a] * 0x1p-23;  // (= ldexp(radius, -23): exact)
                lo = nextafterf((float)((double)lo - pad), -kFltMax);
                hi = nextafterf((float)((double)hi + pad), kFltMax);
            }
            r[8 * a + c] = lo;
            r[8 * a + 4 + c] = hi;
        }
    for (int c = 0; c < 4; c++) r[24 + c] = __int_as_float(link[c]);
    r[28] = r[29] = r[30] = r[31] = 0.f;
}

// ---- PLOC (rt_scene_rebuild, RT_SCENE_DEVICE_BVH): a surface-area-quality tree built on the device -- parallel locally-
// ordered clustering (Meister & Bittner 2018) over 63-bit Morton keys, leaves by the cost model of rt_bvh.h, collapsed to the
// 4-wide records the kernels walk.  Every step is a deterministic function of the vertices (rt_ploc.h holds the expressions
// and the rules; rt_host_check.cpp a sequential twin that gives the same records bit for bit).
struct PlocCluster {  // a cluster: the exact box of its subtree and its node
    float b[6];
    int id, pad;
};
struct PlocNodes {  // the binary tree (rt_ploc.h): ids < n triangles in key order, then the merges
    float *box;     // 6 per node, exact
    int2 *child;    // inner: (left, right); triangle: (-1, original index)
    int *cnt;
    float *cost;
    int *leaf;
    int n;
    __device__ bool is_leaf(int i) const { return leaf[i] != 0; }
    __device__ bool is_tri(int i) const { return i < n; }
    __device__ int tri(int i) const { return child[i].y; }
    __device__ int left(int i) const { return child[i].x; }
    __device__ int right(int i) const { return child[i].y; }
    __device__ int count(int i) const { return cnt[i]; }
    __device__ const float *box_of(int i) const { return box + 6 * (size_t)i; }
};
struct PlocNodesView {  // (rtploc::expand / leaf_tris take box(i) by that name)
    PlocNodes nd;
    __device__ bool is_leaf(int i) const { return nd.is_leaf(i); }
    __device__ bool is_tri(int i) const { return nd.is_tri(i); }
    __device__ int tri(int i) const { return nd.tri(i); }
    __device__ int left(int i) const { return nd.left(i); }
    __device__ int right(int i) const { return nd.right(i); }
    __device__ int count(int i) const { return nd.count(i); }
    __device__ const float *box(int i) const { return nd.box_of(i); }
};
// exclusive prefix sum of v over the 256 threads of a block (4 waves); every thread must call it.  `total`: the block's sum.
__device__ __forceinline__ int ploc_block_scan(int v, int &total) {
    __shared__ int s_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    int off = 0;
    total = 0;
    for (int w = 0; w < 4; w++) {
        if (w < wave) off += s_wave[w];
        total += s_wave[w];
    }
    __syncthreads();  // (s_wave is reused by the next call)
    return off + x - v;
}
// centroid bounds: min / max of the order-preserving bits (exact in any order); bits[0..2] start at ~0, bits[3..5] at 0
__global__ void __launch_bounds__(256) k_ploc_bounds(const float *__restrict__ verts, int n, unsigned *__restrict__ bits) {
    unsigned lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float b[6];
        rtploc::tri_box(verts + 9 * (size_t)i, b);
        for (int a = 0; a < 3; a++) {
            const unsigned u = rtploc::ordered_bits(rtploc::centroid(b, a));
            lo[a] = min(lo[a], u);
            hi[a] = max(hi[a], u);
        }
    }
    for (int a = 0; a < 3; a++) {
        for (int d = 32; d > 0; d >>= 1) {
            lo[a] = min(lo[a], (unsigned)__shfl_xor((int)lo[a], d, 64));
            hi[a] = max(hi[a], (unsigned)__shfl_xor((int)hi[a], d, 64));
        }
    }
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; a++) {
            atomicMin(&bits[a], lo[a]);
            atomicMax(&bits[3 + a], hi[a]);
        }
}
__global__ void k_ploc_keys(const float *__restrict__ verts, int n, int n_pad, float lox, float loy, float loz, float sx, float sy,
                            float sz, unsigned long long *__restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    const float lo[3] = {lox, loy, loz}, s[3] = {sx, sy, sz};
    keys[i] = i < n ? (unsigned long long)rtploc::key(verts + 9 * (size_t)i, i, lo, s) : ~0ull;  // (padding sorts last)
}
// the triangles as the first n nodes (key order) and the first clusters
__global__ void k_ploc_leaves(const float *__restrict__ verts, const unsigned long long *__restrict__ keys, int n, PlocNodes nd,
                              PlocCluster *__restrict__ cl) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int t = rtploc::key_index(keys[k]);
    PlocCluster c;
    rtploc::tri_box(verts + 9 * (size_t)t, c.b);
    c.id = k;
    c.pad = 0;
    for (int a = 0; a < 6; a++) nd.box[6 * (size_t)k + a] = c.b[a];
    nd.child[k] = make_int2(-1, t);
    nd.cnt[k] = 1;
    nd.cost[k] = rtploc::half_area(c.b) * 1.f;
    nd.leaf[k] = 1;
    cl[k] = c;
}
// nearest neighbour of every cluster within the window (ties: rtploc::nearer); the block's window of boxes is staged in LDS
__global__ void __launch_bounds__(256) k_ploc_nearest(const PlocCluster *__restrict__ cl, int m, int pair_ties, int *__restrict__ nn) {
    constexpr int R = rtploc::kRadius, W = 256 + 2 * R;
    __shared__ float s_box[6][W];
    const int base = blockIdx.x * 256;
    for (int t = threadIdx.x; t < W; t += 256) {
        const int g = base - R + t;
        if (g >= 0 && g < m)
            for (int a = 0; a < 6; a++) s_box[a][t] = cl[g].b[a];
    }
    __syncthreads();
    const int i = base + threadIdx.x;
    if (i >= m) return;
    float bi[6];
    for (int a = 0; a < 6; a++) bi[a] = s_box[a][threadIdx.x + R];
    int best_j = -1;
    float best = 0.f;
    const int j_end = min(m - 1, i + R);
    for (int j = max(0, i - R); j <= j_end; j++) {
        if (j == i) continue;
        float bj[6];
        for (int a = 0; a < 6; a++) bj[a] = s_box[a][j - base + R];
        const float d = rtploc::distance(bi, bj);
        if (rtploc::nearer(d, j, i, best, best_j, pair_ties != 0)) {
            best_j = j;
            best = d;
        }
    }
    nn[i] = best_j;
}
__device__ __forceinline__ void ploc_roles(const int *nn, int m, int i, bool &survive, bool &merge) {
    survive = merge = false;
    if (i >= m) return;
    const int j = nn[i];
    const bool mutual = nn[j] == i;
    survive = !mutual || i < j;
    merge = mutual && i < j;
}
// per block: how many clusters survive and how many merges are made (int2 per block)
__global__ void __launch_bounds__(256) k_ploc_count(const int *__restrict__ nn, int m, int2 *__restrict__ block_sums) {
    bool survive, merge;
    ploc_roles(nn, m, blockIdx.x * 256 + threadIdx.x, survive, merge);
    int total = 0;
    ploc_block_scan((survive ? 1 : 0) | (merge ? 1 << 16 : 0), total);  // (two 9-bit counts packed in one scan)
    if (threadIdx.x == 0) block_sums[blockIdx.x] = make_int2(total & 0xffff, total >> 16);
}
// exclusive scan of the per-block sums in place (one block of 1024 threads); totals[0..1] = the sums over all blocks
__global__ void __launch_bounds__(1024) k_ploc_scan(int2 *__restrict__ sums, int nb, int *__restrict__ totals) {
    __shared__ int s_x[1024], s_y[1024];
    const int t = threadIdx.x, per = (nb + 1023) / 1024, b0 = min(nb, t * per), b1 = min(nb, b0 + per);
    int ax = 0, ay = 0;
    for (int b = b0; b < b1; b++) {
        ax += sums[b].x;
        ay += sums[b].y;
    }
    s_x[t] = ax;
    s_y[t] = ay;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int vx = t >= d ? s_x[t - d] : 0, vy = t >= d ? s_y[t - d] : 0;
        __syncthreads();
        s_x[t] += vx;
        s_y[t] += vy;
        __syncthreads();
    }
    int rx = t ? s_x[t - 1] : 0, ry = t ? s_y[t - 1] : 0;
    for (int b = b0; b < b1; b++) {
        const int2 v = sums[b];
        sums[b] = make_int2(rx, ry);
        rx += v.x;
        ry += v.y;
    }
    if (t == 1023) {
        totals[0] = s_x[1023];
        totals[1] = s_y[1023];
    }
}
// merge mutual nearest neighbours into new inner nodes (at the smaller position; ids n + inner_base + rank of the merge) and
// compact the survivors in order
__global__ void __launch_bounds__(256) k_ploc_merge(const PlocCluster *__restrict__ in, const int *__restrict__ nn, int m,
                                                    const int2 *__restrict__ block_offsets, int inner_base, float trav, int max_leaf,
                                                    PlocNodes nd, PlocCluster *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool survive, merge;
    ploc_roles(nn, m, i, survive, merge);
    int total = 0;
    const int r = ploc_block_scan((survive ? 1 : 0) | (merge ? 1 << 16 : 0), total);
    if (!survive) return;
    const int2 off = block_offsets[blockIdx.x];
    const int pos = off.x + (r & 0xffff);
    if (!merge) {
        out[pos] = in[i];
        return;
    }
    const PlocCluster a = in[i], b = in[nn[i]];
    const int id = nd.n + inner_base + off.y + (r >> 16);
    PlocCluster c;
    rtploc::unite(a.b, b.b, c.b);
    c.id = id;
    c.pad = 0;
    const int count = nd.cnt[a.id] + nd.cnt[b.id];
    float cost;
    const bool leaf = rtploc::node_cost(rtploc::half_area(c.b), count, nd.cost[a.id], nd.cost[b.id], trav, max_leaf, cost);
    for (int k = 0; k < 6; k++) nd.box[6 * (size_t)id + k] = c.b[k];
    nd.child[id] = make_int2(a.id, b.id);
    nd.cnt[id] = count;
    nd.cost[id] = cost;
    nd.leaf[id] = leaf ? 1 : 0;
    out[pos] = c;
}
// collapse, one level of 4-wide nodes per launch pair: how many inner children each node of the level has (per block)
__global__ void __launch_bounds__(256) k_ploc_level_count(const int2 *__restrict__ level, int count, PlocNodes nd,
                                                          int2 *__restrict__ block_sums) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int inner = 0;
    if (i < count) {
        const PlocNodesView v{nd};
        int kids[4], firsts[4];
        const int nk = rtploc::expand(v, level[i].x, level[i].y, kids, firsts);
        for (int k = 0; k < nk; k++) inner += v.is_leaf(kids[k]) ? 0 : 1;
    }
    int total = 0;
    ploc_block_scan(inner, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = make_int2(total, 0);
}
// ... and its records: node level_base + i = records 2 (level_base + i) and + 1; inner children become the next level's nodes
// (numbered breadth first: next_base + their rank), leaf children write their triangles into the leaf order
__global__ void __launch_bounds__(256) k_ploc_level_emit(const int2 *__restrict__ level, int count, int level_base, int next_base,
                                                         const int2 *__restrict__ block_offsets, PlocNodes nd,
                                                         rtbvh::Pair *__restrict__ recs, int2 *__restrict__ next_level,
                                                         int *__restrict__ order, int *__restrict__ error) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const PlocNodesView v{nd};
    int kids[4], firsts[4], nk = 0, inner = 0;
    if (i < count) {
        nk = rtploc::expand(v, level[i].x, level[i].y, kids, firsts);
        for (int k = 0; k < nk; k++) inner += v.is_leaf(kids[k]) ? 0 : 1;
    }
    int total = 0;
    int rank = ploc_block_scan(inner, total) + block_offsets[blockIdx.x].x;
    if (i >= count) return;
    rtbvh::Pair rec[2];
    for (int h = 0; h < 2; h++) {
        for (int a = 0; a < 6; a++) rec[h].lbox[a] = rec[h].rbox[a] = INFINITY;
        rec[h].llink = rec[h].rlink = rtbvh::kNoChild;
        rec[h].spare[0] = rec[h].spare[1] = 0;
    }
    for (int k = 0; k < nk; k++) {
        rtbvh::Pair &p = rec[k >> 1];
        const float *b = v.box(kids[k]);
        float *dst = (k & 1) ? p.rbox : p.lbox;
        for (int a = 0; a < 3; a++) {
            dst[a] = pad_ulps2(b[a], -1);
            dst[3 + a] = pad_ulps2(b[3 + a], +1);
        }
        int32_t link;
        if (v.is_leaf(kids[k])) {
            int t[8];
            const int c = rtploc::leaf_tris(v, kids[k], t);
            if (c < 1 || c > 7 || firsts[k] < 0 || firsts[k] + c > nd.n) {
                atomicExch(error, 1);
                return;
            }
            for (int q = 0; q < c; q++) order[firsts[k] + q] = t[q];
            link = ~((firsts[k] << 3) | c);  // (rtbvh::leaf_ref)
        } else {
            next_level[rank] = make_int2(kids[k], firsts[k]);
            link = 2 * (next_base + rank);
            rank++;
        }
        ((k & 1) ? p.rlink : p.llink) = link;
    }
    recs[2 * (size_t)(level_base + i)] = rec[0];
    recs[2 * (size_t)(level_base + i) + 1] = rec[1];
}
// ---- more of the scene's arrays in leaf order (emit_scene), and the reference's tree for a new one (rt_scene_rebuild)
__global__ void k_leaf_inverse(const int *__restrict__ order, int n, int *__restrict__ inverse) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) inverse[order[k]] = k;
}
// (material, light) of every triangle in leaf order, from the caller's two arrays in their order on the device (tri_light
// null: no triangle carries a light)
__global__ void k_leaf_tri_info(const int *__restrict__ tri_material, const int *__restrict__ tri_light, const int *__restrict__ order,
                                int n, int2 *__restrict__ info) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int i = order[k];
    info[k] = make_int2(tri_material[i], tri_light ? tri_light[i] : -1);
}
// rt_scene_set_lights: a new light assignment in the caller's order, the materials as they are (already in leaf order)
__global__ void k_leaf_tri_light(const int2 *__restrict__ old_info, const int *__restrict__ tri_light, const int *__restrict__ order,
                                 int n, int2 *__restrict__ info) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) info[k] = make_int2(old_info[k].x, tri_light[order[k]]);
}
// rt_scene_set_triangles_device / rt_scene_create_device: one pass over the caller's index arrays before anything is built
// from them (in the manner of k_query_prepass) -- how many triangles name a material outside [0, n_mats) (words[0]) or a
// light outside [-1, n_lights) (words[1]; tri_light may be null).  One atomic per wave and word after a wave reduction.
__global__ void __launch_bounds__(kBlock) k_index_prepass(const int *__restrict__ tri_material, const int *__restrict__ tri_light, int n,
                                                          int n_mats, int n_lights, unsigned *__restrict__ words) {
    unsigned bad_m = 0, bad_l = 0;
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < (size_t)n; i += stride) {
        bad_m += (unsigned)tri_material[i] >= (unsigned)n_mats ? 1u : 0u;
        if (tri_light) bad_l += (unsigned)tri_light[i] + 1u >= (unsigned)n_lights + 1u ? 1u : 0u;  // (-1 wraps to 0: no light)
    }
    for (int off = 32; off > 0; off >>= 1) {
        bad_m += __shfl_xor(bad_m, off);
        bad_l += __shfl_xor(bad_l, off);
    }
    if (lane_id() == 0) {
        if (bad_m) atomicAdd(&words[0], bad_m);
        if (bad_l) atomicAdd(&words[1], bad_l);
    }
}
// area lights name their triangle in the caller's order (rt_light.triangle): the leaf-order index the kernels read
__global__ void k_leaf_lights(Light *__restrict__ lights, int n_lights, const int *__restrict__ inverse) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_lights && lights[i].type == RT_AREA_LIGHT) lights[i].tri = inverse[lights[i].tri];
}
// the reference's tree (a function of the triangles alone) for the new leaf order: its primitives' and leaves' indices
__global__ void k_ploc_remap_ref(const int *__restrict__ prims, const int *__restrict__ leaf_of, const int *__restrict__ old_order,
                                 const int *__restrict__ inverse, int n, int *__restrict__ new_prims, int *__restrict__ new_leaf_of) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    new_prims[i] = inverse[old_order[prims[i]]];
    new_leaf_of[inverse[old_order[i]]] = leaf_of[i];
}

#include "rt_host_scene.inc"   // (opens the anonymous namespace that is closed below) rt_scene: upload, reference tree, checks, emit, update, rebuild, edits; what the ray entry points share
#include "rt_host_render.inc"  // Context, kernel selection, frames, test rays, queries, ray tables, AOVs
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
    return rt_scene_create_flags(tri_p0p1p2, n_tris, tri_material, tri_light, materials, n_materials, lights, n_lights, 0u, out_scene);
}

int rt_scene_create_flags(const float *tri_p0p1p2, int n_tris, const int32_t *tri_material, const int32_t *tri_light,
                          const rt_material *materials, int n_materials, const rt_light *lights, int n_lights,
                          uint32_t scene_flags, rt_scene **out_scene) {
    if (!out_scene) return fail("rt_scene_create: out_scene is null");
    if (scene_flags & ~(uint32_t)RT_SCENE_DEVICE_BVH) return fail("rt_scene_create_flags: unknown scene flags");
    const bool device_bvh = (scene_flags & RT_SCENE_DEVICE_BVH) != 0;
    *out_scene = nullptr;
    if (check_scene_counts("rt_scene_create", n_tris, n_tris <= 0 || (tri_p0p1p2 && tri_material), materials, n_materials, lights, n_lights) ||
        check_tri_indices("rt_scene_create", n_tris, tri_material, tri_light, n_materials, n_lights) ||
        check_scene_tables("rt_scene_create", n_tris, materials, n_materials, lights, n_lights))
        return 1;
    auto sc = std::make_unique<rt_scene>();
    HIP_TRY(hipGetDevice(&sc->device));
    sc->wide = true;  // 4-wide nodes (two pair-style records each): half the dependent fetches per ray; RT_BVH_WIDE=0: 2-wide
    if (const char *e = knob("RT_BVH_WIDE")) sc->wide = atoi(e) != 0;
    if (device_bvh && !sc->wide) return fail("rt_scene_create_flags: the device builder writes the 4-wide format only (RT_BVH_WIDE=0 is set)");
    sc->n_tris = n_tris;
    sc->n_lights = n_lights;
    sc->n_mats = n_materials;
    if (n_tris > 0) sc->h_tri9.assign(tri_p0p1p2, tri_p0p1p2 + 9 * (size_t)n_tris);  // (RT_FLAG_REFERENCE_WALK builds its tree from these)
    if (n_tris > 0) sc->h_tri_material.assign(tri_material, tri_material + n_tris);
    if (n_tris > 0 && tri_light) sc->h_tri_light.assign(tri_light, tri_light + n_tris);
    if (n_materials > 0) sc->h_materials.assign(materials, materials + n_materials);
    if (n_lights > 0) sc->h_lights.assign(lights, lights + n_lights);
    sc->note_index_maxima();
    DevScope tmp;
    float *d_verts = nullptr;
    if (n_tris > 0) {
        if (tmp.alloc(d_verts, 9 * (size_t)n_tris)) return 1;
        HIP_TRY(hipMemcpy(d_verts, tri_p0p1p2, sizeof(float) * 9 * (size_t)n_tris, hipMemcpyHostToDevice));
    }
    std::vector<rtbvh::Pair> pairs;  // (2-wide)
    if (device_bvh && n_tris > 0) {
        // the device PLOC builder on this device (the scene's)
        PlocBuild b;
        if (build_ploc_device(d_verts, n_tris, nullptr, b, "rt_scene_create_flags")) return 1;
        if (!ploc_result_ok(b, n_tris)) return fail("rt_scene_create_flags: the device-built tree is malformed");
        adopt_tree(sc.get(), b);
    } else {
        // the host SAH builder (also for a device build of no triangles: there is nothing to build)
        const auto t0 = std::chrono::steady_clock::now();
        rtbvh::Result bvh = rtbvh::build(tri_p0p1p2, n_tris);
        if (!device_bvh) sc->build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        sc->builder = device_bvh ? 2 : 0;
        if (!bvh.ok) return fail("rt_scene_create: BVH build produced an unreferenceable leaf");
        if (n_tris > 0 && !bvh.quads.empty() && !validate_quads(bvh.quads, n_tris))
            return fail("rt_scene_create: the 4-wide BVH is malformed (structure, or an absent child without its +inf box)");
        // a tree too deep for the 4-wide walk's stack (up to 3 entries per level) may still fit the 2-wide walk's (1 per level):
        // a host tree the reinsertion pass deepened
        if (sc->wide && bvh.stack_bound > kMaxStackBound) sc->wide = false;
        if ((sc->wide ? bvh.stack_bound : bvh.pair_depth + 1) > kMaxStackBound)
            return fail("rt_scene_create: BVH depth " + std::to_string(sc->wide ? bvh.max_depth : bvh.pair_depth) + " exceeds the traversal stack");
        sc->n_nodes = sc->wide ? (int)bvh.quads.size() : (int)bvh.pairs.size();  // 64-byte records
        sc->max_depth = sc->wide ? bvh.max_depth : bvh.pair_depth;
        sc->stack_bound = sc->wide ? bvh.stack_bound : bvh.pair_depth + 1;
        sc->n_leaves = bvh.num_leaves;
        sc->set_order(bvh.order);
        HIP_TRY(hipMalloc((void **)&sc->d_order, sizeof(int) * std::max(n_tris, 1)));
        if (n_tris) HIP_TRY(hipMemcpy(sc->d_order, sc->h_order.data(), sizeof(int) * n_tris, hipMemcpyHostToDevice));
        if (sc->wide) {
            sc->h_quads = std::move(bvh.quads);
            HIP_TRY(hipMalloc((void **)&sc->d_recs, sizeof(rtbvh::Pair) * sc->h_quads.size()));
            HIP_TRY(hipMemcpy(sc->d_recs, sc->h_quads.data(), sizeof(rtbvh::Pair) * sc->h_quads.size(), hipMemcpyHostToDevice));
        } else {
            pairs = std::move(bvh.pairs);
        }
    }
    static_assert(sizeof(Light) == sizeof(rt_light), "light layout");
    static_assert(sizeof(Material) == sizeof(rt_material), "material layout");
    static_assert(sizeof(Camera) == sizeof(rt_camera), "camera layout");
    sc->tab_dwords = 5 * n_materials + 24 * n_lights;
    const size_t nt = (size_t)std::max(n_tris, 1);
    HIP_TRY(hipMalloc((void **)&sc->d_nodes, 64 * (size_t)sc->n_nodes));
    HIP_TRY(hipMalloc((void **)&sc->d_radius, sizeof(float) * 3));
    HIP_TRY(hipMalloc((void **)&sc->d_tris, sizeof(float4) * 3 * nt));
    HIP_TRY(hipMalloc((void **)&sc->d_tri_info, sizeof(int2) * nt));
    HIP_TRY(hipMalloc((void **)&sc->d_tri_shade, sizeof(float4) * nt));
    HIP_TRY(hipMalloc((void **)&sc->d_mats, sizeof(Material) * std::max(n_materials, 1)));
    if (n_materials) HIP_TRY(hipMemcpy(sc->d_mats, materials, sizeof(Material) * n_materials, hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc((void **)&sc->d_lights, sizeof(Light) * std::max(n_lights, 1)));
    HIP_TRY(hipMalloc((void **)&sc->d_tables, sizeof(float) * (size_t)std::max(sc->tab_dwords, 1)));
    if (!sc->wide)
        if (int rc = upload_pairs(sc.get(), pairs)) return rc;
    int *d_inverse = nullptr;
    if (tmp.alloc(d_inverse, nt)) return 1;
    EmitSource src;
    if (scene_source(sc.get(), true, nullptr, tmp, src)) return 1;
    if (emit_scene(sc.get(), src, d_verts, sc->arrays(), d_inverse, nullptr)) return 1;
    if (sc->wide) HIP_TRY(hipMemcpy(sc->origin_radius, sc->d_radius, sizeof(float) * 3, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    *out_scene = sc.release();
    return 0;
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
    if (!out_scene) return fail("rt_scene_create_device: out_scene is null");
    *out_scene = nullptr;
    auto sc = std::make_unique<rt_scene>();  // an empty scene on the current device that takes its first triangle set
    HIP_TRY(hipGetDevice(&sc->device));
    sc->wide = true;
    if (const char *e = knob("RT_BVH_WIDE")) sc->wide = atoi(e) != 0;
    if (scene_set_triangles_impl(sc.get(), d_tri_p0p1p2, n_tris, d_tri_material, d_tri_light, materials, n_materials, lights, n_lights,
                                 true, (hipStream_t)stream, "rt_scene_create_device"))
        return 1;
    *out_scene = sc.release();
    return 0;
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

int rt_post_process_fixed(const int64_t *d_sum_fixed, float *d_rgb_out, int num_pixels, int num_samples, void *stream) {
    if (!d_sum_fixed || !d_rgb_out || num_pixels <= 0 || num_samples <= 0) return fail("rt_post_process_fixed: bad argument");
    if (num_pixels > 0x7fffffff / 3) return fail("rt_post_process_fixed: more than 715827882 pixels");
    int nv = num_pixels * 3;
    float inv = 1.f / (float)num_samples;
    hipLaunchKernelGGL(k_post_process_fixed, dim3((nv + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const long long *)d_sum_fixed, d_rgb_out, nv, inv);
    HIP_TRY(hipGetLastError());
    return 0;
}

int rt_render_aov_fixed(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples, uint64_t seed,
                        int shard_index, int shard_count, uint32_t flags, int64_t *d_aov_fixed, int32_t *d_ids, void *stream,
                        rt_stats *stats) {
    return render_aov_impl(scene, camera, width, height, num_samples, seed, shard_index, shard_count, flags, d_aov_fixed, d_ids,
                           (hipStream_t)stream, stats);
}

int rt_render_aov_rays_fixed_device(const rt_scene *scene, int64_t n_rays, const float *d_origin_xyz, const float *d_dir_xyz,
                                    const int32_t *d_pixel, int rays_per_pixel, int n_pixels, uint64_t key_first,
                                    uint32_t key_stride, uint32_t flags, int64_t *d_aov_fixed, int32_t *d_ids, void *stream,
                                    rt_stats *stats) {
    return render_aov_rays_impl(scene, n_rays, d_origin_xyz, d_dir_xyz, d_pixel, rays_per_pixel, n_pixels, key_first, key_stride,
                                flags, d_aov_fixed, d_ids, (hipStream_t)stream, stats);
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

int rt_post_process(float *d_rgb, int num_pixels, int num_samples, void *stream) {
    if (!d_rgb || num_pixels <= 0 || num_samples <= 0) return fail("rt_post_process: bad argument");
    if (num_pixels > 0x7fffffff / 3) return fail("rt_post_process: more than 715827882 pixels");
    int nv = num_pixels * 3;
    float inv = 1.f / (float)num_samples;
    hipLaunchKernelGGL(k_post_process, dim3((nv + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_rgb, nv, inv);
    HIP_TRY(hipGetLastError());
    return 0;
}

int rt_render(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples,
              int max_bounces, uint64_t seed, uint32_t flags, float *out_rgb, rt_stats *stats) {
    if (!out_rgb) return fail("rt_render: out_rgb is null");
    if (width <= 0 || height <= 0) return fail("rt_render: bad dimensions");
    if ((long long)width * height > (long long)(0x7fffffff / 3)) return fail("rt_render: width*height exceeds 715827882 pixels");
    const bool fixed = (flags & RT_FLAG_DETERMINISTIC) != 0;
    const size_t n_values = 3 * (size_t)width * height;
    const size_t bytes = sizeof(float) * n_values;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) return fail("rt_render: device ordinal out of range");
    std::lock_guard<std::mutex> out_lock(g_dev_busy[dev]);  // (this device's cached buffers serve one host-output call at a time)
    float *d_fb = (float *)out_buffer(dev, 0, bytes);
    long long *d_fixed = fixed ? (long long *)out_buffer(dev, 1, sizeof(long long) * n_values) : nullptr;
    if (!d_fb || (fixed && !d_fixed)) return fail("rt_render: out of device memory");
    int rc = 0;
    if (fixed) {
        HIP_TRY(hipMemsetAsync(d_fixed, 0, sizeof(long long) * n_values, nullptr));
        rc = render_overlapped(scene, camera, width, height, num_samples, max_bounces, seed, 0, 1,
                               (flags & ~kFlagFixedFb) | kFlagFixedFb, (float *)d_fixed, nullptr, stats);
        if (rc) return rc;
        rc = rt_post_process_fixed((const int64_t *)d_fixed, d_fb, width * height, num_samples, nullptr);
    } else {
        HIP_TRY(hipMemsetAsync(d_fb, 0, bytes, nullptr));
        rc = render_overlapped(scene, camera, width, height, num_samples, max_bounces, seed, 0, 1, flags & ~kFlagFixedFb,
                               d_fb, nullptr, stats);
        if (rc) return rc;
        rc = rt_post_process(d_fb, width * height, num_samples, nullptr);
    }
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_rgb, d_fb, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// Releases every device allocation the library holds behind the scenes -- the per-device render contexts (path pools, RNG
// states, counters, overflow stacks, events) and the cached output buffers of rt_render / rt_render_multi.  Scenes are the
// caller's (rt_scene_destroy).  No render may be in flight.  The library works again afterwards (everything is re-created on
// demand).  (The reference frees nothing at all: render.cuh:374-391, bvh.cuh:211-217.)
void rt_shutdown(void) {
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

// The scene as it exists on `device`: the scene itself, or a replica created there from the host copies (once per device).
static const rt_scene *scene_on_device(const rt_scene *scene, int device) {
    if (scene->device == device) return scene;
    std::lock_guard<std::mutex> lock(scene->replica_mutex);
    for (const rt_scene *r : scene->replicas)
        if (r->device == device) return r;
    DeviceGuard dev;
    if (dev.enter(device)) {
        fail("rt_render_multi: cannot select device " + std::to_string(device));
        return nullptr;
    }
    rt_scene *rep = nullptr;
    // (a scene whose tree was built on the device gets one built on the replica's device)
    const int rc = rt_scene_create_flags(scene->h_tri9.data(), scene->n_tris, scene->h_tri_material.data(),
                                         scene->h_tri_light.empty() ? nullptr : scene->h_tri_light.data(), scene->h_materials.data(),
                                         scene->n_mats, scene->h_lights.data(), scene->n_lights,
                                         scene->builder == 2 ? (uint32_t)RT_SCENE_DEVICE_BVH : 0u, &rep);
    if (rc != 0) return nullptr;
    scene->replicas.push_back(rep);
    return rep;
}

int rt_render_multi(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples,
                    int max_bounces, uint64_t seed, uint32_t flags, const int *devices, int n_devices, float *out_rgb,
                    rt_stats *stats) {
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
    const uint32_t shard_flags = (flags & ~kFlagFixedFb) | (fixed ? kFlagFixedFb : 0u);
    const size_t n_values = 3 * (size_t)width * height;
    const size_t sum_bytes = n_values * (fixed ? sizeof(long long) : sizeof(float));
    int caller_device = 0;
    HIP_TRY(hipGetDevice(&caller_device));
    // every device's copy of the scene, before any thread starts (replicas are created under the scene's lock)
    std::vector<const rt_scene *> on_dev(n_devices, nullptr);
    for (int k = 0; k < n_devices; k++) {
        on_dev[k] = scene_on_device(scene, devices[k]);
        if (!on_dev[k]) return 1;
    }
    // device buffers: cached per (device, slot) like rt_render's; slot 2 + 2k = shard k's sums on its device, 3 + 2k = its
    // staging copy on devices[0], slot 1 = the post-processed image (fixed-point mode)
    std::vector<int> distinct(devices, devices + n_devices);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    if (distinct.back() >= kMaxDevices) return fail("rt_render_multi: device ordinal out of range");
    std::vector<std::unique_lock<std::mutex>> out_locks;  // (ascending device order: two concurrent calls cannot deadlock)
    for (int d : distinct) out_locks.emplace_back(g_dev_busy[d]);
    struct Home {  // the calling thread's device is restored on every return path
        int device;
        ~Home() { (void)hipSetDevice(device); }
    } home{caller_device};
    struct {
        void *alloc(int device, int slot, size_t bytes) { return hipSetDevice(device) == hipSuccess ? out_buffer(device, slot, bytes) : nullptr; }
    } buf;
    const int dev0 = devices[0];
    // Peer access between devices[0] and every other listed device, once per pair and process: with it the shards' sums travel
    // over xGMI straight into devices[0]'s memory; without it hipMemcpyPeerAsync still works, staged through host memory by
    // the runtime.  (Nothing of this has run on two PHYSICAL devices yet -- one-GPU boxes list a device twice; the first
    // multi-GPU run is the driver's scaling run, where bench.py's probe records what happened here: `peer_access`.)
    {
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
        (void)hipSetDevice(caller_device);
    }
    // shard k renders into its own raw-sum buffer on ITS device; shards 1.. land in a staging buffer on devices[0]
    std::vector<void *> d_sum(n_devices, nullptr), d_stage(n_devices, nullptr);
    for (int k = 0; k < n_devices; k++) {
        d_sum[k] = buf.alloc(devices[k], 2 + 2 * k, sum_bytes);
        if (!d_sum[k]) return fail("rt_render_multi: out of device memory on device " + std::to_string(devices[k]));
        if (k > 0) {
            d_stage[k] = devices[k] == dev0 ? d_sum[k] : buf.alloc(dev0, 3 + 2 * k, sum_bytes);  // (same device: the buffer is its own staging)
            if (!d_stage[k]) return fail("rt_render_multi: out of device memory on device " + std::to_string(dev0));
        }
    }
    float *d_out = fixed ? (float *)buf.alloc(dev0, 1, n_values * sizeof(float)) : (float *)d_sum[0];
    if (!d_out) return fail("rt_render_multi: out of device memory");
    // ---- one host thread per device (render.cuh's render() is one thread on one device: this is the multi-device form of
    // the same call): select the device, zero the shard's sums, render slot shard k of n, hand the sums to devices[0]
    std::vector<rt_stats> sub(n_devices);
    std::vector<int> rc(n_devices, 0);
    std::vector<std::string> err(n_devices);
    std::vector<std::thread> th;
    for (int k = 0; k < n_devices; k++)
        th.emplace_back([&, k] {
            auto bail = [&](const char *what) { rc[k] = 1; err[k] = std::string("rt_render_multi: ") + what + " (device " + std::to_string(devices[k]) + ")"; };
            if (hipSetDevice(devices[k]) != hipSuccess) return bail("hipSetDevice failed");
            hipStream_t st;
            if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return bail("stream create failed");
            if (hipMemsetAsync(d_sum[k], 0, sum_bytes, st) != hipSuccess) {
                bail("memset failed");
            } else {
                rc[k] = render_shard_impl(on_dev[k], camera, width, height, num_samples, max_bounces, seed, k, n_devices, shard_flags,
                                          (float *)d_sum[k], st, &sub[k], /* a context of its own per shard: */ 8 + k);
                if (rc[k]) err[k] = g_last_error;
                else if (k > 0 && d_stage[k] != d_sum[k]) {
                    const hipError_t pe = hipMemcpyPeerAsync(d_stage[k], dev0, d_sum[k], devices[k], sum_bytes, st);
                    if (pe != hipSuccess) bail((std::string("peer copy of the shard's sums failed: ") + hipGetErrorString(pe)).c_str());
                }
            }
            if (hipStreamSynchronize(st) != hipSuccess && rc[k] == 0) bail("stream synchronise failed");
            (void)hipStreamDestroy(st);
        });
    for (auto &t : th) t.join();
    for (int k = 0; k < n_devices; k++)
        if (rc[k]) return fail(err[k]);
    // ---- on devices[0]: add the shards' sums in shard order (a fixed order: the result does not depend on which device
    // finished first), post-process (render.cuh:330-338), copy out
    HIP_TRY(hipSetDevice(dev0));
    const int nv = (int)n_values;
    for (int k = 1; k < n_devices; k++) {
        if (fixed) hipLaunchKernelGGL(k_accumulate_i64, dim3((nv + 255) / 256), dim3(256), 0, nullptr, (long long *)d_sum[0], (const long long *)d_stage[k], nv);
        else hipLaunchKernelGGL(k_accumulate_f32, dim3((nv + 255) / 256), dim3(256), 0, nullptr, (float *)d_sum[0], (const float *)d_stage[k], nv);
    }
    HIP_TRY(hipGetLastError());
    int prc = fixed ? rt_post_process_fixed((const int64_t *)d_sum[0], d_out, width * height, num_samples, nullptr)
                    : rt_post_process(d_out, width * height, num_samples, nullptr);
    if (prc) return prc;
    HIP_TRY(hipMemcpy(out_rgb, d_out, n_values * sizeof(float), hipMemcpyDeviceToHost));
    if (stats) {
        rt_stats tot = sub[0];
        for (int k = 1; k < n_devices; k++) {
            tot.camera_rays += sub[k].camera_rays;
            tot.shade_events += sub[k].shade_events;
            tot.closest_rays += sub[k].closest_rays;
            tot.any_rays += sub[k].any_rays;
            tot.emission_adds += sub[k].emission_adds;
            tot.shadow_adds += sub[k].shadow_adds;
            tot.rr_draws += sub[k].rr_draws;
            tot.iterations = std::max(tot.iterations, sub[k].iterations);
            tot.launches_trace += sub[k].launches_trace;
            tot.seconds_trace = std::max(tot.seconds_trace, sub[k].seconds_trace);
            tot.seconds_advance = std::max(tot.seconds_advance, sub[k].seconds_advance);
            tot.seconds_render = std::max(tot.seconds_render, sub[k].seconds_render);  // the devices render side by side
            tot.seconds_rng_init = std::max(tot.seconds_rng_init, sub[k].seconds_rng_init);
            tot.seconds_reference_tree = std::max(tot.seconds_reference_tree, sub[k].seconds_reference_tree);
            for (int q = 4; q < 7; q++) tot.reserved[q] += sub[k].reserved[q];
        }
        tot.reserved[3] = n_devices;
        *stats = tot;
    }
    return 0;
}

int rt_trace_closest(const rt_scene *scene, int n, const float *origin_xyz, const float *dir_xyz, const float *tmax,
                     int32_t *hit_tri, float *t, float *u, float *v) {
    return rt_trace_closest_flags(scene, 0u, n, origin_xyz, dir_xyz, tmax, hit_tri, t, u, v);
}

int rt_trace_closest_flags(const rt_scene *scene, uint32_t flags, int n, const float *origin_xyz, const float *dir_xyz,
                           const float *tmax, int32_t *hit_tri, float *t, float *u, float *v) {
    if (!scene || n < 0 || (n > 0 && (!origin_xyz || !dir_xyz || !tmax || !hit_tri || !t || !u || !v)))
        return fail("rt_trace_closest: bad argument");
    if (n == 0) return 0;
    float *d_t, *d_u, *d_v;
    int *d_h;
    DevScope tmp;
    if (tmp.alloc(d_t, (size_t)n) || tmp.alloc(d_u, (size_t)n) || tmp.alloc(d_v, (size_t)n) || tmp.alloc(d_h, (size_t)n)) return 1;
    TraceParams tp{};
    tp.order = scene->d_order;
    tp.out_i = d_h;
    tp.out_t = d_t;
    tp.out_u = d_u;
    tp.out_v = d_v;
    if (int rc = trace_test_rays<MODE_TEST_CLOSEST>(scene, flags, n, origin_xyz, dir_xyz, tmax, tp, tmp)) return rc;
    HIP_TRY(hipMemcpy(hit_tri, d_h, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(t, d_t, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(u, d_u, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(v, d_v, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

int rt_trace_any(const rt_scene *scene, int n, const float *origin_xyz, const float *dir_xyz, const float *tmax,
                 const int32_t *excluded_tri, int32_t *occluded) {
    return rt_trace_any_flags(scene, 0u, n, origin_xyz, dir_xyz, tmax, excluded_tri, occluded);
}

int rt_trace_any_flags(const rt_scene *scene, uint32_t flags, int n, const float *origin_xyz, const float *dir_xyz,
                       const float *tmax, const int32_t *excluded_tri, int32_t *occluded) {
    if (!scene || n < 0 || (n > 0 && (!origin_xyz || !dir_xyz || !tmax || !excluded_tri || !occluded)))
        return fail("rt_trace_any: bad argument");
    if (n == 0) return 0;
    std::vector<int> excl(n);
    for (int i = 0; i < n; i++) {
        int e = excluded_tri[i];
        excl[i] = (e >= 0 && e < scene->n_tris) ? scene->h_inverse[e] : -1;
    }
    int *d_e, *d_occ;
    DevScope tmp;
    if (tmp.alloc(d_e, (size_t)n) || tmp.alloc(d_occ, (size_t)n)) return 1;
    HIP_TRY(hipMemcpy(d_e, excl.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    TraceParams tp{};
    tp.excluded = d_e;
    tp.out_i = d_occ;
    if (int rc = trace_test_rays<MODE_TEST_ANY>(scene, flags, n, origin_xyz, dir_xyz, tmax, tp, tmp)) return rc;
    HIP_TRY(hipMemcpy(occluded, d_occ, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
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
