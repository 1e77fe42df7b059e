/* rtcuda_amd_tools.h -- the LAB: measurement entry points of librtcuda_amd_tools.so (rtcuda_amd/csrc/rt_tools.hip).
 *
 * NOT part of the drop-in C-ABI (include/rtcuda_amd.h): nothing here replaces a reference interface -- the reference measures
 * nothing.  bench.py uses the two roofs (copy bandwidth, vector-ALU issue) for its roofline block; the scripts under tools/ use the rest.
 * The tools library is built from the product's own translation unit plus these tools, so the scene handle of
 * rt_split_probe must come from the tools library's own rt_scene_create. */
#ifndef RTCUDA_AMD_TOOLS_H
#define RTCUDA_AMD_TOOLS_H

#include <stdint.h>

#include "rtcuda_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Measured device copy bandwidth in bytes/s (float4 copy of `bytes` bytes, best of `reps`):
 * the HBM roofline denominator SURVEY.md section 8d asks to be measured in the same run. */
int rt_measure_copy_bandwidth(int64_t bytes, int reps, double *out_bytes_per_s);

/* Measured vector-ALU roof in lane-operations/s: `waves_per_simd` waves on every SIMD of the chip, each issuing
 * iters x 16 independent v_fma_f32 (best of 6 timed launches).  The render kernels are bound by VALU issue, not
 * by HBM, so this -- next to the 157.3 TFLOP/s = 78.6 T lane-FMA/s spec -- is what bench.py's roofline divides by.
 * out_wave_instr (may be NULL): v_fma_f32 wave-instructions of one launch, for calibrating PMC counters.
 * No reference counterpart (the reference measures nothing). */
int rt_calibrate_valu(int waves_per_simd, int iters, double *out_lane_ops_per_s, double *out_wave_instr);

/* The same measurement with PACKED fp32 instructions (kind 1: v_pk_fma_f32, 2: v_pk_mul_f32, 3: v_pk_add_f32) on aligned
 * register pairs; lane-operations are counted as two per lane and instruction.  No reference counterpart. */
int rt_calibrate_valu_packed(int waves_per_simd, int iters, int kind, double *out_lane_ops_per_s);

/* How long ONE wave needs per instruction of a given kind, with `waves_per_simd` waves on every SIMD: out_seconds = best launch
 * time of a kernel in which every wave issues *out_wave_instr_per_wave instructions of kind (16 independent chains per lane
 * unless noted): 0 v_fma_f32 (VOP3), 1 v_fmac_f32, 2 v_mul_f32, 3 v_add_f32, 4 v_mov_b32, 5 v_xor_b32, 6 v_lshlrev_b32,
 * 7 v_max_f32, 8 v_rcp_f32, 9 v_sqrt_f32, 10 v_cndmask_b32, 11 v_mul_f32 + dependent v_add_f32, 12 ONE dependent chain of
 * v_fma_f32, 13 one dependent chain of v_mul_f32, 14 v_mul_f32 with a literal, 15 v_mul_f32 with an SGPR operand,
 * 16 v_fma_f32 with two SGPR operands, 17 v_cndmask_b32 with an SGPR-pair mask, 18 v_cmp_lt_f32 -> vcc, 19 v_cmp_lt_f32 +
 * dependent v_cndmask_b32, 20 v_bfi_b32, 21 v_and_b32, 22 - 25 three v_mul_f32 + one v_cndmask_b32 / v_max_f32 / v_mul_f32 /
 * v_mov_b32 per chain (an instruction's cost inside a mix).  No reference counterpart (tools/issue_probe.py). */
int rt_probe_issue(int kind, int waves_per_simd, int iters, double *out_seconds, double *out_wave_instr_per_wave);

/* Measurement tool for the design question "one persistent kernel, or the reference's stage split (render.cuh:428-449:
 * init/mat/gen kernels and ah/ch kernels with dense queues between them)?".  Runs the round-per-launch pipeline of the
 * frame from its start until `target_rays` rays have been traced, copying every round's rays (closest-hit and any-hit
 * apart) and every round's shading inputs (by material kind) into dense device arrays; then times, on those arrays,
 *   - the trace kernel alone at 8 / 6 / 5 / 4 waves per SIMD: the walker the product ships for dense ray arrays (k_query's
 *     ends on stream_walk, watertight build) compiled at each budget -- so the eight trace-only entries price the stage
 *     split with that kernel (up to commit 78db776: with dense-array modes of the pool kernel k_trace, which are gone),
 *   - the shading code alone (the product's init() + mat()), one material kind per launch, every lane shading,
 * each as the best of three launches (HIP events).  out[] is indexed by the RT_PROBE_* enum; times in seconds.
 * No reference counterpart. */
enum {
    RT_PROBE_ROUNDS = 0,          /* rounds of the pipeline that were run and dumped */
    RT_PROBE_CLOSEST_RAYS,        /* rays in the closest-hit array */
    RT_PROBE_ANY_RAYS,            /* rays in the any-hit array */
    RT_PROBE_S_ADVANCE_ROUND0,    /* k_advance of round 0: every slot runs gen() */
    RT_PROBE_S_ADVANCE,           /* k_advance, rounds 1.. (sum) */
    RT_PROBE_S_TRACE_POOL,        /* k_trace over the pools, all rounds (sum) */
    RT_PROBE_S_TRACE_CLOSEST,     /* [4]: closest-hit array at 8 / 6 / 5 / 4 waves per SIMD */
    RT_PROBE_S_TRACE_ANY = RT_PROBE_S_TRACE_CLOSEST + 4,            /* [4]: any-hit array */
    RT_PROBE_TRACE_BLOCKS_PER_CU = RT_PROBE_S_TRACE_ANY + 4,        /* [4]: resident 256-thread blocks per CU of each build */
    RT_PROBE_SHADES = RT_PROBE_TRACE_BLOCKS_PER_CU + 4,             /* [3]: shading records per kind (matte, mirror, glass) */
    RT_PROBE_S_SHADE = RT_PROBE_SHADES + 3,                         /* [3]: shading-only launch per kind */
    RT_PROBE_COUNT = RT_PROBE_S_SHADE + 3
};
int rt_split_probe(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples,
                   int max_bounces, uint64_t seed, int64_t target_rays, double *out, int n_out);

/* A scene's 4-wide tree as the builder left it: the unpadded node records (two 64-byte records per node, children 0, 1 |
 * 2, 3, as rt_bvh.h's `quads`) and the leaf order (leaf-order index -> caller's triangle index).  out2 = [records,
 * triangles]; the records and the order are copied when the buffers are given and large enough.  For comparing the device
 * builder (RT_SCENE_DEVICE_BVH, rt_scene_rebuild) with its host twin (rt_host_check.cpp).  4-wide scenes only. */
int rt_scene_tree_copy(const rt_scene *scene, void *records, int64_t cap_records, int32_t *order, int64_t cap_order,
                       int64_t *out2);

/* The product's shading FUNCTIONS on a table of inputs, one lane per row: the device side of the reference pins
 * (tests/golden/ref_shade_fixture.npz).  `func` and the row layouts are those of oracle/ref_shade_driver.cpp, 32-bit words in
 * and out, for the ten functions the device has as functions of their own:
 *    1 sample_f, 2 get_f, 6 intersect, 7 offset_ray_origin, 8 power_heuristic, 9 same_hemisphere, 10 reflect,
 *    11 refract (4 arguments), 12 uniform_sample_sphere, 13 get_ray
 * with two differences.  Where the driver's row ends in two uniforms (1 and 12), the row here ends in the six words of an
 * XORWOW state {d, v0 .. v4} instead -- the state the lane's generator starts from (17 and 6 words in); `draws` comes out as
 * the number of draws made from it.  And sample_f writes one word more, 12 in all: again_draws, what a second call with the
 * same arguments would consume.  intersect: t, u, v are the device function's, meaningful on a hit only.
 * in_words and out_words are HOST arrays of n_rows rows; out_words is copied to the device first, so a word no lane writes
 * keeps the caller's value.  Any other func (3 sample_Li, 4 pdf_Li and 5 sample_p have no device function of their own:
 * rt_shade_records) is an error; n_rows = 0 succeeds.  No reference counterpart. */
int rt_shade_table(int func, int n_rows, const uint32_t *in_words, uint32_t *out_words);

/* The product's init() + mat() -- advance_core as the persistent kernel compiles it, through the shading probe of
 * rt_split_probe -- on n path states of the caller's, one lane each, against a scene of THIS library's rt_scene_create.
 * records_in: n rows of RT_SHADE_RECORD_IN words: bounces, hit_info (-1 = a miss, else material | (light + 1) << 16),
 * pixel, gen, XORWOW state d v0 .. v4, beta 3, wo 3, isect_p 3, isect_n 3.  Every row names a pixel of its own in 0 .. n - 1.
 * records_out: n rows of RT_SHADE_RECORD_OUT words: the next ray o d (0 - 5, written when the state shades), the shadow ray
 * o d (6 - 11), its tmax (12: -1.0f when there is none), its radiance (13 - 15) and the triangle it must not hit (16: the
 * caller's index, -1 for a point light), beta (17 - 19), the XORWOW state (20 - 25), bounces (26), and the three floats of
 * pixel i of a framebuffer that was zero before the launch (27 - 29: the bounce-0 emission of the record that names pixel
 * i).  Words the kernel does not write (no new ray, no shadow ray) hold RT_SHADE_UNWRITTEN.
 * lds_tables: 1 = the build that stages the shading tables in LDS (an error with more than 64 materials or lights), 0 = the
 * build that reads them from global memory.  The BSDF-sampled MIS ray of mat() does not exist on the device (its draws are
 * burnt), so Light::pdf_Li has no counterpart here.  No reference counterpart. */
enum { RT_SHADE_RECORD_IN = 22, RT_SHADE_RECORD_OUT = 30 };
#define RT_SHADE_UNWRITTEN 0xffffffffu
int rt_shade_records(const rt_scene *scene, int max_bounces, int lds_tables, int n, const uint32_t *records_in,
                     uint32_t *records_out);

/* One pass of rt_denoise_fixed in one form, `reps` launches timed one by one with HIP events (out_ms, a HOST array).  d_scratch:
 * the scratch an rt_denoise_fixed call with passes = 0 left for the same frame (prepared {u, z} and {n}); the pass of `stride`
 * (a power of two up to 128, with its kc) reads them and writes the scratch's second array.  form: 1 = the direct form
 * k_atrous, 2 = the LDS form k_atrous_lds. */
int rt_denoise_pass_time(void *d_scratch, int width, int height, int stride, int form, float sigma_color, float sigma_depth,
                         int normal_power_log2, int reps, float *out_ms);

/* One pass of rt_denoise_dual_fixed, `reps` launches timed one by one with HIP events (out_ms, a HOST array).  d_scratch: the
 * scratch an rt_denoise_dual_fixed call with passes = 0 left for the same frame (prepared {u, v} and {n, z}); the pass of `stride`
 * (a power of two up to 128) reads them and writes the scratch's second array.  form: 1 = the direct form k_atrous_var, 2 = the
 * LDS form k_atrous_var_lds.  g_place: 1 = the variance prefilter in the pass, 2 = k_dn_var_blur before it, inside the timed
 * interval. */
int rt_denoise_dual_pass_time(void *d_scratch, int width, int height, int stride, int form, int g_place, float sigma_variance,
                              float sigma_depth, int normal_power_log2, int reps, float *out_ms);

#ifdef __cplusplus
}
#endif
#endif /* RTCUDA_AMD_TOOLS_H */
