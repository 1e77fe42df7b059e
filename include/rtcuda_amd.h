/* rtcuda_amd.h -- C-ABI of the MI355X-native render path (drop-in for lashhw/rtcuda's render()).
 *
 * Plain C: opaque handles, plain pointers and sizes, int status codes.  No torch / HIP types.
 * Every entry point names the reference interface it replaces (file:line into the reference
 * tree).  The C++ host API that keeps the reference's class names (Vec3 / Triangle / Material /
 * Light / Primitive / Bvh / Scene / Camera / render) is include/rtcuda/rtcuda.hpp -- a
 * header-only layer over exactly these functions.
 *
 * Conventions
 *   - return 0 on success, non-zero on failure; rt_last_error() gives the message
 *     (the reference prints and exit()s instead: utility.cuh:6-13).
 *   - all device memory is owned by the library behind rt_scene* / an internal per-device
 *     context (the reference leaks every allocation: main.cu:50,121,136; bvh.cuh:211-217;
 *     render.cuh:374-391).
 *   - "current device" is the calling thread's current HIP device (hipSetDevice /
 *     torch.cuda.set_device); one process per GPU is the intended deployment.
 *   - triangle, material and light POINTERS of the reference API become INDICES here.
 */
#ifndef RTCUDA_AMD_H
#define RTCUDA_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_NUM_WORKING_PATHS 1048576 /* constant.hpp:8 -- number of path slots == RNG streams */

enum { RT_MATTE = 0, RT_MIRROR = 1, RT_GLASS = 2 };  /* material.cuh:4-8 */
enum { RT_POINT_LIGHT = 0, RT_AREA_LIGHT = 1 };      /* light.cuh:4-7 */

/* material.cuh:20-22 (same field order, 20 bytes) */
typedef struct rt_material {
    float albedo[3];
    float index_of_refraction;
    int32_t type;
} rt_material;

/* light.cuh:20-26 with `Triangle *d_triangle` flattened to a triangle index (32 bytes) */
typedef struct rt_light {
    int32_t type;
    float pos[3];     /* point light */
    int32_t triangle; /* area light: index into the scene's triangle array */
    float L[3];       /* radiance (area) or intensity I (point) */
} rt_light;

/* camera.cuh:11-14 (48 bytes): what Camera's constructor leaves in the object */
typedef struct rt_camera {
    float lookfrom[3];
    float upper_left[3];
    float horizontal[3];
    float vertical[3];
} rt_camera;

typedef struct rt_scene rt_scene;

/* Per-render counters (the reference has only stdout).  All counts are for THIS shard.
 * camera_rays and closest_rays count every camera ray the reference generates and traces, including those of background
 * pixels -- pixels outside the rectangle the scene's bounds project to, whose rays cannot hit anything -- which the persistent
 * kernel counts, draws the jitter of, and no longer walks.  bench.py's grays_per_s therefore includes them. */
typedef struct rt_stats {
    int64_t camera_rays;     /* gen events      (render.cuh:250)  */
    int64_t shade_events;    /* mat events      (render.cuh:139)  */
    int64_t closest_rays;    /* rays traced by the closest-hit kernel */
    int64_t any_rays;        /* rays traced by the any-hit kernel */
    int64_t emission_adds;   /* bounce-0 emission deposits (render.cuh:98-103) */
    int64_t shadow_adds;     /* unoccluded NEE deposits    (render.cuh:291-293) */
    int64_t rr_draws;        /* Russian-roulette draws     (render.cuh:117) */
    int64_t iterations;      /* stage rounds launched */
    int64_t bvh_nodes;       /* node records of the device BVH */
    int64_t bvh_depth;
    double seconds_render;   /* device time of the render loop (HIP events), excl. RNG init */
    double seconds_rng_init; /* device time of the one-off XORWOW state initialisation */
    double seconds_trace;    /* trace kernel (closest-hit + any-hit rays of a round in one launch): average
                                launch duration (HIP events on the launch stream, every 4th round sampled)
                                x launches; 0 unless RT_FLAG_TIME_KERNELS */
    double seconds_reference_tree; /* host seconds this call spent building + uploading the reference's own tree (first render of
                                      a scene without RT_FLAG_WATERTIGHT; 0 afterwards): a one-off like the BVH build */
    double seconds_advance;  /* same for the advance kernel */
    int64_t launches_trace;  /* launches of each stage kernel (= iterations) */
    int64_t reserved[7];     /* reserved[0] = launches actually sampled by the event timer;
                                reserved[1] = nonzero when the frame ran as one persistent k_paths launch (then
                                seconds_trace is that launch's duration and launches_trace is 1): 1 + the camera rays
                                per task of the chunked deal of slots to lanes in its low 32 bits, so 1 = the static deal,
                                and in bits 32 .. 47 the slot sets a lane ran statically before that deal began; bit 48: the launch
                                was a build that makes no camera ray for background pixels (k_paths<PathsBg> / k_paths<PathsChunkedBg>);
                                reserved[2] = BVH node records that launch staged in LDS (small shards only);
                                reserved[3] = rt_render_multi: number of device shards behind these totals;
                                default kernels (no RT_FLAG_WATERTIGHT): reserved[4] = rays re-traced through the reference's
                                own tree, reserved[5] = accepted hits the reference's box test loses, reserved[6] = closest
                                hits with an exact tie at the final distance */
} rt_stats;

/* Flags for rt_render / rt_render_shard */
#define RT_FLAG_TIME_KERNELS 1u  /* time the stage kernels with HIP events on the launch stream (fills seconds_*) */
#define RT_FLAG_DETERMINISTIC 2u /* rt_render: accumulate in 64-bit fixed point (2^-30) instead of float atomics
                                    (vec3.cuh:149-153): bit-reproducible image, independent of summation order */

#define RT_FLAG_RNG_PER_SAMPLE 4u /* NOT the reference's random numbers: every camera ray starts a stream of its own, keyed by
                                    (seed, camera ray id), instead of continuing its path SLOT's stream (render.cuh:72,156,263).
                                    The image is a statistically equivalent estimate, not the reference's image sample for
                                    sample -- no test compares it with the reference's image.  It is exactly defined all the
                                    same: camera ray G = 0 .. width * height * num_samples - 1 has the
                                    pixel G / num_samples and the stream curand_init's seed scramble (subsequence 0) makes of
                                    the 64-bit word splitmix64 yields for (seed, G): z = seed + 0x9E3779B97F4A7C15 * (G + 1),
                                    finalised; its path is the reference's estimator on that stream alone, run to its own end
                                    with the RT_FLAG_WATERTIGHT hit definition, and its contributions are summed in float in
                                    path order and added to the pixel once.  The CPU oracle restates this as a loop over camera
                                    rays, and the GPU suite holds the mode's fixed-point sums and event totals to that
                                    restatement bit for bit (tests/test_gpu_per_sample.py).  What it buys: the frame no longer depends on which
                                    slot or GPU serves a camera ray, so with rt_render_shard every rank runs ALL W slots on
                                    num_samples / shard_count samples of every pixel (num_samples % shard_count == 0), the
                                    shards' fixed-point sums add up to the 1-GPU sums exactly, and 8 GPUs are not held to
                                    1/8 of the W chains each (SURVEY.md section 7 "per_sample", section 8b `rng_mode`) */

/* WHICH HITS A RAY FINDS: the reference's own decisions are the default.
 * Two results of lashhw/rtcuda are properties of its own BVH, not of the scene: its fp32 slab test on exact boxes
 * (aabb_intersector.cuh:14-36, hit iff entry <= exit, no look at tmax) drops about one accepted hit in 10^7 rays, and among
 * hits at exactly equal t the triangle its walk tests last wins (triangle.cuh:49).  Both are functions of the ray alone --
 * a triangle is visible to the reference's walk iff the box of its LEAF passes that slab test (the boxes above it are nested
 * exactly and fp32 rounding is monotone, so they pass with it) -- which lets the library reproduce them on its OWN tree:
 *
 *   flags = 0 (default; what bench.py times): the product's 4-wide walk; a shadow ray's occluder counts only if the
 *       reference's walk can see it; a path ray's closest hit is checked once (visible? no exact tie at the final distance?)
 *       and the ~2 rays in 10^7 that fail are re-traced through the reference's own binary SAH tree (bvh.cuh:30-219, built
 *       from the scene's triangles on first use).  The image equals the reference ALGORITHM's image ray for ray: every
 *       event total and every fixed-point pixel sum of the six full BASELINE frames equals the literal CPU restatement's.
 *   RT_FLAG_REFERENCE_WALK: every ray walks the reference's own tree as Bvh::traverse does (bvh.cuh:221-357).  Same image as
 *       the default, five times slower: the cross-check of the default, kept for that.
 *   RT_FLAG_WATERTIGHT: the triangle-list definition instead -- an accepted hit is never lost to a box test, ties go to the
 *       larger caller index: what exhaustive search over all triangles returns.  About 1 path in 4 * 10^6 differs from the
 *       reference's image (on BASELINE config 5 those paths carry whole light deposits: RMS 3.2e-4); 3 - 4 % faster.
 *       LIMIT of that promise: a triangle the ray sees nearer to edge-on than cos(d, n) = 2^-11 (about 2 hits in 10^7) has an
 *       fp32 t made of rounding noise, which can lie in front of its own box by any amount; if another triangle's hit lies in
 *       between, the walk may return that one where exhaustive search returns the edge-on one.  Down to that angle the distance
 *       limit of the box test is widened for it (rt_bvh.h, kCullTmaxWiden; profiles/ray_families.md).
 *
 * FAR-OFF AND DUPLICATED GEOMETRY.  The rate of the rare path is a property of where the scene sits: the reference's slab test
 * loses hits in proportion to the size of the coordinates, so a scene shifted by 1e4 sends 42 of 20 000 camera rays (and 20 to 30
 * of 20 000 bounce rays) through the literal re-trace where the scene in [0, 1]^3 sends none; stretching x by 1e3 or squashing
 * y by 1e-3: 0 to 5.  The answers hold all the same -- flags 0 and RT_FLAG_REFERENCE_WALK the literal restatement's, RT_FLAG_
 * WATERTIGHT exhaustive search's, bit for bit on every ray (tests/test_placed_scenes_host.py on the CPU twin of the kernels' procedure, tests/test_gpu_placed_scenes.py on the kernels:
 * queries, frames and a refit from [0, 1]^3 to 1e4; the bunny at 1e5 host-built, device-built and rebuilt).
 * Duplicated triangles and triangles that fp32 collapsed to points (the bunny at 1e5: 34 815 distinct of 69 467) are scenes
 * like any other: both builders cut runs of equal boxes by count, rt_scene_create and rt_scene_rebuild
 * accept them, and hits at equal t on identical triangles go to the reference's tree order (default) or the larger index.
 *
 * CAVEAT ("the reference" = its algorithm in separately rounded fp32): this library and the CPU oracle are built with
 * -ffp-contract=off, so inv * bound + scaled_origin is a multiplication and an addition.  The reference's CMake build uses
 * nvcc's defaults (fmad on): a CUDA binary contracts that expression -- and others -- into FMAs and loses a DIFFERENT handful
 * of rays; its libdevice sincosf / powf differ from the pinned forms here as well.  Bit parity with a CUDA binary is unpinned
 * and cannot be had offline; what is exact is parity with the literal restatement of the source. */
#define RT_FLAG_REFERENCE_WALK 8u /* every ray through the reference's own tree (see above); not with RT_FLAG_RNG_PER_SAMPLE */
#define RT_FLAG_WATERTIGHT 16u    /* the triangle-list definition of the hits (see above); not with RT_FLAG_REFERENCE_WALK */

/* ---- scene -------------------------------------------------------------------------------
 * Replaces: Triangle(p0,p1,p2) x n (triangle.cuh:6-7), cudaMalloc/Memcpy of triangles,
 * materials and lights (main.cu:50-51,119-122,136-137), Primitive(tri*,mat*,light*)
 * (primitive.cuh:6-7), Bvh(triangles, primitives) (bvh.cuh:30-219) and the Scene aggregate
 * (scene.cuh:4-8).  tri_p0p1p2 is n_tris x 9 floats; tri_light[i] is the index into `lights`
 * of the area light that triangle i carries, or -1 (may be NULL = no area lights).
 * The light ORDER is the caller's (the reference's comes from unordered_map iteration,
 * main.cu:128).  Uploads to the current device. */
int rt_scene_create(const float *tri_p0p1p2, int n_tris, const int32_t *tri_material,
                    const int32_t *tri_light, const rt_material *materials, int n_materials,
                    const rt_light *lights, int n_lights, rt_scene **out_scene);
/* rt_scene_create with options.  RT_SCENE_DEVICE_BVH: the BVH is built on the current device by PLOC (parallel locally-
 * ordered clustering over Morton-ordered triangles, surface-area cost model for the leaves, collapsed to the same 4-wide
 * records) in milliseconds instead of the host SAH build's tenths of a second; traversal quality is close to the host
 * tree's.  The image is the same, bit for bit, in every mode.  rt_render_multi replicas of such a scene are built on their
 * own device the same way.  Fails (instead of falling back) if the tree does not fit the traversal stack, or with
 * RT_BVH_WIDE=0.  scene_flags 0 is rt_scene_create. */
#define RT_SCENE_DEVICE_BVH 1u
int rt_scene_create_flags(const float *tri_p0p1p2, int n_tris, const int32_t *tri_material,
                          const int32_t *tri_light, const rt_material *materials, int n_materials,
                          const rt_light *lights, int n_lights, uint32_t scene_flags, rt_scene **out_scene);
void rt_scene_destroy(rt_scene *scene);

/* out[0]=node records, out[1]=triangles, out[2]=max depth, out[3]=leaves */
int rt_scene_info(const rt_scene *scene, int64_t out[4]);
/* Which BVH builder made the scene (0 = host SAH, the default; 2 = device PLOC, RT_SCENE_DEVICE_BVH or rt_scene_rebuild;
 * 1 is retired and no longer reported) and how long the build took (host wall clock / HIP events).  The reference times
 * "Top-down constructing BVH" on stdout (bvh.cuh:106-201). */
int rt_scene_build_info(const rt_scene *scene, int *builder, double *seconds);

/* ---- moving geometry (no reference counterpart: its Bvh is built once, bvh.cuh:30-219) ----------------------------
 * New positions for the scene's triangles: n_tris x 9 floats, the caller's ORIGINAL order, the scene's count (that of its
 * creation or of its last rt_scene_set_triangles*).
 * Materials, light assignment and topology are kept.  The BVH is refit on the scene's device (same tree, new boxes);
 * triangle, shading and light-triangle records are recomputed.  No render of this scene may be in flight.
 * The image is that of a scene created anew from the same vertices, bit for bit, in every mode (hits never depend on the
 * product's own tree).  What follows an update: the reference's tree (default mode, RT_FLAG_REFERENCE_WALK) is rebuilt on the
 * host from the new triangles by the next render that needs it (about 0.045 s on the bunny, reported in
 * seconds_reference_tree; RT_FLAG_WATERTIGHT never pays it), and replicas made by rt_render_multi are dropped and recreated
 * on their next use.  Errors (null scene or pointer, another triangle count, a 2-wide RT_BVH_WIDE=0 scene) leave the scene
 * as it was. */
int rt_scene_update(rt_scene *scene, const float *tri_p0p1p2, int n_tris);
/* Same, from a DEVICE buffer on the scene's device, ordered on `stream` (NULL = default stream), synchronous on return. */
int rt_scene_update_device(rt_scene *scene, const float *d_tri_p0p1p2, int n_tris, void *stream);
/* refits since creation, device seconds of the last refit (HIP events), and the tree's surface-area cost relative to its
 * value at build time (advisory: when it grows, rebuild the tree with rt_scene_rebuild) */
int rt_scene_refit_info(const rt_scene *scene, int64_t *refits, double *seconds_last, double *sah_ratio);
/* A new tree for the scene, built on its device by the RT_SCENE_DEVICE_BVH builder: from the scene's current vertices
 * (tri_p0p1p2 NULL) or from new ones (as rt_scene_update takes them).  When to call it: a refit keeps the tree's topology,
 * so as vertices move its quality decays -- rebuild when rt_scene_refit_info's sah_ratio has grown (say past 1.2); the
 * ratio reads 1.0 again afterwards.  Preconditions are rt_scene_update's: the scene's count, a 4-wide scene, no render in
 * flight.  The image is unchanged, bit for bit, in every mode: it is that of a scene created from the same vertices.  The
 * leaf order changes; triangle, shading, light and table records are re-emitted on the device.  The reference's tree
 * (RT_FLAG_REFERENCE_WALK, default mode) is kept when the vertices did not change and rebuilt by the next render that needs
 * it when they did; rt_render_multi replicas are dropped.  rt_scene_build_info reports builder 2 and the device build time.
 * Errors (null scene, another count, a 2-wide RT_BVH_WIDE=0 scene, a tree deeper than the traversal stack) leave the scene
 * rendering as before. */
int rt_scene_rebuild(rt_scene *scene, const float *tri_p0p1p2, int n_tris);
/* Same, from a DEVICE buffer on the scene's device (or NULL: the current vertices), ordered on `stream` (NULL = default
 * stream), synchronous on return. */
int rt_scene_rebuild_device(rt_scene *scene, const float *d_tri_p0p1p2, int n_tris, void *stream);

/* ---- editing a scene in place (no reference counterpart: its Scene is assembled once, main.cu:119-137) -------------
 * What a scene IS may change between frames without rt_scene_destroy + rt_scene_create: its material table, its lights and
 * its whole triangle set.  THE CONTRACT, for all five entry points: afterwards every render, query and ray-table render of
 * the scene gives, bit for bit and in every mode, what a scene created by rt_scene_create from the same arrays gives.
 * Preconditions are rt_scene_rebuild's: no render or query of the scene in flight; the calling thread's current device is
 * left as it was.  The checks are rt_scene_create's (counts, index ranges, material and light types, an area light's
 * triangle within the triangle count, at most 65535 materials and 32766 lights, fewer than 2^24 triangles).  Every error
 * returns non-zero, names the entry point in rt_last_error() and leaves the scene rendering its old bits: new records are
 * built in fresh buffers and adopted at the end.  After an edit rt_scene_update* / rt_scene_rebuild* take the NEW count.
 *
 * rt_scene_set_materials: a new material table (HOST array, any count >= 1 that covers every index the triangles name).
 * rt_scene_set_lights: new lights (HOST array, n_lights may be 0) and, unless tri_light is NULL, a new light assignment of
 *   the triangles (HOST array of the scene's triangle count, -1 = none).  With NULL the assignment is kept and must fit
 *   the new count.
 * Both keep the tree, the leaf order, rt_scene_build_info, the refit state and the reference's tree (none depends on
 * materials or lights): they cost table uploads and one or two small launches whatever the triangle count.  The shading
 * tables are re-made for the new counts, so the next render stages them in LDS or reads them from memory as the counts
 * allow; rt_render_multi replicas are dropped. */
int rt_scene_set_materials(rt_scene *scene, const rt_material *materials, int n_materials);
int rt_scene_set_lights(rt_scene *scene, const rt_light *lights, int n_lights, const int32_t *tri_light);
/* A new triangle set: any count >= 1, with the per-triangle indices and the tables they index into (all of
 * rt_scene_create's arguments; materials and lights are HOST arrays in every form, tri_light may be NULL = no area lights).
 * The tree is built on the scene's device by the RT_SCENE_DEVICE_BVH builder and every record is re-emitted there, as
 * rt_scene_rebuild does for moved vertices, with every array re-allocated for the new count.  rt_scene_info follows,
 * rt_scene_build_info reports builder 2 and the device build time, rt_scene_refit_info keeps its refit count and reads
 * ratio 1.0; the reference's tree is rebuilt by the next render that needs it, replicas are dropped.  Needs a 4-wide scene.
 * An empty scene stays with rt_scene_create. */
int rt_scene_set_triangles(rt_scene *scene, const float *tri_p0p1p2, int n_tris, const int32_t *tri_material,
                           const int32_t *tri_light, const rt_material *materials, int n_materials,
                           const rt_light *lights, int n_lights);
/* Same, the three per-triangle arrays from DEVICE buffers on the scene's device (a host pointer is an error), ordered on
 * `stream` (NULL = default stream), synchronous on return.  The index ranges are checked on the device before anything is
 * adopted; the error names how many triangles are out of range.  The library's host mirrors (reference tree, replicas) are
 * filled by one device-to-host copy per array. */
int rt_scene_set_triangles_device(rt_scene *scene, const float *d_tri_p0p1p2, int n_tris, const int32_t *d_tri_material,
                                  const int32_t *d_tri_light, const rt_material *materials, int n_materials,
                                  const rt_light *lights, int n_lights, void *stream);
/* rt_scene_create_flags(RT_SCENE_DEVICE_BVH) from DEVICE buffers on the current device: no host copy of the triangles is
 * needed to make a scene.  n_tris >= 1; `stream` as above. */
int rt_scene_create_device(const float *d_tri_p0p1p2, int n_tris, const int32_t *d_tri_material,
                           const int32_t *d_tri_light, const rt_material *materials, int n_materials,
                           const rt_light *lights, int n_lights, void *stream, rt_scene **out_scene);

/* Replaces Camera::Camera(lookfrom, lookat, up, vfov_deg, aspect) (camera.cuh:15-29). Host only. */
int rt_camera_make(const float lookfrom[3], const float lookat[3], const float up[3], float vfov_deg,
                   float aspect_ratio, rt_camera *out);

/* ---- render ------------------------------------------------------------------------------
 * Replaces render(width, height, num_samples, max_bounces, camera, scene, framebuffer)
 * (render.cuh:366-457) with RAND_SEED (render.cuh:417) exposed as `seed` (reference: 1).
 * out_rgb: HOST buffer of width*height*3 floats, row-major, top row first, each channel
 * sqrt(sum/spp) exactly as post_process_framebuffer leaves it (render.cuh:330-338). */
int rt_render(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples,
              int max_bounces, uint64_t seed, uint32_t flags, float *out_rgb, rt_stats *stats);

/* The same call over several GPUs of one node, in ONE process (no reference counterpart: render.cuh:366-367 drives one
 * device from one thread).  devices[0 .. n_devices) are HIP device ordinals; n_devices must divide W (1, 2, 4, 8, ...).
 * The scene is replicated onto every listed device on first use (the replicas belong to `scene` and die with it), one
 * host thread per device renders slot shard k of n_devices (see rt_render_shard) into a raw-sum buffer on its own
 * device, the shards' sums are copied to devices[0] (peer copies over xGMI), added there in shard order, post-processed
 * and copied to out_rgb (HOST, as rt_render).  A device may be listed more than once (its shards then run side by side
 * on it) -- which is also how the path is tested on a one-GPU box: THE COPY BETWEEN TWO PHYSICAL DEVICES HAS NOT RUN YET (see
 * rt_peer_access_log).  Peer access devices[0] <-> devices[k] is enabled on first use where the devices offer it; without it
 * the copies go through host memory.  With RT_FLAG_DETERMINISTIC the result is bit-equal
 * to rt_render's with the same flag, whatever the device list.  stats: counts summed over the shards, times the
 * maximum over the shards, reserved[3] = n_devices.  The calling thread's current device is left as it was.
 * (The process-per-GPU deployment -- rt_render_shard under torch.distributed / RCCL, bench.py -- is the other way to
 * the same image; this entry point is for a C++ driver that wants all GPUs behind one call.) */
int rt_render_multi(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples,
                    int max_bounces, uint64_t seed, uint32_t flags, const int *devices, int n_devices, float *out_rgb,
                    rt_stats *stats);

/* Multi-GPU building block: render only the camera rays owned by path slots
 * [shard_index*W/shard_count, (shard_index+1)*W/shard_count) -- slot s serves exactly the camera
 * rays c with c % W == s, so shards are disjoint and their raw sums add up to the 1-GPU image.
 * d_sum_rgb: DEVICE buffer of width*height*3 floats on the current device; contributions are
 * ADDED to it (zero it first).  stream: hipStream_t (NULL = default stream).  The call is
 * synchronous on that stream when it returns.  shard_count must divide W.
 * (Every render entry point: the scene's BVH records are padded for ray origins within the scene's own bounds; the first
 * render from a camera whose lookfrom lies outside them widens the padding and uploads the records again, once, a few
 * milliseconds.  Thread-safe; the image does not depend on it.) */
int rt_render_shard(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples,
                    int max_bounces, uint64_t seed, int shard_index, int shard_count, uint32_t flags,
                    float *d_sum_rgb, void *stream, rt_stats *stats);

/* Order-independent variant of rt_render_shard: d_sum_fixed is a DEVICE buffer of width*height*3 int64
 * fixed-point sums (units of 2^-30), ADDED to.  Integer adds commute, so the sums of the shards of a
 * multi-GPU render add up to EXACTLY the single-GPU sums and every run gives the same bits (the
 * reference's float atomicAdd, vec3.cuh:149-153, does not).  rt_post_process_fixed converts to the
 * post-processed float image: c = sqrt(float(sum * 2^-30) * (1/spp)). */
int rt_render_shard_fixed(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples,
                          int max_bounces, uint64_t seed, int shard_index, int shard_count, uint32_t flags,
                          int64_t *d_sum_fixed, void *stream, rt_stats *stats);
int rt_post_process_fixed(const int64_t *d_sum_fixed, float *d_rgb_out, int num_pixels, int num_samples, void *stream);

/* post_process_framebuffer (render.cuh:330-338) on a DEVICE buffer: c = sqrt(c * (1/spp)). */
int rt_post_process(float *d_rgb, int num_pixels, int num_samples, void *stream);

/* ---- render along the caller's camera rays (the reference's render() with camera.get_ray() replaced by a table) ----------
 * "Radiance along my rays, from my buffers, on my stream": orthographic, fisheye, lat-long, stereo or thin-lens views, probe
 * and light-map bakes, a pixel filter of one's own.  The estimator never reads the camera after gen() has written (origin,
 * direction, pixel), so the definition is small and exact.  A frame of n_rays camera rays; camera ray c (0 <= c < n_rays)
 *   - is served by path slot c % W, in increasing c per slot, on that slot's XORWOW stream -- exactly as rt_render_shard's;
 *   - starts with the two jitter draws of gen() (x, then y: render.cuh:250-275) made and thrown away.  They cost nothing
 *     and keep every slot's stream where the reference's is, which is what lets the CPU oracle pin this path bit for bit:
 *     a table filled with a pinhole camera's own rays gives rt_render_shard's sums;
 *   - has origin d_origin_xyz[3c ..], direction d_dir_xyz[3c ..] (AoS triples, as the queries take them), tmax = FLT_MAX;
 *   - deposits into pixel d_pixel[c] if d_pixel is given, else into pixel c / rays_per_pixel (render.cuh:257);
 *   - everything after gen() -- init(), mat(), next-event estimation, Russian roulette, the lockstep final generation, the
 *     stop rule, rt_stats -- is unchanged.
 * d_sum_rgb: n_pixels x 3 floats, ADDED to (zero it first); the fixed variant: n_pixels x 3 int64 in units of 2^-30, as
 * rt_render_shard_fixed.  Post-processing stays with the caller (rt_post_process / rt_post_process_fixed take the divisor).
 * All pointers are DEVICE buffers on the scene's device.  The work is ordered on `stream` (NULL = default stream) and the
 * call is synchronous on that stream when it returns; the calling thread's current device is left as it was; the steady path
 * allocates nothing beyond what a render context owns.  Rendering only reads the scene: may overlap queries and renders of
 * the same scene, not rt_scene_update* / rt_scene_rebuild*.
 * flags: 0, RT_FLAG_WATERTIGHT, RT_FLAG_TIME_KERNELS.  Out of scope (an error that names the flag): RT_FLAG_REFERENCE_WALK and
 * RT_FLAG_RNG_PER_SAMPLE -- each would be further builds of the persistent kernel.  No shard parameters either: one device,
 * all W slots.  (A table with a stream per RAY, which splits over calls and devices: rt_render_rays_keyed_device below.)
 * CHECKED ON THE DEVICE BEFORE ANYTHING IS WRITTEN: every direction component finite and below 2^126 in magnitude, no
 * direction other than zero with every component below 2^-60 (as for rt_query_closest_device), every
 * d_pixel[c] in [0, n_pixels) -- the error names the number of offending rays.  Origins outside the radius the scene's
 * records are padded for widen the padding once, as for the queries; a non-finite ORIGIN is legal: that ray misses.
 * Host-side: non-null scene / origins / directions / sum buffer, 1 <= n_rays (below the int32 camera-ray range of
 * rt_render_shard), 1 <= n_pixels <= 715827882, 0 <= max_bounces <= 2^24, and with d_pixel NULL rays_per_pixel >= 1 and
 * (n_rays - 1) / rays_per_pixel < n_pixels.  Every error returns non-zero, sets rt_last_error() and writes nothing. */
int rt_render_rays_device(const rt_scene *scene, int64_t n_rays, const float *d_origin_xyz, const float *d_dir_xyz,
                          const int32_t *d_pixel /* may be NULL */, int rays_per_pixel /* used when d_pixel == NULL */,
                          int n_pixels, int max_bounces, uint64_t seed, uint32_t flags, float *d_sum_rgb, void *stream,
                          rt_stats *stats);
int rt_render_rays_fixed_device(const rt_scene *scene, int64_t n_rays, const float *d_origin_xyz, const float *d_dir_xyz,
                                const int32_t *d_pixel /* may be NULL */, int rays_per_pixel, int n_pixels, int max_bounces,
                                uint64_t seed, uint32_t flags, int64_t *d_sum_fixed, void *stream, rt_stats *stats);

/* ---- keyed ray tables: a stream per ray, so a table splits by key range or stride and the pieces add up exactly ------------
 * The two entry points above tie ray c to slot c % W's stream: a frame is one indivisible call.  Here table row c
 * (0 <= c < n_rays) carries the 64-bit key K = key_first + c * key_stride, and
 *   - its stream is the per-sample stream of (seed, K): exactly that of camera ray G = K of an RT_FLAG_RNG_PER_SAMPLE frame
 *     (splitmix64 of the key, then curand_init's seed scramble: see that flag);
 *   - the first two draws (jitter x, then y) are made and thrown away, as above: a table filled with a pinhole camera's own
 *     per-sample rays gives rt_render_shard_fixed(RT_FLAG_RNG_PER_SAMPLE)'s sums, draw for draw;
 *   - origin and direction are row c, tmax = FLT_MAX;
 *   - it deposits into pixel d_pixel[c] if d_pixel is given, else into pixel K / rays_per_pixel -- by the KEY, not the row:
 *     a chunk that starts mid-pixel, or rank r of R, lands where the whole frame puts it;
 *   - everything after gen() is the per-sample mode's: the path runs to its own end (no lockstep final generation), hits are
 *     RT_FLAG_WATERTIGHT's, a camera ray's contributions are summed in float in path order and added to its pixel once.
 * Sums are ADDED to the buffer, so ANY split of a table -- chunks streamed through one buffer (key_first = first row of the
 * chunk, key_stride = 1), rank r of R (key_first = r, key_stride = R, the rows G = r mod R), passes of a progressive render --
 * gives, in the fixed variant, EXACTLY the int64 sums of the whole frame, in any order.
 * flags: 0, RT_FLAG_TIME_KERNELS; RT_FLAG_RNG_PER_SAMPLE and RT_FLAG_WATERTIGHT are accepted and change nothing (both are what
 * the mode is); RT_FLAG_REFERENCE_WALK and any other bit is an error that names the flag.
 * Checks: those of rt_render_rays_device (host and device, before anything is written), and key_stride >= 1, the last key
 * key_first + (n_rays - 1) * key_stride does not wrap 2^64, and with d_pixel NULL rays_per_pixel >= 1 and the last key's
 * pixel < n_pixels.  A scene with 2-wide nodes (RT_BVH_WIDE=0), or a process without the persistent kernel (RT_PERSISTENT=0),
 * is an error: the per-sample mode runs on k_paths only.  Every error returns non-zero, names the entry point in
 * rt_last_error() and writes nothing. */
int rt_render_rays_keyed_device(const rt_scene *scene, int64_t n_rays, const float *d_origin_xyz, const float *d_dir_xyz,
                                const int32_t *d_pixel /* may be NULL */, int rays_per_pixel /* used when d_pixel == NULL */,
                                int n_pixels, int max_bounces, uint64_t seed, uint64_t key_first, uint32_t key_stride,
                                uint32_t flags, float *d_sum_rgb, void *stream, rt_stats *stats);
int rt_render_rays_keyed_fixed_device(const rt_scene *scene, int64_t n_rays, const float *d_origin_xyz, const float *d_dir_xyz,
                                      const int32_t *d_pixel /* may be NULL */, int rays_per_pixel, int n_pixels, int max_bounces,
                                      uint64_t seed, uint64_t key_first, uint32_t key_stride, uint32_t flags,
                                      int64_t *d_sum_fixed, void *stream, rt_stats *stats);

/* ---- counted frames: a sample count per pixel, so samples go where the error is and the passes add up exactly --------------
 * Every entry point above takes one num_samples for the whole image.  Here pixel p (0 <= p < width * height) renders the
 * samples k = d_first[p] .. d_first[p] + d_count[p] - 1 (d_first NULL: all 0) of the RT_FLAG_RNG_PER_SAMPLE frame
 * (width, height, num_samples = sample_stride, seed):
 *   - sample k of pixel p IS camera ray G = p * sample_stride + k of that frame: its stream is the per-sample stream of
 *     (seed, G) with a 64-bit key (sample_stride may be as large as 2^31 - 1), it draws jitter x then y, makes the pinhole ray,
 *     runs its path to its own end with RT_FLAG_WATERTIGHT's hits, sums its contributions in float in path order and adds them
 *     to its pixel once;
 *   - d_first and d_count are device arrays of width * height int32; d_sum_fixed is width * height * 3 int64 in units of 2^-30
 *     and is ADDED to; d_samples, if given, is width * height int32 and gets d_count[p] ADDED: the divisor a caller keeps over
 *     several passes (rt_normalize_counts_fixed, rt_post_process_counts_fixed below).
 * Three promises follow from the definition, and the tests hold them:
 *   WHOLE FRAME  with d_first NULL and every count equal to sample_stride, the sums and the six event totals are those of
 *                rt_render_shard_fixed(..., num_samples = sample_stride, shard 0 of 1, RT_FLAG_RNG_PER_SAMPLE), bit for bit;
 *   TILING       any set of calls whose ranges [first, first + count) tile [0, sample_stride) for every pixel gives exactly
 *                those sums, in any order: progressive passes, a base pass and an adaptive one, rank r of R on another device;
 *   KEYED TABLE  a call equals rt_render_rays_keyed_fixed_device on the table that lists the same keys.
 * rt_stats: camera_rays is the sum of the counts; the samples of a pixel through which no ray can hit the scene are counted as
 * in the per-sample camera path (camera_rays, closest_rays) and passed over without a stream or a ray; everything else is the
 * per-sample mode's.
 * flags: 0, RT_FLAG_TIME_KERNELS; RT_FLAG_RNG_PER_SAMPLE and RT_FLAG_WATERTIGHT are accepted and change nothing (both are what
 * the mode is); RT_FLAG_REFERENCE_WALK and any other bit is an error that names the flag.  A scene with 2-wide nodes
 * (RT_BVH_WIDE=0), or a process without the persistent kernel (RT_PERSISTENT=0), is an error, as for the keyed tables.
 * Checks.  Host-side: non-null scene, camera, d_count and d_sum_fixed; 1 <= sample_stride <= 2^31 - 1; width, height >= 1 and
 * width * height <= 715827882; 0 <= max_bounces <= 2^24.  On the device, before anything is written: d_count[p] >= 0,
 * d_first[p] >= 0 and d_first[p] + d_count[p] <= sample_stride (without int32 overflow) for every pixel -- the error names the
 * number of offending pixels -- and the sum of the counts stays below the camera-ray range of rt_render_shard (ids within
 * 13 * 2^20 of 2^31).  Every error returns non-zero, names rt_render_counts_fixed in rt_last_error() and writes nothing.
 * A sum of 0 is legal: the call returns 0, writes nothing and reports zero events.
 * The work is ordered on `stream` and complete when the call returns; the current device is left as it was; once the render
 * context owns its scratch for this image size (width * height + 1 words) the call allocates nothing.
 * Out of scope: count maps for ray tables and for the AOV, follow and motion kernels; a float-atomic framebuffer variant;
 * a helper that splits a count map over ranks (a rank passes its own d_first / d_count). */
int rt_render_counts_fixed(const rt_scene *scene, const rt_camera *camera, int width, int height, int sample_stride,
                           const int32_t *d_first /* may be NULL: all 0 */, const int32_t *d_count, int max_bounces,
                           uint64_t seed, uint32_t flags, int64_t *d_sum_fixed, int32_t *d_samples /* may be NULL */,
                           void *stream, rt_stats *stats);

/* Sums with a per-pixel divisor -> the format the temporal accumulators emit: int64 sums of ONE sample of the mean, so that
 * rt_denoise_fixed(out, 1, aov, aov_spp, ...), rt_denoise_variance_fixed and the accumulators take an adaptive frame unchanged.
 * Per channel, with n = d_samples[p]: n == 0 gives 0, otherwise sign(s) * ((|s| + (n >> 1)) / n) in exact 64-bit integer
 * arithmetic (n == 1: the identity).  In place (d_out_fixed == d_sum_fixed) is allowed.  A negative n is an error, checked on
 * the device before anything is written (the message names the number of such pixels); the call waits for that check. */
int rt_normalize_counts_fixed(const int64_t *d_sum_fixed, const int32_t *d_samples, int num_pixels, int64_t *d_out_fixed,
                              void *stream);
/* rt_post_process_fixed with the pixel's own count where that has num_samples: sqrt(float(sum * 2^-30) * (1 / float(n))), the
 * same operations in the same order; n <= 0 gives 0.  Asynchronous on `stream`. */
int rt_post_process_counts_fixed(const int64_t *d_sum_fixed, const int32_t *d_samples, int num_pixels, float *d_rgb_out,
                                 void *stream);

/* From a weight map to counts under a budget, in exact integer arithmetic (what the weight means stays with the caller: the
 * documented loop uses the relative standard deviation from rt_temporal_accumulate_moments_fixed's variance plus a floor):
 *   q[p]     = 0 unless w > 0 (NaN, zero, negatives), else (uint64) floorf(fminf(w, 4096.f) * 1048576.f): exact in fp32, <= 2^32
 *   T        = the sum of q[p] as a 64-bit integer
 *   extra    = budget - num_pixels * min_count
 *   count[p] = min(max_count, min_count + (T ? (extra * q[p]) / T : extra / num_pixels))
 *   *total_out (host) = the sum of count[p] <= budget.
 * What flooring and the cap leave over is NOT redistributed: *total_out says how much of the budget was placed.
 * Errors (nothing is written): a null pointer, num_pixels < 1, min_count < 0, max_count < min_count, extra < 0, extra >= 2^31.
 * Ordered on `stream`; the call waits for the total. */
int rt_sample_allocate(const float *d_weight, int num_pixels, int min_count, int max_count, int64_t budget,
                       int32_t *d_count_out, int64_t *total_out /* host */, void *stream);

/* ---- first-hit feature buffers (AOVs): albedo, normal, emission, depth, coverage per pixel, and object ids ----------------
 * What a denoiser, a compositor or a learning pipeline takes next to the noisy image, from one kernel that makes the ray,
 * finds the hit and deposits the features: no ray table, no round trip (no reference counterpart: its render() writes
 * radiance only).  An AOV frame of (camera, width, height, num_samples, seed) has the samples G = 0 .. width * height *
 * num_samples - 1:
 *   1. THE RAY of sample G is camera ray G of an RT_FLAG_RNG_PER_SAMPLE frame: pixel G / num_samples, the stream of (seed, G),
 *      jitter = its first two draws (x, then y), ray = camera.get_ray((px + jx) / width, (py + jy) / height), operation for
 *      operation.  No further draw is made.  An AOV frame and an RT_FLAG_RNG_PER_SAMPLE | RT_FLAG_WATERTIGHT beauty frame of the
 *      same seed therefore use the same camera ray, sample for sample.
 *   2. SHARDS: shard (r, R) with num_samples % R == 0 serves the samples with G % R == r, as that mode's shards do.
 *   3. THE HIT is the closest hit with tmax = FLT_MAX under `flags`, exactly as rt_query_closest_device defines them: 0 (the
 *      reference's decisions: visibility check, tie rule, literal re-trace), RT_FLAG_REFERENCE_WALK or RT_FLAG_WATERTIGHT.
 *      Both tree widths are served.
 *   4. THE DEPOSIT: a sample that misses deposits nothing.  A sample that hits triangle k ADDS to its pixel, each value
 *      converted to fixed point (units of 2^-30, int64, magnitudes clamped to 2^31 as rt_render_shard_fixed's):
 *        channels 0-2  albedo    the albedo of the triangle's material, whatever its type
 *        channels 3-5  normal    n = -unit(tri.n), the record mat() shades with (render.cuh:153), faced to the viewer:
 *                                dot(n, d) > 0 ? -n : n, with dot = x*x + y*y + z*z left to right, every operation rounded
 *        channels 6-8  emission  L of the area light the triangle carries, else 0: what init() deposits at bounce 0
 *                                (render.cuh:98-103)
 *        channel  9    depth     t of the hit
 *        channel  10   hits      the integer 1 (a count, not scaled)
 *      d_aov_fixed is n_pixels x RT_AOV_CHANNELS int64, interleaved per pixel, ADDED to (zero it first).  A channel whose
 *      value is 0 is not added.
 *   5. IDS (d_ids may be NULL): n_pixels x 2 int32.  The sample with G % num_samples == 0 writes {triangle in the caller's
 *      order, material index} of its hit, or {-1, -1} on a miss, with a plain store.  Such a sample belongs to shard 0, so
 *      the other shards write nothing there.  (Mirror and glass are not followed to the first diffuse vertex here: the material
 *      index tells the caller that a pixel is specular, and rt_render_aov_follow_fixed below follows them.)
 *   6. THE RAY-TABLE FORM (rt_render_aov_rays_fixed_device): row c has the key K = key_first + c * key_stride, exactly as
 *      rt_render_rays_keyed_device defines keys and their checks.  Origin and direction are row c; no stream is needed.  The
 *      pixel is d_pixel[c], else K / rays_per_pixel.  Ids are written by the rows with K % rays_per_pixel == 0, and only when
 *      d_pixel is NULL: d_ids together with d_pixel is an error.  The device prepasses of the ray tables (directions, pixel
 *      range, origin radius) run before anything is written.
 *   7. RESOLVE (rt_aov_resolve): n_pixels x RT_AOV_CHANNELS floats from the sums.  With s = float(double(sum) * 2^-30), as
 *      rt_post_process_fixed forms it, and inv = 1.f / num_samples: albedo, normal and emission are s * inv (the mean normal
 *      is not renormalised); depth is hits > 0 ? s / float(hits) : 0; channel 10 is float(hits) * inv (coverage).
 * WHAT FOLLOWS: the sums are integers, so any split of a frame -- shards, key ranges, chunks in any order -- adds up to
 * exactly the whole frame; the camera form and a table that holds the pinhole's own per-sample rays give the same integers;
 * with RT_FLAG_WATERTIGHT the emission channels are the fixed-point sums of the per-sample frame at max_bounces = 0.
 * The contract is the neighbouring entry points': all buffers are DEVICE buffers on the scene's device; the work is ordered on
 * `stream` (NULL = default stream) and the call is synchronous on it at return; the calling thread's current device is left
 * as it was; the steady path allocates nothing (the scratch words, the overflow stacks and the timing events belong to the
 * scene's query state, so AOV calls and queries of ONE scene take turns); only the scene is read; a camera or origins outside
 * the radius the records are padded for widen the padding once.
 * stats (may be NULL): camera_rays and closest_rays = the samples of this call, seconds_render = device time of the kernel,
 * bvh_nodes, bvh_depth, and with flags 0 reserved[4..6] = the rare-path counters as rt_render_shard fills them.
 * ERRORS return non-zero, name the entry point in rt_last_error() and write nothing: a null pointer that may not be null;
 * width, height or num_samples < 1, more than 715827882 pixels, width * height * num_samples beyond the int32 camera-ray range
 * of rt_render_shard; shard_index outside 0 .. shard_count - 1 or num_samples % shard_count != 0; a flag other than
 * RT_FLAG_WATERTIGHT, RT_FLAG_REFERENCE_WALK or RT_FLAG_TIME_KERNELS (accepted, changes nothing), or both hit flags together;
 * the table checks of rt_render_rays_keyed_device (n_rays, n_pixels, key_stride, a key that wraps, the last key's pixel, and on
 * the device the directions and the pixel indices: the error names the number of offending rays). */
#define RT_AOV_CHANNELS 11
enum { RT_AOV_ALBEDO = 0, RT_AOV_NORMAL = 3, RT_AOV_EMISSION = 6, RT_AOV_DEPTH = 9, RT_AOV_HITS = 10 };
int rt_render_aov_fixed(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples, uint64_t seed,
                        int shard_index, int shard_count, uint32_t flags, int64_t *d_aov_fixed,
                        int32_t *d_ids /* may be NULL */, void *stream, rt_stats *stats /* may be NULL */);
int rt_render_aov_rays_fixed_device(const rt_scene *scene, int64_t n_rays, const float *d_origin_xyz, const float *d_dir_xyz,
                                    const int32_t *d_pixel /* may be NULL */, int rays_per_pixel, int n_pixels,
                                    uint64_t key_first, uint32_t key_stride, uint32_t flags, int64_t *d_aov_fixed,
                                    int32_t *d_ids /* may be NULL */, void *stream, rt_stats *stats /* may be NULL */);
int rt_aov_resolve(const int64_t *d_aov_fixed, float *d_out, int n_pixels, int num_samples, void *stream);

/* ---- followed AOVs: the features of the first non-specular vertex behind mirror and glass -----------------------------------
 * The same eleven channels, so every consumer of an AOV buffer (rt_denoise_fixed, rt_denoise_dual_fixed,
 * rt_denoise_variance_fixed, both temporal accumulators, rt_aov_resolve) takes them unchanged -- but on a mirror or a glass
 * surface the guides describe what is SEEN in it.  Samples, rays, shards, keys, hit flags, the
 * fixed-point conversion, "a zero channel is not added", the device checks, the errors and the stream / thread contract are
 * those of rt_render_aov_fixed / rt_render_aov_rays_fixed_device above.  New:
 *   1. THE FOLLOWED PATH of sample G is the path of sample G of the RT_FLAG_RNG_PER_SAMPLE beauty frame of the same seed, draw
 *      for draw.  Vertex 0 is the first hit.  While the material at vertex j is MIRROR or GLASS and j < max_specular, the
 *      sample takes the step mat() takes there (render.cuh:139-248): n = -unit(tri.n) of the hit triangle,
 *      f = sample_f(material, wo = d_j, stream, n, wi, pdf), the next ray starts at offset_ray_origin(p(u, v), n) with
 *      direction wi and tmax = FLT_MAX, and beta = beta * ((f * dot(wi, n)) / pdf), from beta = (1, 1, 1).
 *   2. THE STREAM is that of (seed, G), continued after the two jitter draws; in the table form that of (seed, K) with its first
 *      two draws made and thrown away, as rt_render_rays_keyed_device does.  After sample_f the stream is advanced by the draws
 *      that mat() makes at that vertex and whose values the features do not need: none in a scene without lights; otherwise
 *      the light-pick draw (its value selects the light), and for an area light the two draws of Triangle::sample_p and the
 *      draws of the second sample_f call (none for a mirror; one for glass that can refract).  A point light draws no more.
 *   3. NO RUSSIAN ROULETTE: init() first rolls at bounces > RR_START = 4, and the last vertex shaded here has
 *      bounces = max_specular - 1 <= 4.  That is why RT_AOV_FOLLOW_MAX is 5.
 *   4. THE NEXT HIT is the closest hit under the call's hit flags; with RT_FLAG_WATERTIGHT the chain is the beauty frame's own.
 *   5. THE DEPOSIT of a sample whose chain ends at vertex j -- the material there is not specular, or j == max_specular:
 *        albedo    beta * albedo(material_j), one rounded product per channel (j = 0: beta is exactly 1, today's bits)
 *        normal    -unit(tri.n) of vertex j, faced against the arriving direction d_j by rule 4 of the first-hit buffers
 *        depth     ((t_0 + t_1) + ...) + t_j in fp32: the length of the path
 *        hits      1
 *        emission  L of the area light that the FIRST hit's triangle carries (the estimator adds emission at bounce 0 only)
 *      A chain that leaves the scene behind a specular vertex deposits that emission and nothing else: hits is not incremented
 *      (its beauty sample carries nothing but that emission).  A first ray that misses deposits nothing.
 *   6. IDS keep {triangle, material} of the FIRST hit: the material index still tells the caller that a pixel is specular.
 *   7. max_specular = 0 is rt_render_aov_fixed / rt_render_aov_rays_fixed_device bit for bit, sums and ids (the same kernel;
 *      the table form's seed is then not used).  max_specular outside 0 .. RT_AOV_FOLLOW_MAX is an error.
 * stats: camera_rays = the samples of this call, closest_rays = all rays traced, chain rays included; the rest as above.
 * Motion vectors are NOT followed: rt_render_motion reprojects the surface a pixel is seen on. */
#define RT_AOV_FOLLOW_MAX 5
int rt_render_aov_follow_fixed(const rt_scene *scene, const rt_camera *camera, int width, int height, int num_samples,
                               uint64_t seed, int shard_index, int shard_count, uint32_t flags, int max_specular,
                               int64_t *d_aov_fixed, int32_t *d_ids /* may be NULL */, void *stream,
                               rt_stats *stats /* may be NULL */);
int rt_render_aov_follow_rays_fixed_device(const rt_scene *scene, int64_t n_rays, const float *d_origin_xyz,
                                           const float *d_dir_xyz, const int32_t *d_pixel /* may be NULL */, int rays_per_pixel,
                                           int n_pixels, uint64_t seed, uint64_t key_first, uint32_t key_stride, uint32_t flags,
                                           int max_specular, int64_t *d_aov_fixed, int32_t *d_ids /* may be NULL */, void *stream,
                                           rt_stats *stats /* may be NULL */);

/* ---- the denoiser: an AOV-guided a-trous wavelet filter on fixed-point frames ----------------------------------------------
 * One more call after rt_render_shard_fixed and rt_render_aov_fixed: the beauty sums and the feature sums of one view become
 * a clean image, on the same device and stream (no reference counterpart).  An edge-avoiding a-trous filter (Dammertz et al.
 * 2010) on albedo-demodulated radiance, guided by the first-hit normal and depth.  The whole filter is ONE STATED SEQUENCE of
 * individually rounded fp32 operations (no FMA; the library is built with -ffp-contract=off), so the kernels, the CPU twin
 * (hc_denoise of librt_hostcheck.so) and the numpy restatement of the tests agree in every bit.
 * "x > t ? x : t" below is that comparison and selection, not fmax (the inputs cannot be NaN; the sign of a zero is the
 * selection's).  Sums start at 0.f.
 *   1. INPUTS per pixel.  c = float(double(sum) * 2^-30) * (1.f / num_samples) per channel of d_sum_fixed (what
 *      rt_post_process_fixed forms before its sqrt).  The features are exactly what rt_aov_resolve gives for aov_samples:
 *      albedo a, normal n (the mean, not renormalised), emission e, depth z (the mean over the hits, 0 on a pixel with none).
 *      Fixed-point sums are finite, so no input is NaN or infinite.
 *   2. DEMODULATE.  d = a > 2^-10 ? a : 2^-10 per channel; t = c - e; u = (t > 0 ? t : 0) / d, a true division.  First-hit
 *      emission is free of noise and is kept out of the filter.
 *   3. PASSES i = 0 .. passes - 1 with stride s = 2^i, each from one buffer of u to another (a pass never reads what it
 *      writes).  For pixel p visit the 25 taps q = p + s * (dx, dy), dy outer and dx inner, both from -2 to 2; a tap outside
 *      the image is skipped.  h = k[dx] * k[dy] with k = {1/16, 1/4, 3/8, 1/4, 1/16} (exact products).  The centre tap has the
 *      weight h.  Every other tap has w = (h * rt_expnegf(-(x_c + x_z))) * w_n with
 *          x_c = ((du.x * du.x + du.y * du.y) + du.z * du.z) * kc_i,   du = u_q - u_p,
 *          kc_i = float(4^i) / (sigma_color * sigma_color)   (made on the host: sigma_color halves every pass),
 *          x_z = (dz * dz) * kz,   dz = z_q - z_p,   kz = 1.f / (sigma_depth * sigma_depth),
 *          w_n = (t > 0 ? (t < 1 ? t : 1) : 0) squared normal_power_log2 times,
 *                                                        t = (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z.
 *      (Means of unit normals have t <= 1 up to rounding; the upper clamp keeps every weight at or below h whatever the sums
 *      hold, so no sum overflows and no NaN can arise -- a NaN's bits would differ between processors.)
 *      sw = sw + w and su = su + w * u_q per channel, in tap order; the pixel's new u is su / sw per channel (the centre
 *      weight is positive, so sw is).  z and n do not change.
 *   4. REMODULATE.  out = u * d + e per channel: LINEAR MEAN RADIANCE.  A caller who wants the reference's display transform
 *      calls rt_post_process(d_rgb_out, width * height, 1, stream) afterwards.
 *   5. rt_expnegf(x) (rt_pinned_math.h), x <= 0: exactly 0 for x <= -87 and for NaN (an overflowing x_c therefore gives the
 *      weight 0); else kf = floor(x * 1.44269504f + 0.5f); r = x - kf * 0.693359375f; r = r - kf * -2.12194440e-4f;
 *      p = 1.9875691500e-4f, then p = p * r + c for c = 1.3981999507e-3f, 8.3334519073e-3f, 4.1665795894e-2f,
 *      1.6666665459e-1f, 5.0000001201e-1f; y = (p * (r * r) + r) + 1.f; the result is y * 2^kf, 2^kf built from its bits.
 *      Exactly 1 at 0; within 2 ulp of exp.
 * rt_denoise_params: NULL = the defaults, which rt_denoise_default_params writes (chosen on the CPU against 1024-spp frames:
 * profiles/denoise_quality.json).
 * d_scratch: rt_denoise_scratch_bytes(width, height) bytes (48 per pixel: {u, z} twice, {n} once), 16-byte aligned, the
 * caller's; its contents before the call do not matter and are undefined after it.
 * The contract is the neighbouring entry points': all buffers are DEVICE buffers on the current device; the work is ordered on
 * `stream` (NULL = default stream) and the call is synchronous on it at return; the calling thread's current device is left as
 * it was; nothing is allocated; the two input buffers are only read; every pixel of d_rgb_out is written.
 * ERRORS return non-zero, name the entry point in rt_last_error() and write nothing: a null pointer other than params; width or
 * height < 1 or more than 715827882 pixels; num_samples or aov_samples < 1; a scratch pointer that is not 16-byte aligned;
 * passes or normal_power_log2 outside 0 .. 8; a sigma that is not finite and positive, or whose kc_i (for an i < passes) or kz
 * is not finite and positive; flags != 0; with passes >= 1, a frame so narrow or so flat that a pass would need more than
 * 16777215 workgroups of 32 x 8 pixels (a launch holds fewer than 2^32 threads: a 1 x 7 * 10^8 frame is refused, any frame
 * with both sides of 32 or more is served).  "Writes nothing" is the guarantee for these ARGUMENT errors, all found before the
 * first launch; should a launch or the synchronisation itself fail in the runtime, the call returns its message and the
 * scratch and the output are undefined.  rt_denoise_scratch_bytes returns a negative number for sizes < 1 or beyond the
 * pixel limit. */
typedef struct rt_denoise_params {
    int32_t passes;             /* 0 .. 8; pass i uses tap stride 2^i */
    float   sigma_color;        /* > 0; halves every pass */
    float   sigma_depth;        /* > 0; scene units */
    int32_t normal_power_log2;  /* 0 .. 8: w_n = min(max(0, n_p . n_q), 1) squared this many times */
    uint32_t flags;             /* must be 0 */
} rt_denoise_params;
int64_t rt_denoise_scratch_bytes(int width, int height);
int rt_denoise_default_params(rt_denoise_params *out);
int rt_denoise_fixed(const int64_t *d_sum_fixed, int num_samples, const int64_t *d_aov_fixed, int aov_samples, int width,
                     int height, const rt_denoise_params *params /* NULL = defaults */, void *d_scratch,
                     float *d_rgb_out /* width * height * 3 */, void *stream);

/* ---- the dual-buffer denoiser: variance-guided a-trous from two half frames ----------------------------------------------------
 * rt_denoise_fixed's filter with the fixed sigma_color replaced by a per-pixel noise estimate (the spatial part of SVGF, Schied
 * et al. 2017).  The caller renders the view as two half frames A and B -- with RT_FLAG_RNG_PER_SAMPLE, shard (r, 2) of
 * rt_render_shard_fixed into two zeroed buffers: their sum is the whole frame exactly -- and one rt_render_aov_fixed.  The
 * difference of the halves gives, per pixel, an unbiased estimate of the variance of their mean; a colour distance is then
 * measured in standard deviations of that estimate, so a firefly (large variance) is absorbed where a fixed colour stop would
 * protect it as an edge.  ONE STATED SEQUENCE again: every operation below is one rounded fp32 operation, no FMA, every
 * "x > t ? x : t" a comparison and selection, sums start at 0.f; kernels, CPU twin (hc_denoise_dual) and the tests' numpy
 * restatement agree in every bit.
 *   1. INPUTS per pixel.  S = sum_a + sum_b per channel, a two's-complement WRAPPING add (done in uint64_t: every pair of inputs
 *      is defined); n = samples_a + samples_b.  c, d, e, z, the normal and u are exactly steps 1 and 2 of rt_denoise_fixed for
 *      (S, n): with passes = 0 the output is rt_denoise_fixed's on the summed buffer, bit for bit.  u_a and u_b are formed the
 *      same way from (sum_a, samples_a) and (sum_b, samples_b) with the same d and e:
 *      u_a = (t > 0 ? t : 0) / d, t = float(double(sum_a) * 2^-30) * (1.f / samples_a) - e.
 *   2. VARIANCE OF THE MEAN, summed over the channels of demodulated radiance:
 *          v = (((u_a.x - u_b.x)^2 + (u_a.y - u_b.y)^2) + (u_a.z - u_b.z)^2) * kv,
 *      each difference and each square rounded; kv = float(double(samples_a) * samples_b / (double(n) * n)), made on the host
 *      (1/4 for equal halves).
 *   3. PASSES i = 0 .. passes - 1 with stride s = 2^i, each from one buffer of {u, v} to another.  For pixel p:
 *      a. the 3 x 3 prefilter of the variance on the pass's INPUT: taps at stride 1 whatever s is, dy outer and dx inner, both
 *         from -1 to 1, taps outside the image skipped, k3 = {1/4, 1/2, 1/4} (exact products):
 *         sg = sg + (k3[dx] * k3[dy]) * v_q, sk = sk + k3[dx] * k3[dy]; g = sg / sk.
 *      b. r = 1.f / (ks * g + 2^-26), ks = sigma_variance * sigma_variance made on the host.  One division per pixel.
 *      c. the 25 taps in rt_denoise_fixed's order with its skip rule, h = k[dx] * k[dy].  The centre tap has the weight h.
 *         Every other tap has w = (h * rt_expnegf(-(x_v + x_z))) * w_n with
 *             x_v = ((du.x * du.x + du.y * du.y) + du.z * du.z) * r,   du = u_q - u_p,
 *         and x_z, w_n as in rt_denoise_fixed (kz = 1.f / (sigma_depth * sigma_depth); w_n clamped to 0 .. 1).
 *      d. per tap, in order: sw = sw + w; su = su + w * u_q per channel; sv = sv + (w * w) * v_q (the centre tap contributes
 *         (h * h) * v_p).  New u = su / sw per channel; new v = sv / (sw * sw).  z and n do not change.
 *   4. REMODULATE.  out = u * d + e per channel: linear mean radiance, as rt_denoise_fixed leaves it.
 * FINITENESS.  |sum| * 2^-30 <= 2^33 and d >= 2^-10, so 0 <= u, u_a, u_b <= 2^43 and v <= 3 * 2^86 * kv < 2^87.  sk is at
 * least 1/4 (a one-pixel image) and g is a weighted mean of v: finite and not negative.  ks * g may overflow to +inf (r = 0:
 * the colour stop vanishes, x_v = 0) or underflow to 0 (r = 2^26), so 0 <= r <= 2^26 and x_v <= 3 * 2^86 * 2^26 < 2^128: no
 * inf - inf and no 0 * inf anywhere; x_v + x_z may be +inf, which rt_expnegf maps to the weight 0.  Weights are at most h,
 * sw >= 9/64 (the centre), the new u is a weighted mean of the taps' u, and the new v is at most the largest v of the taps
 * times (sum of w^2) / (sum of w)^2 <= 1, up to rounding.  Products w * w and (w * w) * v may be denormal or underflow to 0;
 * that is defined and the same on every processor the library runs on.  No NaN can arise from any finite sums.
 * d_sum_a == d_sum_b is legal: v = 0 everywhere, r = 2^26, and only taps whose u equals the centre's to within 2^-13 carry weight.
 * rt_denoise_dual_params: NULL = the defaults, which rt_denoise_dual_default_params writes (chosen on the CPU against 1024-spp
 * frames: profiles/denoise_dual_quality.json).
 * d_scratch: rt_denoise_dual_scratch_bytes(width, height) bytes (52 per pixel: {u, v} twice, {n, z} once, r once), 16-byte
 * aligned, the caller's; its contents before the call do not matter and are undefined after it.  (The r array is written only
 * by passes that take r from a kernel of their own before the pass -- as built, the pass of stride 2 -- and is otherwise left
 * untouched; every other pass forms r inside the pass.)
 * The contract, the size limits and the error style are rt_denoise_fixed's: device buffers on the current device, ordered on
 * `stream` and synchronous on it at return, nothing allocated, inputs only read, every pixel of d_rgb_out written.  ERRORS
 * return non-zero, begin "rt_denoise_dual_fixed: " in rt_last_error() and write nothing: rt_denoise_fixed's list with
 * sigma_variance in the place of sigma_color, and also samples_a or samples_b < 1, samples_a + samples_b beyond int32, a
 * sigma_variance that is not finite and positive or whose ks is not. */
typedef struct rt_denoise_dual_params {
    int32_t passes;             /* 0 .. 8; pass i uses tap stride 2^i */
    float   sigma_variance;     /* > 0: colour distances are measured in standard deviations of the local estimate */
    float   sigma_depth;        /* > 0; scene units */
    int32_t normal_power_log2;  /* 0 .. 8 */
    uint32_t flags;             /* must be 0 */
} rt_denoise_dual_params;
int64_t rt_denoise_dual_scratch_bytes(int width, int height);
int rt_denoise_dual_default_params(rt_denoise_dual_params *out);
int rt_denoise_dual_fixed(const int64_t *d_sum_a, int samples_a, const int64_t *d_sum_b, int samples_b,
                          const int64_t *d_aov_fixed, int aov_samples, int width, int height,
                          const rt_denoise_dual_params *params /* NULL = defaults */, void *d_scratch,
                          float *d_rgb_out /* width * height * 3 */, void *stream);

/* ---- temporal accumulation: a motion buffer and the reprojected history ----------------------------------------------------------
 * The temporal part of SVGF (Schied et al. 2017) for a sequence of frames: where the surface point under a pixel was one frame ago
 * (rt_render_motion), and the blend of the new frame into the history found there (rt_temporal_accumulate_fixed).  No reference
 * counterpart.  THE ACCUMULATED FRAME HAS THE FORMAT OF A RENDERED FRAME: int64 sums in units of 2^-30 that stand for ONE sample
 * of the accumulated mean, so both denoisers run on it unchanged with num_samples = 1, and two half frames accumulated with the
 * same taps and weights stay two independent estimates of one mean: rt_denoise_dual_fixed(hist_a, 1, hist_b, 1, ...) sees the
 * variance shrink as the history grows.  The loop of one frame:
 *     rt_render_shard_fixed  (RT_FLAG_RNG_PER_SAMPLE, shards (0, 2) and (1, 2) into two zeroed buffers, a new seed per frame)
 *       -> rt_render_aov_fixed
 *       -> rt_render_motion
 *       -> rt_temporal_accumulate_fixed
 *       -> rt_denoise_dual_fixed(hist_a_out, 1, hist_b_out, 1, aov, ...)
 * (with one buffer the last stage is rt_denoise_fixed(hist_a_out, 1, ...)); the `out` buffers of frame N, and its AOV sums, are
 * the `in` buffers of frame N + 1: the caller ping-pongs two sets.
 * Both definitions are ONE STATED SEQUENCE of individually rounded fp32 operations (no FMA), every max or min a comparison and
 * selection, dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z as everywhere, cross as rt_device.h's (a.y * b.z - a.z * b.y, ...);
 * the kernels, the CPU twins (hc_motion_records, hc_temporal_accumulate of librt_hostcheck.so: rt_temporal.h is their shared
 * arithmetic) and the numpy restatement of the tests agree in every bit.
 *
 * rt_render_motion.  Pixel p = py * width + px of d_motion (width * height records of 4 floats, 16-byte aligned):
 *   1. THE RAY is camera.get_ray((px + 0.5f) / width, (py + 0.5f) / height): the operations of rt_render_aov_fixed's ray with
 *      both jitters equal to 0.5f.  No stream is drawn.
 *   2. THE HIT is the closest hit with tmax = FLT_MAX under `flags`, exactly as rt_query_closest_device defines it: 0,
 *      RT_FLAG_REFERENCE_WALK or RT_FLAG_WATERTIGHT; RT_FLAG_TIME_KERNELS is accepted and changes nothing; both hit flags
 *      together, or any other bit, is an error.  Both tree widths are served.
 *   3. A MISS writes {0.f, 0.f, 0.f, the bits of int32 -1}.
 *   4. A HIT on triangle k (the caller's order) with barycentrics (u, v): the PREVIOUS position of that surface point is
 *      tri_point on the previous vertices q0, q1, q2 = row k of d_prev_tri_p0p1p2: e1 = q0 - q1, e2 = q2 - q0 per component, then
 *      P = (q0 - e1 * u) + e2 * v.  With d_prev_tri_p0p1p2 NULL (the vertices did not move) the scene's own stored record
 *      {p0, e1, e2} is used: the same operations on the current vertices.
 *   5. THE PROJECTION into prev_camera (primed: its fields):  a = P - lookfrom';  A = upper_left' - lookfrom';
 *      m = cross(horizontal', vertical');  lam = dot(A, m) / dot(a, m);  r = a * lam - A;
 *      sx = (dot(r, horizontal') / dot(horizontal', horizontal')) * float(width);
 *      sy = (dot(r, vertical') / dot(vertical', vertical')) * float(height);  dist = sqrt(dot(a, a)).
 *   6. VALIDITY: if lam > 0 and lam is finite the record is {sx, sy, dist, the bits of k}; otherwise the point is behind or beside
 *      the previous pinhole and the record is {-1.f, -1.f, dist, the bits of k}.
 *   7. sx and sy are continuous pixel coordinates: the centre of pixel (x, y) is (x + 0.5, y + 0.5).
 * Every record is written with a plain store.  stats (may be NULL) is filled as rt_render_aov_fixed fills it, for width * height
 * rays.  The contract is the AOV entry points': device buffers on the scene's device, ordered on `stream` (NULL = default stream)
 * and synchronous on it at return, the current device left as it was, nothing allocated on the steady path -- the scratch words,
 * the overflow stacks and the timing events belong to the scene's query state, so MOTION CALLS, QUERIES AND AOV CALLS OF ONE SCENE
 * TAKE TURNS -- and a camera whose lookfrom lies outside the radius the records are padded for widens the padding once.
 * ERRORS return non-zero, begin "rt_render_motion: " in rt_last_error() and write nothing: a null scene, camera, prev_camera or
 * d_motion; width or height < 1; more than 715827882 pixels; the flags above; a d_motion that is not 16-byte aligned.  (Previous
 * vertices are read by the caller's index, so a 2-wide RT_BVH_WIDE=0 scene serves them too.)
 * OUT OF SCOPE: ray-table cameras; a previous triangle set of another count (d_prev_tri_p0p1p2 has the scene's count); following
 * mirror or glass to the first diffuse vertex (the record is the first hit's, as the AOVs' are).
 *
 * rt_temporal_accumulate_fixed.  Per pixel p = (x, y), for each supplied colour buffer k in {a, b} (d_sum_b, d_hist_b_in -- when
 * history is given -- and d_hist_b_out are NULL together):
 *   1. INPUTS.  c_k = float(double(sum_k) * 2^-30) * (1.f / samples_k) per channel.  n_p is the mean normal of this frame's AOV
 *      sums, exactly as rt_aov_resolve forms it for aov_samples.  (sx, sy, dist, tri) is the pixel's motion record.
 *   2. NO HISTORY: the output is to_fixed(c_k) per channel and len = 1 when the history pointers are NULL (the first frame), when
 *      tri < 0, or when step 3 leaves sw = 0.
 *   3. TAPS.  fx = sx - 0.5f, fy = sy - 0.5f.  Unless fx >= -1.f, fx < float(width), fy >= -1.f and fy < float(height) all hold
 *      there is no history (so a NaN gives none).  x0 = floor(fx), ax = fx - x0, likewise y0 and ay.  The four taps are
 *      q = (x0 + i, y0 + j), j outer and i inner, with the weight b = (i ? ax : 1.f - ax) * (j ? ay : 1.f - ay).  A tap is
 *      ACCEPTED when it lies inside the image, len_in[q] >= 1, the previous AOV sums at q have hits > 0, the resolved mean depth
 *      z_q there (sum / float(hits)) has, with dz = z_q - dist, (dz < 0 ? -dz : dz) <= depth_tolerance * dist, and
 *      dot(n_p, n_q) >= normal_cos_min with n_q resolved from the previous AOV sums with prev_aov_samples.  Over the accepted
 *      taps in order, from 0.f: sw = sw + b, and per channel and buffer sh_k = sh_k + b * h, h = float(double(hist_k_in[q]) * 2^-30).
 *      N_prev is the minimum of len_in[q] over the accepted taps (a tap of weight 0 counts).
 *   4. BLEND, when sw > 0: hbar_k = sh_k / sw; N = min(N_prev + 1, max_history); alpha = 1.f / float(N), then
 *      alpha = alpha > alpha_min ? alpha : alpha_min; out_k = (c_k - hbar_k) * alpha + hbar_k; hist_k_out = to_fixed(out_k) and
 *      len_out = N.
 * to_fixed is the kernels' own: magnitudes clamped at 2^31, NaN to 0, x * 2^30 rounded to the nearest integer, ties to even.
 * FINITENESS.  All inputs are finite sums: |c|, |h| <= 2^33.  ax and ay lie in [0, 1] (fx - floor(fx) is exact or rounds to 1),
 * so every b lies in [0, 1]; a motion coordinate is a float, so a b that is not 0 is at least 2^-50 and so is sw, while
 * |sh| <= 4 * 2^33: hbar is a convex mean of the taps' h up to rounding, and the blend of two finite values with alpha in
 * (0, 1] is finite.  A dist that is NaN or infinite fails the depth stop of every tap.  No NaN can arise.
 * Every pixel of every output buffer is written; inputs are only read.  An output buffer that overlaps any input range (or
 * another output) is an argument error.  rt_temporal_params: NULL = the defaults, which rt_temporal_default_params writes (chosen
 * on the CPU against 1024-spp frames: profiles/temporal_quality.json).
 * The contract is the denoisers': device buffers on the current device, ordered on `stream` and synchronous on it at return, the
 * current device left as it was, nothing allocated.  ERRORS return non-zero, begin "rt_temporal_accumulate_fixed: " in
 * rt_last_error() and write nothing: a null d_sum_a, d_aov_fixed, d_motion, d_hist_a_out or d_len_out; width or height < 1 or more
 * than 715827882 pixels; samples_a, aov_samples, samples_b (with d_sum_b) or prev_aov_samples (with history) < 1; d_sum_b and
 * d_hist_b_out not NULL together; d_hist_a_in, d_len_in and d_prev_aov_fixed (and d_hist_b_in with d_sum_b) not all NULL or all
 * set; a d_motion that is not 16-byte aligned; flags != 0; max_history < 1; alpha_min outside (0, 1]; a depth_tolerance that is
 * not finite and positive; normal_cos_min outside [-1, 1]; an overlap; a frame so narrow or so flat that it needs more than
 * 16777215 workgroups of 32 x 8 pixels. */
int rt_render_motion(const rt_scene *scene, const rt_camera *camera, int width, int height, const rt_camera *prev_camera,
                     const float *d_prev_tri_p0p1p2 /* n_tris x 9, caller's order; NULL = vertices did not move */, uint32_t flags,
                     float *d_motion /* width * height x 4 */, void *stream, rt_stats *stats /* may be NULL */);
typedef struct rt_temporal_params {
    int32_t max_history;      /* >= 1: the history length is capped here */
    float   alpha_min;        /* in (0, 1]: floor of the blend factor */
    float   depth_tolerance;  /* > 0, finite: relative */
    float   normal_cos_min;   /* in [-1, 1] */
    uint32_t flags;           /* must be 0 */
} rt_temporal_params;
int rt_temporal_default_params(rt_temporal_params *out);
int rt_temporal_accumulate_fixed(const int64_t *d_sum_a, int samples_a, const int64_t *d_sum_b /* may be NULL */, int samples_b,
                                 const int64_t *d_aov_fixed, int aov_samples, const float *d_motion,
                                 const int64_t *d_hist_a_in, const int64_t *d_hist_b_in, const int32_t *d_len_in /* all NULL = first frame */,
                                 const int64_t *d_prev_aov_fixed, int prev_aov_samples, int width, int height,
                                 const rt_temporal_params *params /* NULL = defaults */, int64_t *d_hist_a_out,
                                 int64_t *d_hist_b_out /* NULL iff d_sum_b is */, int32_t *d_len_out, void *stream);

/* ---- temporal moments and two more stops; the dual filter fed from a variance buffer -----------------------------------------------
 * The single-buffer form of the loop above (SVGF proper: the variance comes from temporally accumulated first and second moments
 * of ONE frame sequence, from a spatial estimate where history is short), and stops that see an edge which depth and normal do
 * not -- an area light in the plane of its ceiling:
 *     rt_render_shard_fixed  (ONE call)
 *       -> rt_render_aov_fixed
 *       -> rt_render_motion
 *       -> rt_temporal_accumulate_moments_fixed
 *       -> rt_denoise_variance_fixed(hist_a_out, 1, variance_out, aov, ...)
 * The caller ping-pongs, next to the sets of rt_temporal_accumulate_fixed, the moments and the MOTION buffer (last frame's motion
 * buffer is "last frame's triangle ids").  Both definitions are ONE STATED SEQUENCE of individually rounded fp32 operations (no
 * FMA), every max or min a comparison and selection, dot as everywhere; the kernels, the CPU twins (hc_temporal_accumulate_moments,
 * hc_denoise_variance: rt_temporal.h and rt_denoise.h are the shared arithmetic) and the numpy restatement of the tests agree in
 * every bit.
 *
 * rt_temporal_accumulate_moments_fixed.  rt_temporal_accumulate_fixed's steps 1 - 4 for the hist and len outputs, with:
 *   EMISSION STOP, part of step 3's acceptance after the normal stop.  e_p[k] = float(double(aov[RT_AOV_EMISSION + k]) * 2^-30) *
 *      (1.f / aov_samples), e_q[k] the same of the previous AOV sums at q with prev_aov_samples; a[k] = |e_p[k] - e_q[k]| (the
 *      difference rounded, then d < 0 ? -d : d); de = a[0], then de = a[k] > de ? a[k] : de for k = 1, 2.  The tap is accepted iff
 *      de <= emission_tolerance.  All sums are finite, so +inf accepts every tap.
 *   TRIANGLE STOP, only with d_prev_motion: the tap is accepted iff the int32 bits of d_prev_motion[4 q + 3] equal this pixel's
 *      tri.  (A tap's id of -1, a miss, never equals: tri >= 0 wherever taps are visited.)
 *   MOMENTS, only with d_moments_out.  S = sum_a, or sum_a + sum_b as rt_denoise_dual_fixed's wrapping add with n = samples_a +
 *      samples_b (n = samples_a with one buffer).  u_p is steps 1 and 2 of rt_denoise_fixed for (S, n) and this frame's AOV sums.
 *      The frame's moments are f = {u.x, u.y, u.z, (u.x * u.x + u.y * u.y) + u.z * u.z}.  With d_moments_in, over the accepted
 *      taps in step 3's order and with its b, from 0.f: sm[j] = sm[j] + b * m_q[j], m_q = d_moments_in[4 q ..].  When sw > 0 and
 *      d_moments_in is given: mbar[j] = sm[j] / sw and m_out[j] = (f[j] - mbar[j]) * alpha + mbar[j] with step 4's alpha.
 *      Otherwise m_out = f.
 *   VARIANCE of the mean of demodulated radiance, summed over the channels (rt_denoise_dual_fixed's step-2 quantity), written
 *      with the moments.  N is the pixel's len_out.
 *      Temporal, when N >= variance_min_history: m1 = m_out[0 .. 2]; t = m_out[3] - dot(m1, m1); v = (t > 0 ? t : 0) / float(N).
 *      Spatial, of this frame, otherwise: visit the 5 x 5 window at stride 1 around p, dy outer and dx inner, both from -2 to 2,
 *      taps outside the image skipped.  The centre counts.  Another tap q counts iff its AOV hits are > 0, with dz = z_q - z_p
 *      (dz < 0 ? -dz : dz) <= depth_tolerance * z_p, and dot(n_p, n_q) >= normal_cos_min (z and n of this frame's AOV sums, as
 *      rt_aov_resolve forms them).  Over the counted taps, from 0.f: cnt = cnt + 1.f, s[j] = s[j] + f_q[j].  M[j] = s[j] / cnt;
 *      t = M[3] - dot(M1, M1); v = (t > 0 ? t : 0) / float(N).
 * FINITENESS.  0 <= u <= 2^43 (rt_denoise_dual_fixed), so every square is at most 2^86 and every dot(u, u) at most 3 * 2^86 <
 * 2^89; b lies in [0, 1] and sw >= 2^-50 where it is not 0, so mbar is a convex mean of previous moments up to rounding and the
 * blend with alpha in (0, 1] stays within the same bounds: moments that are previous outputs of this entry point stay below 2^89,
 * dot(m1, m1) < 2^89, t is finite, and the spatial sums hold at most 25 terms below 2^89.  No NaN and no infinity can arise from
 * finite sums and such moments.  A d_moments_in that is NOT a previous output of this entry point (a NaN, an infinity) may
 * carry a NaN or +inf into d_moments_out and +inf into d_variance_out (a NaN t gives v = 0); rt_denoise_variance_fixed's step 2
 * absorbs either.  The hist and len outputs do not depend on the moments.
 * With emission_tolerance = +inf, d_prev_motion = NULL and d_moments_out = NULL the outputs are rt_temporal_accumulate_fixed's,
 * bit for bit.  rt_temporal_moments_params: NULL = the defaults, which rt_temporal_moments_default_params writes (chosen on the CPU
 * against 1024-spp frames: profiles/temporal_moments_quality.json).
 * The contract is rt_temporal_accumulate_fixed's; every pixel of every supplied output is written.  ERRORS return non-zero, begin
 * "rt_temporal_accumulate_moments_fixed: " in rt_last_error() and write nothing: that entry point's list, and also d_moments_in or
 * d_prev_motion without history; d_moments_out and d_variance_out not NULL together; d_moments_in without d_moments_out; with
 * moments and two buffers, samples_a + samples_b beyond int32; a d_prev_motion, d_moments_in or d_moments_out that is not 16-byte
 * aligned; an emission_tolerance that is negative or NaN; variance_min_history < 1; an overlap of any output (the two new ones
 * included) with any input or another output.
 *
 * rt_denoise_variance_fixed.
 *   1. c, d, e, z, n and u are exactly steps 1 and 2 of rt_denoise_fixed for (d_sum_fixed, num_samples).
 *   2. With x = d_variance[p]: v = x > 0 ? (x < 2^87 ? x : 2^87) : 0.  A NaN or a negative x gives 0; v <= 2^87 is the bound
 *      rt_denoise_dual_fixed's FINITENESS paragraph starts from, so that paragraph holds here unchanged.
 *   3., 4.  rt_denoise_dual_fixed's steps 3 and 4: its text, its kernels, its parameters and defaults, its scratch
 *      (rt_denoise_dual_scratch_bytes).
 * v is the variance of the MEAN of demodulated radiance summed over the three channels, the quantity of rt_denoise_dual_fixed's
 * step 2: with d_variance holding that v, sum = a + b and num_samples = samples_a + samples_b the output is
 * rt_denoise_dual_fixed's, bit for bit.  ERRORS begin "rt_denoise_variance_fixed: ": rt_denoise_dual_fixed's list with d_variance
 * among the pointers that may not be null and num_samples in the place of the two sample counts. */
typedef struct rt_temporal_moments_params {
    int32_t max_history;           /* as rt_temporal_params */
    float   alpha_min;
    float   depth_tolerance;
    float   normal_cos_min;
    float   emission_tolerance;    /* >= 0 or +inf; +inf: the stop passes every tap */
    int32_t variance_min_history;  /* >= 1: below it the variance is the spatial estimate */
    uint32_t flags;                /* must be 0 */
} rt_temporal_moments_params;
int rt_temporal_moments_default_params(rt_temporal_moments_params *out);
int rt_temporal_accumulate_moments_fixed(const int64_t *d_sum_a, int samples_a, const int64_t *d_sum_b /* may be NULL */, int samples_b,
                                         const int64_t *d_aov_fixed, int aov_samples, const float *d_motion,
                                         const int64_t *d_hist_a_in, const int64_t *d_hist_b_in, const int32_t *d_len_in /* all NULL = first frame */,
                                         const int64_t *d_prev_aov_fixed, int prev_aov_samples,
                                         const float *d_prev_motion /* may be NULL: no triangle stop */,
                                         const float *d_moments_in /* width * height x 4; NULL on the first frame or without moments */,
                                         int width, int height, const rt_temporal_moments_params *params /* NULL = defaults */,
                                         int64_t *d_hist_a_out, int64_t *d_hist_b_out /* NULL iff d_sum_b is */, int32_t *d_len_out,
                                         float *d_moments_out /* width * height x 4, may be NULL */,
                                         float *d_variance_out /* width * height; NULL together with d_moments_out */, void *stream);
int rt_denoise_variance_fixed(const int64_t *d_sum_fixed, int num_samples, const float *d_variance /* width * height */,
                              const int64_t *d_aov_fixed, int aov_samples, int width, int height,
                              const rt_denoise_dual_params *params /* NULL = rt_denoise_dual_fixed's defaults */,
                              void *d_scratch /* rt_denoise_dual_scratch_bytes */, float *d_rgb_out /* width * height * 3 */, void *stream);

/* ---- AOV-guided upsampling: a low-resolution frame and full-resolution features become a full-resolution frame -----------------
 * The beauty frame is where the time goes and its feature buffers are noise-free at any sample count, so a path-tracing budget
 * is spent best on radiance at half or quarter resolution and on features at full resolution (no reference counterpart).  This is
 * the call that joins the two: joint bilateral upsampling (Kopf et al. 2007) on albedo-demodulated radiance, as SVGF-style
 * pipelines do it.  The loop is
 *   rt_render_shard_fixed (low size)  +  rt_render_aov_fixed (low size)  +  rt_render_aov_fixed (full size), one rt_camera
 *       -> rt_upsample_fixed(sum_lo, spp, aov_lo, ..., aov_hi, ..., d_rgb_out, d_out_fixed)
 *       -> rt_denoise_fixed(d_out_fixed, 1, aov_hi, ...) | rt_denoise_variance_fixed | a temporal accumulator
 * and rt_upsample_rgb takes a float frame in the place of the sums, for example a denoiser's output at the low size.  The full
 * frame is width = factor * low_width by height = factor * low_height -- exactly the case in which a pinhole frame of the same
 * rt_camera covers the same frustum at both sizes.  factor is 2, 3 or 4.
 * Like rt_denoise_fixed the whole filter is ONE STATED SEQUENCE of individually rounded fp32 operations (no FMA, sums start at
 * 0.f, "x > t ? x : t" is that selection): the kernel, the CPU twin (hc_upsample of librt_hostcheck.so) and the numpy restatement
 * of the tests agree in every bit of every pixel.
 *   1. LOW PIXEL q.  Steps 1 and 2 of rt_denoise_fixed for (d_sum_lo[q], num_samples) and (d_aov_lo[q], aov_samples_lo) give
 *      u_q, z_q, n_q.  In rt_upsample_rgb c is the given float, and a c that is NaN or infinite is taken as 0.f (so that no
 *      0 * inf can arise); everything after c is the same text.  (A finite c of 2^118 or more can still overflow u over the
 *      albedo floor 2^-10; the output of such a frame is undefined.  Radiance this renderer forms stays below 2^31.)
 *   2. FULL PIXEL p = (x, y).  z_p, n_p, d_p, e_p are exactly those steps' for d_aov_hi[p] and aov_samples_hi.  If the hits
 *      channel of d_aov_hi[p] is <= 0, u_p = 0 on every channel and no tap is visited: a pixel no sample hit has no radiance in
 *      this renderer.
 *   3. POSITION, per axis, in integers: a = 2 * x + 1 - factor; X0 = floor(a / (2 * factor)), rounding toward minus infinity;
 *      r = a - 2 * factor * X0; fx = float(r) / float(2 * factor), a true division.  The same in y (Y0, fy).
 *   4. TAPS.  jy outer and jx inner, both from -1 to 2; the low pixel is (X0 + jx, Y0 + jy); a tap outside the low image is
 *      skipped.  t = float(j) - f; k = 1.f - 0.5f * (t < 0 ? -t : t); h = ky * kx: a tent of radius 2.  At least one tap with
 *      k >= 0.5 lies inside the image on each axis, so the sum of h is positive.
 *      w = (h * rt_expnegf(-x_z)) * w_n, rt_denoise_fixed's tap weight with both colour arguments equal and kc = 0 (its colour
 *      term is exactly +0): x_z = (dz * dz) * kz, dz = z_q - z_p, kz = 1.f / (sigma_depth * sigma_depth) made on the host, w_n
 *      from n_p . n_q clamped to 0 .. 1 and squared normal_power_log2 times.
 *      Four running sums in tap order: sw = sw + w, su = su + w * u_q, sh = sh + h, sb = sb + h * u_q.
 *   5. RESULT.  u_p = sw > 0.f ? su / sw : sb / sh per channel.  The second form is the plain tent filter: it serves a pixel
 *      whose features no low tap shares, a thin edge for example.
 *   6. REMODULATE with the full-resolution features: out = u_p * d_p + e_p per channel, LINEAR MEAN RADIANCE, what the
 *      denoisers write.  d_out_fixed is the accumulators' to_fixed of it (magnitudes clamped to 2^31, NaN to 0, units of 2^-30,
 *      round to nearest even): int64 sums of ONE sample of the mean, the format the accumulators emit, so rt_denoise_fixed(out, 1,
 *      aov_hi, ...), rt_denoise_variance_fixed and both accumulators take an upsampled frame unchanged.
 * rt_upsample_params: NULL = the defaults, which rt_upsample_default_params writes (profiles/upsample_quality.json).
 * No scratch is needed.  rt_render_aov_follow_fixed's buffers have the same layout and may be passed as either feature buffer.
 * The contract is the denoisers': device buffers on the current device, ordered on `stream` and synchronous on it at return, the
 * current device left as it was, nothing allocated, inputs only read, every pixel of each non-null output written; outputs
 * that overlap inputs are undefined.  ERRORS return non-zero, begin "rt_upsample_fixed: " / "rt_upsample_rgb: " in
 * rt_last_error() and write nothing: a null pointer other than params and ONE of the two outputs (both null is an error);
 * factor outside 2 .. 4; a low size below 1, or a full frame of more than 715827882 pixels; a sample count below 1;
 * normal_power_log2 outside 0 .. 8; a sigma_depth that is not finite and positive, or whose kz is not; flags != 0; a full frame
 * that would need more than 16777215 workgroups of 32 x 8 pixels. */
typedef struct rt_upsample_params {
    float   sigma_depth;        /* > 0; scene units */
    int32_t normal_power_log2;  /* 0 .. 8: w_n = min(max(0, n_p . n_q), 1) squared this many times */
    uint32_t flags;             /* must be 0 */
} rt_upsample_params;
int rt_upsample_default_params(rt_upsample_params *out);
int rt_upsample_fixed(const int64_t *d_sum_lo /* low_width * low_height * 3 */, int num_samples,
                      const int64_t *d_aov_lo /* low_width * low_height * 11 */, int aov_samples_lo, int low_width, int low_height,
                      int factor, const int64_t *d_aov_hi /* factor^2 * low_width * low_height * 11 */, int aov_samples_hi,
                      const rt_upsample_params *params /* NULL = defaults */, float *d_rgb_out /* full size * 3, may be NULL */,
                      int64_t *d_out_fixed /* full size * 3, may be NULL */, void *stream);
int rt_upsample_rgb(const float *d_rgb_lo /* low_width * low_height * 3, linear mean radiance, e.g. a denoiser's output */,
                    const int64_t *d_aov_lo, int aov_samples_lo, int low_width, int low_height, int factor,
                    const int64_t *d_aov_hi, int aov_samples_hi, const rt_upsample_params *params /* NULL = defaults */,
                    float *d_rgb_out /* may be NULL */, int64_t *d_out_fixed /* may be NULL */, void *stream);

/* ---- ray queries (no reference counterpart: its Bvh::traverse is reachable only from render()) ----------------------------
 * "Trace my rays, from my buffers, on my stream."  All pointers are DEVICE buffers on the scene's device (a buffer on another
 * device or on the host cannot be told apart from a good one: the call faults instead of failing); origins and directions are
 * n AoS xyz triples.  d_tmax NULL = FLT_MAX for every ray.  flags: 0, RT_FLAG_REFERENCE_WALK or RT_FLAG_WATERTIGHT (see the
 * flags; both together, or any other flag, is an error).  rt_trace_closest_flags / rt_trace_any_flags below are the host-pointer
 * form of these two calls -- one implementation, so their answers are these, bit for bit:
 *   closest: d_hit_tri[i] = the hit triangle in the caller's ORIGINAL order or -1; t, u, v as Intersection
 *       (intersection.hpp:4-6), and t = u = v = 0 on a miss, so every output buffer is fully defined after the call.  Any
 *       of d_t, d_u, d_v may be NULL (not written).
 *   any: d_occluded[i] in {0, 1}; d_excluded_tri[i] (caller's order) is the one triangle ray i may pass through -- an index
 *       < 0 or >= n_tris excludes nothing, and so does d_excluded_tri = NULL.
 * Directions are unit vectors; what is CHECKED, on the device before anything is written, is that every component is finite
 * and below 2^126 in magnitude (beyond that the reference's slab arithmetic overflows and a visibility decision would not be
 * the reference's): otherwise the call fails and names the number of offending rays.  Directions need not have unit length: a
 * direction scaled by s gives the same hits at t / s.  One whose largest component is below 2^-60 in magnitude and that is not
 * zero is refused in the same way, with the number of such rays (the traversal keeps 1 / d finite by a floor of 2^-90 under
 * each component, which such a ray would feel; a zero direction hits nothing).  A non-finite ORIGIN is legal: the ray
 * misses.  0 <= n <= 2^30; n = 0 succeeds and touches nothing.
 * The work is ordered on `stream` (NULL = default stream) and the call is synchronous on that stream when it returns, as
 * rt_scene_update_device and rt_render_shard are.  The calling thread's current device is left as it was.  The steady path
 * allocates nothing: the few words of scratch and the overflow stacks belong to the scene and are made by its first query
 * (queries of ONE scene therefore take turns).  Origins outside the radius the scene's records are padded for widen the
 * padding once, as a render from outside the bounds does.  Queries only read the scene: queries and renders of one scene may
 * overlap; rt_scene_update* / rt_scene_rebuild* may not overlap a query, as for renders.
 * Errors (null scene, a null pointer that may not be null, n out of range, bad flags, bad directions) return non-zero, set
 * rt_last_error() and write nothing. */
int rt_query_closest_device(const rt_scene *scene, uint32_t flags, int n, const float *d_origin_xyz, const float *d_dir_xyz,
                            const float *d_tmax, int32_t *d_hit_tri, float *d_t, float *d_u, float *d_v, void *stream);
int rt_query_any_device(const rt_scene *scene, uint32_t flags, int n, const float *d_origin_xyz, const float *d_dir_xyz,
                        const float *d_tmax, const int32_t *d_excluded_tri, int32_t *d_occluded, void *stream);
/* The rare path of the LAST query on this scene (flags = 0 only; zero otherwise): out[0] = closest hits re-traced through the
 * reference's own tree, out[1] = accepted hits the reference's box test loses, out[2] = exact ties at the final distance --
 * per call what rt_stats.reserved[4..6] are per render. */
int rt_query_last_counters(const rt_scene *scene, int64_t out[3]);

/* ---- stage-level entry points (parity tests call these; HOST pointers, AoS xyz triples) -----
 * The host-pointer form of the queries above, kept for the parity tests; applications use rt_query_*_device.  A call uploads
 * the caller's arrays, runs the query's walk on the default stream and copies the answers back; calls on ONE scene take turns
 * with its queries.  Unlike the queries they check no direction (the precondition below is the caller's to keep) and leave
 * rt_query_last_counters alone.
 * Closest hit (Bvh::traverse, bvh.cuh:251-303; ch(), render.cuh:297-328): hit_tri = index of
 * the hit triangle in the caller's ORIGINAL order or -1; t,u,v as Intersection
 * (intersection.hpp:4-6), t = u = v = 0 on a miss. */
int rt_trace_closest(const rt_scene *scene, int n, const float *origin_xyz, const float *dir_xyz,
                     const float *tmax, int32_t *hit_tri, float *t, float *u, float *v);
/* Any hit excluding one triangle (bvh.cuh:306-357; ah(), render.cuh:278-294): occluded[i] in {0,1}; excluded_tri[i] in the
 * caller's order, an index < 0 or >= n_tris excludes nothing. */
int rt_trace_any(const rt_scene *scene, int n, const float *origin_xyz, const float *dir_xyz,
                 const float *tmax, const int32_t *excluded_tri, int32_t *occluded);
/* The same two entry points with a flags word (RT_FLAG_REFERENCE_WALK / RT_FLAG_WATERTIGHT: see the flags).  flags = 0 is
 * rt_trace_closest / rt_trace_any: hit_tri, t, u, v and occluded are the reference's answers, ties and lost hits included.
 * Directions are unit vectors.  PRECONDITION, not checked here: every component finite and below 2^126 in magnitude, and the
 * largest component at least 2^-60 (or the direction zero) -- what rt_query_*_device refuse. */
int rt_trace_closest_flags(const rt_scene *scene, uint32_t flags, int n, const float *origin_xyz, const float *dir_xyz,
                           const float *tmax, int32_t *hit_tri, float *t, float *u, float *v);
int rt_trace_any_flags(const rt_scene *scene, uint32_t flags, int n, const float *origin_xyz, const float *dir_xyz,
                       const float *tmax, const int32_t *excluded_tri, int32_t *occluded);
/* curand_init(seed, subsequence, 0) for subsequences [first, first+count) (render.cuh:68-73):
 * state6 receives count x {d, v0..v4}.  Then `draws` uniforms per state into uniforms
 * (count x draws, may be 0 / NULL), advancing the returned states. */
int rt_xorwow_states(uint64_t seed, uint32_t first, uint32_t count, int draws, uint32_t *state6,
                     float *uniforms);

/* Releases every device allocation the library holds behind the scenes: the per-device render contexts (path pools, RNG
 * states, counters, overflow stacks, events) and the cached output buffers of rt_render / rt_render_multi.  Scenes are the
 * caller's (rt_scene_destroy).  No render may be in flight; the library keeps working afterwards (everything is re-created on
 * demand).  The reference frees nothing at all (render.cuh:374-391, bvh.cuh:211-217). */
void rt_shutdown(void);

/* rt_render_multi: what became of peer access between devices[0] and every other listed device, pair by pair, since the process
 * started ("devices 0 <-> 1: peer access enabled; ..." or the reason it is not and that copies go through host memory).  Empty
 * until a call has listed two different devices.  NOTE: that path has not run on two PHYSICAL GPUs yet (one-GPU boxes list a
 * device twice); bench.py's multi-GPU probe records this string so that a first real run can be diagnosed from its output. */
const char *rt_peer_access_log(void);

const char *rt_last_error(void);
const char *rt_version(void);
/* Hash of the sources, compiler flags and experiment defines this library's device code was built from (csrc/Makefile).
 * Measurement artefacts (profiles/pmc_k_paths.json) carry it, so counters are never priced against another build. */
const char *rt_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* RTCUDA_AMD_H */
