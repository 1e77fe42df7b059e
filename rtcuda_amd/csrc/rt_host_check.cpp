// rt_host_check.cpp -- host-only checks of the BVH builder (rt_bvh.h) and a CPU walk of the product's tree, g++.
//
// Runs without a GPU:
//   * rt_bvh_selfcheck  validates both record formats the kernels can be given -- `quads` (4-wide, the default: two
//     pair-style records per node) and `pairs` (2-wide) -- structurally (every triangle in exactly one leaf, every node
//     reachable exactly once, every record box contains what lies beneath it, stack bound) and walks both on the CPU
//     with the control flow and the fp32 expressions of inner_step (rt_walk.inc) / the triangle blocks of the kernels, comparing
//     with an exhaustive search.  A malformed tree would hang or fault the GPU; this is where it is caught first.
//   * rt_bvh_refit_check  the host twin of the device refit (rt_scene_update): the builder's records with new vertices,
//     checked as above (bit-equal to the builder's with the creation vertices; structure and walk with moved ones).
//   * rt_ploc_build / rt_ploc_check  the host twin of the device PLOC builder (rt_scene_rebuild, RT_SCENE_DEVICE_BVH):
//     its records and leaf order (bit-equal to the device's), checked as above, with its surface-area cost next to rtbvh::build's.
//   * rt_hostwalk_*     the same walk for arbitrary rays (closest hit / any hit), with work counters: the traversal
//     audit (tests/test_traversal_audit.py) replays the rays of an oracle render through it.
//   * rt_plan_paths_launch  the launch geometry of the persistent frame kernels (rt_launch_plan.h), as the library computes it.
//   * rt_slot_chunk_*   the chunked deal of k_paths (rt_slot_chunks.h): task -> slot, the static deal's slots, the counts and
//     the decisions, as the kernel makes them.
//   * rt_background_rect  the pixel rectangle outside which k_paths makes no camera ray (rt_background.h), as the library computes it.
//   * hc_denoise / hc_expnegf  the CPU twin of rt_denoise_fixed: a serial loop over rt_denoise.h, the arithmetic of the kernels.
//   * hc_denoise_dual   the CPU twin of rt_denoise_dual_fixed, likewise; both walk the pixels with dn_walk, the twins' own loop.
//   * hc_upsample       the CPU twin of rt_upsample_fixed and rt_upsample_rgb: a serial loop over rt_upsample.h.
//   * hc_merge_shard_stats  the merge of the shards' rt_stats (rt_stats_merge.h), the library's own function.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>

#include "rt_background.h"
#include "rt_bvh.h"
#include "rt_denoise.h"
#include "rt_launch_plan.h"
#include "rt_ploc.h"
#include "rt_ref_tree.h"
#include "rt_slot_chunks.h"
#include "rt_stats_merge.h"
#include "rt_temporal.h"
#include "rt_upsample.h"

namespace {
struct V3 { float x, y, z; };
inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
struct Tri { V3 p0, e1, e2, n; };
inline bool tri_hit(const Tri &tr, V3 o, V3 d, float tmax, float &t) {
    V3 c = sub(tr.p0, o);
    V3 r = cross(d, c);
    float inv_det = 1.f / dot(d, tr.n);
    float u = inv_det * dot(tr.e2, r);
    float v = inv_det * dot(tr.e1, r);
    if (u >= 0.0f && v >= 0.0f && (u + v) <= 1.0f) {
        float tt = inv_det * dot(c, tr.n);
        if (0 < tt && tt <= tmax) { t = tt; return true; }
    }
    return false;
}
// (as box_hit / inner_step in rt_walk.inc; the kernels' 1 / d is v_rcp_f32, 1 ulp, here an exact division)
inline bool box_hit(V3 o, V3 inv, const float *lo, const float *hi, float tmax, float &entry) {
    float ax = (lo[0] - o.x) * inv.x, bx = (hi[0] - o.x) * inv.x;
    float ay = (lo[1] - o.y) * inv.y, by = (hi[1] - o.y) * inv.y;
    float az = (lo[2] - o.z) * inv.z, bz = (hi[2] - o.z) * inv.z;
    float t_in = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
    float t_out = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
    entry = t_in;
    t_out = t_out * 1.000001f;
    return t_in <= t_out && t_out >= 0.f && t_in <= tmax * rtbvh::kCullTmaxWiden;
}
// The 4-wide node step of the kernels: plane distance as ONE fma, b * (1 / d) + s with s = -o * (1 / d) rounded on its own
// (inner_step<true> in rt_walk.inc); the records it is given are padded for that (rt_bvh.h, pad_quads_for_origins)
inline bool box_hit_fma(V3 o, V3 inv, const float *lo, const float *hi, float tmax, float &entry) {
    const float sx = -o.x * inv.x, sy = -o.y * inv.y, sz = -o.z * inv.z;
    float ax = fmaf(lo[0], inv.x, sx), bx = fmaf(hi[0], inv.x, sx);
    float ay = fmaf(lo[1], inv.y, sy), by = fmaf(hi[1], inv.y, sy);
    float az = fmaf(lo[2], inv.z, sz), bz = fmaf(hi[2], inv.z, sz);
    float t_in = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
    float t_out = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
    entry = t_in;
    t_out = t_out * 1.000001f;
    return fmaxf(t_in, 0.f) <= fminf(t_out, fminf(tmax * rtbvh::kCullTmaxWiden, FLT_MAX));
}
inline V3 inv_dir(V3 d) {  // the cull's 1 / d: the true direction's, kept finite (rt_bvh.h, kCullDirFloor)
    auto clampinv = [](float x) { return 1.f / ((fabsf(x) < rtbvh::kCullDirFloor) ? copysignf(rtbvh::kCullDirFloor, x) : x); };
    return V3{clampinv(d.x), clampinv(d.y), clampinv(d.z)};
}
std::vector<Tri> leaf_order_triangles(const float *verts, const rtbvh::Result &r, int n) {
    std::vector<Tri> tris(n);
    for (int k = 0; k < n; k++) {
        const float *q = verts + 9 * (size_t)r.order[k];
        V3 p0{q[0], q[1], q[2]}, p1{q[3], q[4], q[5]}, p2{q[6], q[7], q[8]};
        tris[k].p0 = p0; tris[k].e1 = sub(p0, p1); tris[k].e2 = sub(p2, p0); tris[k].n = cross(tris[k].e1, tris[k].e2);
    }
    return tris;
}

struct WalkResult {
    int best = -1;          // closest: leaf-order triangle index or -1
    float t = 0.f;
    bool occluded = false;  // any hit
    long long nodes = 0, tris = 0, leaves = 0;
    int max_sp = 0;
    long long sp_hist[32] = {0};  // node steps by the stack size the lane has when it makes them (>= 31 in the last bin)
    bool failed = false;
    bool unseen_occluder = false;  // verified any-hit walks: the occluder found is invisible to the reference's walk
    float tie_t = -1.f;     // closest: the distance of the last EXACT tie between two accepted hits (a tie at the final t
                            // is what the reference's tree order decides: triangle.cuh:49)
    long long own_fail = 0, leaf_fail = 0;  // verified walks: hits whose own box / whose reference leaf box fails the reference's slab test
};

// ---- the reference's slab test (aabb_intersector.cuh:14-36), as reference_walk / ref_visible in rt_walk.inc
struct RefSlab {
    bool nx, ny, nz;
    V3 inv, so;
    bool neg_zero;  // a direction component is -0.0: the octant (d < 0: false) and the sign of 1 / d disagree
};
inline bool is_neg_zero(float x) { uint32_t b; memcpy(&b, &x, 4); return b == 0x80000000u; }
inline RefSlab ref_slab(V3 o, V3 d) {
    RefSlab s;
    s.nx = d.x < 0; s.ny = d.y < 0; s.nz = d.z < 0;
    auto refinv = [](float x) { return 1.f / ((fabsf(x) < FLT_EPSILON) ? copysignf(FLT_EPSILON, x) : x); };  // aabb_intersector.cuh:17-19
    s.inv = V3{refinv(d.x), refinv(d.y), refinv(d.z)};
    s.so = V3{(-o.x) * s.inv.x, (-o.y) * s.inv.y, (-o.z) * s.inv.z};
    s.neg_zero = is_neg_zero(d.x) || is_neg_zero(d.y) || is_neg_zero(d.z);
    return s;
}
// b = [xmin, xmax, ymin, ymax, zmin, zmax] (bounding_box.cuh:15)
inline bool ref_box(const RefSlab &s, const float *b, float &entry) {
    const float ex = s.inv.x * b[s.nx ? 1 : 0] + s.so.x;
    const float ey = s.inv.y * b[s.ny ? 3 : 2] + s.so.y;
    const float ez = s.inv.z * b[s.nz ? 5 : 4] + s.so.z;
    entry = fmaxf(ex, fmaxf(ey, ez));
    const float xx = s.inv.x * b[s.nx ? 0 : 1] + s.so.x;
    const float xy = s.inv.y * b[s.ny ? 2 : 3] + s.so.y;
    const float xz = s.inv.z * b[s.nz ? 4 : 5] + s.so.z;
    return entry <= fminf(xx, fminf(xy, xz));
}
// What the reference's walk can SEE.  Its box test does not look at tmax (aabb_intersector.cuh:35), so whether it ever
// reaches a triangle depends on the ray alone: every box on the way down to the triangle's leaf must pass.  Those
// boxes are nested exactly (a node's box is the min / max of its triangles' boxes, bvh.cuh:57-61,150-160), rounding is
// monotone, and a slab term inv * bound + so is a monotone function of the bound -- so (octants consistent with the
// signs of 1 / d, i.e. no -0.0 component) a parent's entry distance is <= its child's and its exit distance >= its
// child's: IF THE LEAF'S BOX PASSES, EVERY ANCESTOR'S PASSES.  The triangle's own box (triangle.cuh:22-37) lies inside
// the leaf's, so a pass on it is a pass on the leaf: the common case needs no memory access at all.
// The one case in which octant and sign of 1 / d disagree is a direction component of exactly -0.0: the nesting argument
// does not hold then, and the ancestors are tested one by one through the parent links.
struct RefView {
    rtref::Tree tree;
    std::vector<int> leaf_of;  // caller's triangle index -> node index of its leaf in the reference's tree
    std::vector<int> parent;   // node -> parent node (root: -1)
    bool root_leaf = true;
};
inline void own_box(const Tri &tr, float *b) {  // triangle.cuh:9-10,22-37 on the stored record
    const V3 p1 = sub(tr.p0, tr.e1), p2{tr.p0.x + tr.e2.x, tr.p0.y + tr.e2.y, tr.p0.z + tr.e2.z};
    b[0] = fminf(tr.p0.x, fminf(p1.x, p2.x)); b[1] = fmaxf(tr.p0.x, fmaxf(p1.x, p2.x));
    b[2] = fminf(tr.p0.y, fminf(p1.y, p2.y)); b[3] = fmaxf(tr.p0.y, fmaxf(p1.y, p2.y));
    b[4] = fminf(tr.p0.z, fminf(p1.z, p2.z)); b[5] = fmaxf(tr.p0.z, fmaxf(p1.z, p2.z));
}
inline bool ref_visible(const RefView &rv, const RefSlab &s, const Tri &tr, int caller_index, WalkResult &w) {
    float b[6], e;
    own_box(tr, b);
    if (ref_box(s, b, e) && !s.neg_zero) return true;
    w.own_fail++;
    if (rv.root_leaf) return true;  // bvh.cuh:252 / :307: a root that is a leaf is intersected without a box test
    int node = rv.leaf_of[(size_t)caller_index];
    bool vis = ref_box(s, rv.tree.nodes[(size_t)node].box.b, e);
    if (vis && s.neg_zero)
        for (node = rv.parent[(size_t)node]; vis && node > 0; node = rv.parent[(size_t)node])  // (the root's own box is never tested)
            vis = ref_box(s, rv.tree.nodes[(size_t)node].box.b, e);
    if (!vis) w.leaf_fail++;
    return vis;
}
// One ray through one of the two record formats.  wide: node = records cur, cur + 1 (children 0, 1 | 2, 3): the nearest
// child the ray may enter becomes the cursor, the others are pushed in record order; 2-wide: near child, far child
// pushed.  mode 0: closest hit (ties: the larger caller index, closest_hit_wins); mode 1: any hit but `excl`.
// `rv` (verified walks, mode 1): the first accepted hit ends the walk, as always; if the reference's walk cannot see its
// triangle, the result is flagged (`unseen_occluder`) and the caller asks the literal walk.
WalkResult walk_ray(const std::vector<rtbvh::Pair> &rec, bool wide, const std::vector<Tri> &tris, const std::vector<int32_t> &order,
                    int stack_entries, int mode, V3 o, V3 d, float tmax, int excl, const RefView *rv = nullptr) {
    WalkResult w;
    RefSlab slab{};
    if (rv) slab = ref_slab(o, d);
    std::vector<int> stack(stack_entries + 8);
    const V3 inv = inv_dir(d);
    int sp = 0, cur = tris.empty() ? rtbvh::kNoChild : 0;
    long long steps = 0;
    float t;
    while (cur != rtbvh::kNoChild && !w.occluded) {
        if (++steps > 1000000) { w.failed = true; break; }
        if (cur >= 0) {
            w.nodes++;
            w.sp_hist[sp < 31 ? sp : 31]++;
            const float *boxes[4];
            int links[4];
            int nk = 0;
            for (int half = 0; half < (wide ? 2 : 1); half++) {
                const rtbvh::Pair &p = rec[cur + half];
                boxes[nk] = p.lbox; links[nk++] = p.llink;
                boxes[nk] = p.rbox; links[nk++] = p.rlink;
            }
            float e[4];
            bool h[4];
            for (int k = 0; k < nk; k++)
                h[k] = (wide ? box_hit_fma(o, inv, boxes[k], boxes[k] + 3, tmax, e[k]) : box_hit(o, inv, boxes[k], boxes[k] + 3, tmax, e[k])) &&
                       links[k] != rtbvh::kNoChild;
            int near_k = -1;
            for (int k = 0; k < nk; k++)  // nearest entered child; ties: the lower index (as the kernels' !(a > b) selects)
                if (h[k] && (near_k < 0 || e[k] < e[near_k])) near_k = k;
            if (near_k < 0) {
                cur = sp > 0 ? stack[--sp] : rtbvh::kNoChild;
            } else {
                for (int k = 0; k < nk; k++)
                    if (h[k] && k != near_k) {
                        if (sp >= (int)stack.size()) { w.failed = true; break; }
                        stack[sp++] = links[k];
                    }
                if (w.failed) break;
                cur = links[near_k];
                if (sp > w.max_sp) w.max_sp = sp;
            }
        } else {
            int ref = ~cur, first = ref >> 3, count = ref & 7;
            w.leaves++;
            for (int k = first; k < first + count; k++) {
                w.tris++;
                if (tri_hit(tris[k], o, d, tmax, t)) {
                    if (mode == 1) {
                        if (k != excl) {
                            w.occluded = true;
                            w.unseen_occluder = rv && !ref_visible(*rv, slab, tris[k], order[k], w);
                            break;
                        }
                    } else {
                        if (t == tmax && w.best >= 0) w.tie_t = t;
                        if (!(t == tmax && w.best >= 0) || order[k] > order[w.best]) {  // closest_hit_wins()
                            tmax = t;
                            w.best = k;
                        }
                    }
                }
            }
            cur = sp > 0 ? stack[--sp] : rtbvh::kNoChild;
        }
    }
    w.t = w.best >= 0 ? tmax : 0.f;
    return w;
}

// The 4-wide records as the kernels are given them: padded for the origins of the rays at hand (the scene's own bounds, and
// whatever lies farther out in this batch -- ensure_origin_radius in rtcuda_amd.hip does the same per render / per call)
std::vector<rtbvh::Pair> padded_quads(const rtbvh::Result &r, int n_rays, const float *o3) {
    float radius[3];
    rtbvh::quads_abs_bounds(r.quads, radius);
    for (int i = 0; i < n_rays; i++)
        for (int a = 0; a < 3; a++) {
            const float v = o3[3 * (size_t)i + a];
            if (std::isfinite(v) && std::fabs(v) * 1.001f > radius[a]) radius[a] = 2.f * std::fabs(v) * 1.001f;
        }
    if (rtbvh::knob("RT_NO_ORIGIN_PAD")) radius[0] = radius[1] = radius[2] = 0.f;  // (tests: shows what the padding is for)
    std::vector<rtbvh::Pair> out;
    rtbvh::pad_quads_for_origins(r.quads, radius, out);
    return out;
}
// structural validation of one record format: returns the number of errors
int64_t validate(const rtbvh::Result &r, const std::vector<rtbvh::Pair> &rec, bool wide, const float *verts, int n, int &max_leaf) {
    const int per_node = wide ? 2 : 1;
    const int n_nodes = (int)rec.size() / per_node;
    int64_t errors = (int)rec.size() % per_node ? 1 : 0;
    std::vector<int> seen_tri(n, 0), seen_node(n_nodes, 0);
    if (n_nodes > 0) seen_node[0] = 1;
    for (int ni = 0; ni < n_nodes; ni++)
        for (int k = 0; k < 2 * per_node; k++) {
            const rtbvh::Pair &p = rec[per_node * ni + (k >> 1)];
            const int link = (k & 1) ? p.rlink : p.llink;
            const float *box = (k & 1) ? p.rbox : p.lbox;
            if (link == rtbvh::kNoChild) continue;
            if (link < 0) {
                int ref = ~link, first = ref >> 3, count = ref & 7;
                if (count <= 0 || first < 0 || first + count > n) { errors++; continue; }
                max_leaf = std::max(max_leaf, count);
                for (int q = first; q < first + count; q++) {
                    int ti = r.order[q];
                    if (ti < 0 || ti >= n) { errors++; continue; }
                    seen_tri[ti]++;
                    const float *v = verts + 9 * (size_t)ti;
                    for (int c = 0; c < 3; c++)
                        for (int a = 0; a < 3; a++)
                            if (!(v[3 * c + a] >= box[a]) || !(v[3 * c + a] <= box[3 + a])) errors++;
                }
            } else {
                if (link % per_node != 0 || link / per_node >= n_nodes || link / per_node <= ni) { errors++; continue; }  // children come later
                seen_node[link / per_node]++;
                for (int g = 0; g < 2 * per_node; g++) {  // every grandchild box lies inside this child box
                    const rtbvh::Pair &cp = rec[link + (g >> 1)];
                    if (((g & 1) ? cp.rlink : cp.llink) == rtbvh::kNoChild) continue;
                    const float *gb = (g & 1) ? cp.rbox : cp.lbox;
                    for (int a = 0; a < 3; a++)
                        if (gb[a] < box[a] - 1e-6f || gb[3 + a] > box[3 + a] + 1e-6f) errors++;  // (both padded by 2 ulps)
                }
            }
        }
    for (int i = 0; i < n; i++) if (seen_tri[i] != 1) errors++;
    for (int i = 0; i < n_nodes; i++) if (seen_node[i] != 1) errors++;
    return errors;
}
// ---- host twin of the device refit (k_refit_level in rt_build_kernels.inc): the builder's 4-wide records with new vertices.
// A node's child boxes are exact -- a leaf child's from the triangles' vertices p0, p1, p2, an inner child's the union of
// its own children's exact boxes -- and padded by 2 ulps only when written, as rtbvh::build writes them.  Children come
// after their parent in record order, so one backward sweep is bottom-up.
std::vector<rtbvh::Pair> refit_quads(const std::vector<rtbvh::Pair> &quads, const std::vector<int32_t> &order, const float *verts) {
    std::vector<rtbvh::Pair> out = quads;
    const size_t n_nodes = quads.size() / 2;
    std::vector<rtbvh::Box> exact(n_nodes);
    for (size_t j = n_nodes; j-- > 0;) {
        exact[j].reset();
        for (int k = 0; k < 4; k++) {
            rtbvh::Pair &rec = out[2 * j + (k >> 1)];
            const int32_t link = (k & 1) ? rec.rlink : rec.llink;
            if (link == rtbvh::kNoChild) continue;
            rtbvh::Box b;
            b.reset();
            if (link < 0) {
                const int ref = ~link, first = ref >> 3, count = ref & 7;
                for (int t = first; t < first + count; t++) {
                    const float *v = verts + 9 * (size_t)order[(size_t)t];
                    for (int a = 0; a < 3; a++) {
                        b.lo[a] = std::min(b.lo[a], std::min(v[a], std::min(v[3 + a], v[6 + a])));
                        b.hi[a] = std::max(b.hi[a], std::max(v[a], std::max(v[3 + a], v[6 + a])));
                    }
                }
            } else {
                b = exact[(size_t)link / 2];
            }
            float *dst = (k & 1) ? rec.rbox : rec.lbox;
            for (int a = 0; a < 3; a++) {
                dst[a] = rtbvh::pad_down(b.lo[a], 2);
                dst[3 + a] = rtbvh::pad_up(b.hi[a], 2);
            }
            exact[j].extend(b);
        }
    }
    return out;
}

// Surface-area cost of a 4-wide tree, relative to the area of the root's bounds: quads_sah in rtcuda_amd.hip (double sums
// over the records' padded boxes, a leaf child weighted by its triangles, an inner child by one node step)
double quads_sah_host(const std::vector<rtbvh::Pair> &quads) {
    auto half_area = [](const float *b) {
        const double e0 = (double)b[3] - b[0], e1 = (double)b[4] - b[1], e2 = (double)b[5] - b[2];
        return (e0 + e1) * e2 + e0 * e1;
    };
    double cost = 0.0, root[6] = {DBL_MAX, DBL_MAX, DBL_MAX, -DBL_MAX, -DBL_MAX, -DBL_MAX};
    for (size_t k = 0; k < quads.size(); k++)
        for (int side = 0; side < 2; side++) {
            const int32_t l = side ? quads[k].rlink : quads[k].llink;
            if (l == rtbvh::kNoChild) continue;
            const float *b = side ? quads[k].rbox : quads[k].lbox;
            cost += half_area(b) * (l < 0 ? (double)((~l) & 7) : 1.0);
            if (k < 2)
                for (int a = 0; a < 3; a++) {
                    root[a] = std::min(root[a], (double)b[a]);
                    root[3 + a] = std::max(root[3 + a], (double)b[3 + a]);
                }
        }
    const double e0 = root[3] - root[0], e1 = root[4] - root[1], e2 = root[5] - root[2];
    return quads.size() < 2 || !(e0 >= 0.0) ? 0.0 : cost / std::max((e0 + e1) * e2 + e0 * e1, 1e-30);
}

// ---- host twin of the device PLOC builder (k_ploc_* in rt_build_kernels.inc): the same keys, nearest neighbours, merges, leaves
// and 4-wide collapse, one after the other, with rt_ploc.h's expressions -- the device's records and leaf order, bit for bit.
struct PlocHostNodes {
    int n = 0;
    std::vector<float> boxes;       // 6 per node, exact
    std::vector<int> lft, rgt, cnt;  // triangle nodes: lft = -1, rgt = original index
    std::vector<float> cost;
    std::vector<char> leaf;
    bool is_leaf(int i) const { return leaf[(size_t)i] != 0; }
    bool is_tri(int i) const { return i < n; }
    int tri(int i) const { return rgt[(size_t)i]; }
    int left(int i) const { return lft[(size_t)i]; }
    int right(int i) const { return rgt[(size_t)i]; }
    int count(int i) const { return cnt[(size_t)i]; }
    const float *box(int i) const { return &boxes[6 * (size_t)i]; }
};
struct PlocTwin {
    rtbvh::Result r;
    int iterations = 0;
    bool ok = false;
};
PlocTwin ploc_build(const float *verts, int n) {
    PlocTwin out;
    rtbvh::Result &res = out.r;
    if (n <= 0) {
        res = rtbvh::build(verts, 0);
        out.ok = true;
        return out;
    }
    uint32_t lo_b[3] = {~0u, ~0u, ~0u}, hi_b[3] = {0u, 0u, 0u};
    for (int i = 0; i < n; i++) {
        float b[6];
        rtploc::tri_box(verts + 9 * (size_t)i, b);
        for (int a = 0; a < 3; a++) {
            lo_b[a] = std::min(lo_b[a], rtploc::ordered_bits(rtploc::centroid(b, a)));
            hi_b[a] = std::max(hi_b[a], rtploc::ordered_bits(rtploc::centroid(b, a)));
        }
    }
    float lo[3], s[3];
    for (int a = 0; a < 3; a++) {
        lo[a] = rtploc::from_ordered_bits(lo_b[a]);
        s[a] = rtploc::quant_scale(lo[a], rtploc::from_ordered_bits(hi_b[a]));
    }
    std::vector<uint64_t> keys((size_t)n);
    for (int i = 0; i < n; i++) keys[(size_t)i] = rtploc::key(verts + 9 * (size_t)i, i, lo, s);
    std::sort(keys.begin(), keys.end());
    const size_t n_all = 2 * (size_t)n - 1;
    PlocHostNodes nd;
    nd.n = n;
    nd.boxes.resize(6 * n_all);
    nd.lft.assign(n_all, -1);
    nd.rgt.assign(n_all, -1);
    nd.cnt.assign(n_all, 0);
    nd.cost.assign(n_all, 0.f);
    nd.leaf.assign(n_all, 0);
    std::vector<int> cl((size_t)n), next, nn((size_t)n);
    for (int k = 0; k < n; k++) {
        float *b = &nd.boxes[6 * (size_t)k];
        rtploc::tri_box(verts + 9 * (size_t)rtploc::key_index(keys[(size_t)k]), b);
        nd.rgt[(size_t)k] = rtploc::key_index(keys[(size_t)k]);
        nd.cnt[(size_t)k] = 1;
        nd.cost[(size_t)k] = rtploc::half_area(b) * 1.f;
        nd.leaf[(size_t)k] = 1;
        cl[(size_t)k] = k;
    }
    const float trav = rtbvh::trav_cost();
    const int max_leaf = rtbvh::max_leaf();
    int inner = 0;
    while (cl.size() > 1) {
        if (++out.iterations > rtploc::kMaxIterations) return out;
        const int m = (int)cl.size();
        const bool pair_ties = out.iterations > rtploc::kTieIterations;
        for (int i = 0; i < m; i++) {
            int best_j = -1;
            float best = 0.f;
            for (int j = std::max(0, i - rtploc::kRadius); j <= std::min(m - 1, i + rtploc::kRadius); j++) {
                if (j == i) continue;
                const float d = rtploc::distance(nd.box(cl[(size_t)i]), nd.box(cl[(size_t)j]));
                if (rtploc::nearer(d, j, i, best, best_j, pair_ties)) {
                    best_j = j;
                    best = d;
                }
            }
            nn[(size_t)i] = best_j;
        }
        next.clear();
        const int inner_before = inner;
        for (int i = 0; i < m; i++) {
            const int j = nn[(size_t)i];
            const bool mutual = nn[(size_t)j] == i;
            if (mutual && j < i) continue;  // (merged into the cluster at j)
            if (!mutual) {
                next.push_back(cl[(size_t)i]);
                continue;
            }
            const int id = n + inner++, a = cl[(size_t)i], b = cl[(size_t)j];
            rtploc::unite(nd.box(a), nd.box(b), &nd.boxes[6 * (size_t)id]);
            nd.lft[(size_t)id] = a;
            nd.rgt[(size_t)id] = b;
            nd.cnt[(size_t)id] = nd.cnt[(size_t)a] + nd.cnt[(size_t)b];
            nd.leaf[(size_t)id] = rtploc::node_cost(rtploc::half_area(nd.box(id)), nd.cnt[(size_t)id], nd.cost[(size_t)a],
                                                    nd.cost[(size_t)b], trav, max_leaf, nd.cost[(size_t)id]);
            next.push_back(id);
        }
        if (inner == inner_before) return out;  // (no mutual pair: cannot happen with finite boxes)
        cl.swap(next);
    }
    // collapse to 4-wide, breadth first from the root
    std::vector<std::pair<int, int>> level{{cl[0], 0}}, below;  // (binary node, first triangle in leaf order)
    res.order.assign((size_t)n, -1);
    res.quads.clear();
    res.num_leaves = 0;
    int levels = 0, base = 0;
    while (!level.empty()) {
        levels++;
        below.clear();
        const int next_base = base + (int)level.size();
        for (const auto &[node, first] : level) {
            int kids[4], firsts[4];
            const int nk = rtploc::expand(nd, node, first, kids, firsts);
            rtbvh::Pair rec[2] = {rtbvh::absent_quad_record(), rtbvh::absent_quad_record()};
            for (int k = 0; k < nk; k++) {
                rtbvh::Pair &p = rec[k >> 1];
                const float *b = nd.box(kids[k]);
                float *dst = (k & 1) ? p.rbox : p.lbox;
                for (int a = 0; a < 3; a++) {
                    dst[a] = rtbvh::pad_down(b[a], 2);
                    dst[3 + a] = rtbvh::pad_up(b[3 + a], 2);
                }
                int32_t link;
                if (nd.is_leaf(kids[k])) {
                    int t[8];
                    const int c = rtploc::leaf_tris(nd, kids[k], t);
                    if (c < 1 || c > 7 || firsts[k] + c > n) return out;
                    for (int q = 0; q < c; q++) res.order[(size_t)firsts[k] + q] = t[q];
                    link = rtbvh::leaf_ref(firsts[k], c);
                    res.num_leaves++;
                } else {
                    link = 2 * (next_base + (int)below.size());
                    below.push_back({kids[k], firsts[k]});
                }
                ((k & 1) ? p.rlink : p.llink) = link;
            }
            res.quads.push_back(rec[0]);
            res.quads.push_back(rec[1]);
        }
        base = next_base;
        level.swap(below);
    }
    res.max_depth = levels;
    res.stack_bound = 3 * levels + 1;
    out.ok = true;
    return out;
}

// The serial walk of both denoiser twins: `passes` a-trous passes over uv, four floats {u.x, u.y, u.z, v} per pixel (v is carried
// only with kVar), guided by px's z and n.  k[i]: pass i's kc, or with kVar ks, from which every pixel's r is formed.
template <bool kVar>
void dn_walk(std::vector<float> &uv, const std::vector<DnPixel> &px, int width, int height, int passes, const float *k, float kz,
                    int normal_power_log2) {
    std::vector<float> next(uv.size());
    for (int i = 0; i < passes; i++) {
        const long long s = 1ll << i;
        for (long long y = 0; y < height; y++)
            for (long long x = 0; x < width; x++) {
                const size_t p = (size_t)(y * width + x);
                const float kp = kVar ? dn_var_rcp(k[i], dn_var_blur(uv.data(), x, y, width, height)) : k[i];
                float sw = 0.f, sv = 0.f, su[3] = {0.f, 0.f, 0.f};
                for (int dy = -2; dy <= 2; dy++) {
                    const long long yy = y + s * dy;
                    if (yy < 0 || yy >= height) continue;
                    for (int dx = -2; dx <= 2; dx++) {
                        const long long xx = x + s * dx;
                        if (xx < 0 || xx >= width) continue;
                        const size_t q = (size_t)(yy * width + xx);
                        const float h = dn_kernel(dx) * dn_kernel(dy);
                        const float w = (dx == 0 && dy == 0) ? h
                                                             : dn_tap_weight(h, &uv[4 * p], px[p].z, px[p].n, &uv[4 * q], px[q].z, px[q].n, kp, kz,
                                                                             normal_power_log2);
                        sw = sw + w;
                        for (int c = 0; c < 3; c++) su[c] = su[c] + w * uv[4 * q + c];
                        if (kVar) sv = sv + (w * w) * uv[4 * q + 3];
                    }
                }
                for (int c = 0; c < 3; c++) next[4 * p + c] = su[c] / sw;
                next[4 * p + 3] = kVar ? sv / (sw * sw) : 0.f;
            }
        uv.swap(next);
    }
}
}  // namespace

extern "C" {
// out: [4-wide nodes, leaves, depth of the 4-wide tree, max_leaf_size, structural_errors, walk_mismatches, max_stack, max_steps
//       (node visits of the longest walk), stack_bound, binary_depth]
int rt_bvh_selfcheck(const float *verts, int n, int n_rays, const float *o3, const float *d3, int64_t *out10) {
    rtbvh::Result r = rtbvh::build(verts, n);
    memset(out10, 0, 10 * sizeof(int64_t));
    out10[0] = (int64_t)r.nodes.size();
    out10[1] = r.num_leaves;
    out10[2] = r.max_depth;
    out10[8] = r.stack_bound;
    out10[9] = r.bin_depth;
    int max_leaf = 0;
    int64_t errors = r.ok ? 0 : 1;
    if (r.quads.size() != 2 * r.nodes.size()) errors++;
    if (n > 0) {
        errors += validate(r, r.quads, true, verts, n, max_leaf);
        {   // the records as the kernels are given them (padded for the origins of this call's rays): the same structure, and
            // every plane at least 2^-24 x radius farther out than the builder's -- what the one-fma plane distance needs
            float radius[3];
            rtbvh::quads_abs_bounds(r.quads, radius);
            for (int i = 0; i < n_rays; i++)
                for (int a = 0; a < 3; a++)
                    if (std::isfinite(o3[3 * (size_t)i + a])) radius[a] = std::max(radius[a], std::fabs(o3[3 * (size_t)i + a]));
            const std::vector<rtbvh::Pair> padded = padded_quads(r, n_rays, o3);
            int ml = 0;
            errors += validate(r, padded, true, verts, n, ml);
            if (padded.size() != r.quads.size()) errors++;
            else if (!rtbvh::knob("RT_NO_ORIGIN_PAD"))
                for (size_t k = 0; k < padded.size(); k++)
                    for (int side = 0; side < 2; side++) {
                        if ((side ? padded[k].rlink : padded[k].llink) != (side ? r.quads[k].rlink : r.quads[k].llink)) errors++;
                        if ((side ? padded[k].rlink : padded[k].llink) == rtbvh::kNoChild) continue;
                        const float *pb = side ? padded[k].rbox : padded[k].lbox, *bb = side ? r.quads[k].rbox : r.quads[k].lbox;
                        for (int a = 0; a < 3; a++) {
                            const double need = std::ldexp((double)radius[a], -24);
                            if (!((double)bb[a] - (double)pb[a] >= need) || !((double)pb[3 + a] - (double)bb[3 + a] >= need)) errors++;
                        }
                    }
        }
        if (r.pairs.size() > 1 || r.pairs[0].llink != rtbvh::kNoChild) errors += validate(r, r.pairs, false, verts, n, max_leaf);
    }
    out10[3] = max_leaf;
    out10[4] = errors;
    if (errors) return 0;
    // CPU walks with the kernels' control flow vs exhaustive search, both formats
    const std::vector<Tri> tris = leaf_order_triangles(verts, r, n);
    int64_t mism = 0, max_stack = 0, max_steps = 0, mism_fmt[2] = {0, 0};
    double sum_nodes[2] = {0, 0}, sum_tris[2] = {0, 0};
    const std::vector<rtbvh::Pair> wide_recs = padded_quads(r, n_rays, o3);  // (as the kernels are given them)
    for (int i = 0; i < n_rays; i++) {
        V3 o{o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]}, d{d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]};
        float bt = FLT_MAX, t;
        int bb = -1;
        for (int k = 0; k < n; k++)
            if (tri_hit(tris[k], o, d, bt, t) && (!(t == bt && bb >= 0) || r.order[k] > r.order[bb])) { bt = t; bb = k; }
        for (int fmt = 0; fmt < 2; fmt++) {
            const bool wide = fmt == 0;
            WalkResult w = walk_ray(wide ? wide_recs : r.pairs, wide, tris, r.order, wide ? r.stack_bound : r.pair_depth + 1, 0, o, d, FLT_MAX, -1);
            if (w.failed) { mism += 1000000; continue; }
            if (w.best != bb || (bb >= 0 && w.t != bt)) { mism++; mism_fmt[fmt]++; }
            if (wide) { max_stack = std::max<int64_t>(max_stack, w.max_sp); max_steps = std::max<int64_t>(max_steps, w.nodes); }
            sum_nodes[fmt] += (double)w.nodes;
            sum_tris[fmt] += (double)w.tris;
        }
    }
    out10[5] = mism; out10[6] = max_stack; out10[7] = max_steps;
    if (getenv("RT_BVH_STATS") && n_rays > 0)
        fprintf(stderr, "bvh walk mismatches: 4-wide %lld, 2-wide %lld\n", (long long)mism_fmt[0], (long long)mism_fmt[1]);
    if (getenv("RT_BVH_STATS") && n_rays > 0)
        fprintf(stderr, "bvh walk per ray: 4-wide %.2f nodes %.2f tris | 2-wide %.2f nodes %.2f tris | %zu quads records, %zu pairs, depths %d / %d\n",
                sum_nodes[0] / n_rays, sum_tris[0] / n_rays, sum_nodes[1] / n_rays, sum_tris[1] / n_rays, r.quads.size(), r.pairs.size(), r.max_depth, r.pair_depth);
    return 0;
}

// The refit's host twin: build the tree from build_verts (rtbvh::build), refit it to new_verts (same triangle count), then
// check the result as rt_bvh_selfcheck checks a build.
// out6: [records, records whose bytes differ from the builder's records of build_verts, structural errors of the refit
//        records (as built and as padded for this call's ray origins), walk mismatches against exhaustive search over
//        new_verts (4-wide walk, closest hit), rays walked, the refit tree's surface-area cost x 10^6]
int rt_bvh_refit_check(const float *build_verts, const float *new_verts, int n, int n_rays, const float *o3, const float *d3,
                       int64_t *out6) {
    memset(out6, 0, 6 * sizeof(int64_t));
    rtbvh::Result r = rtbvh::build(build_verts, n);
    if (!r.ok || n <= 0) return 1;
    rtbvh::Result rf = r;
    rf.quads = refit_quads(r.quads, r.order, new_verts);
    out6[0] = (int64_t)rf.quads.size();
    for (size_t k = 0; k < rf.quads.size(); k++) out6[1] += memcmp(&rf.quads[k], &r.quads[k], sizeof(rtbvh::Pair)) != 0;
    int max_leaf = 0;
    const std::vector<rtbvh::Pair> padded = padded_quads(rf, n_rays, o3);
    out6[2] = validate(rf, rf.quads, true, new_verts, n, max_leaf) + validate(rf, padded, true, new_verts, n, max_leaf);
    const std::vector<Tri> tris = leaf_order_triangles(new_verts, rf, n);
    for (int i = 0; i < n_rays; i++) {
        V3 o{o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]}, d{d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]};
        float bt = FLT_MAX, t;
        int bb = -1;
        for (int k = 0; k < n; k++)
            if (tri_hit(tris[k], o, d, bt, t) && (!(t == bt && bb >= 0) || rf.order[k] > rf.order[bb])) { bt = t; bb = k; }
        WalkResult w = walk_ray(padded, true, tris, rf.order, rf.stack_bound, 0, o, d, FLT_MAX, -1);
        if (w.failed || w.best != bb || (bb >= 0 && w.t != bt)) out6[3]++;
        out6[4]++;
    }
    double cost = 0.0;  // (the form of rtbvh::sah_cost over the 4-wide children, relative to the root's bounds)
    rtbvh::Box root;
    root.reset();
    for (size_t k = 0; k < rf.quads.size(); k++)
        for (int side = 0; side < 2; side++) {
            const int32_t l = side ? rf.quads[k].rlink : rf.quads[k].llink;
            if (l == rtbvh::kNoChild) continue;
            const float *pb = side ? rf.quads[k].rbox : rf.quads[k].lbox;
            rtbvh::Box b;
            memcpy(b.lo, pb, 3 * sizeof(float));
            memcpy(b.hi, pb + 3, 3 * sizeof(float));
            cost += (double)b.half_area() * (l < 0 ? (double)((~l) & 7) : 1.0);
            if (k < 2) root.extend(b);
        }
    out6[5] = (int64_t)llround(1e6 * cost / std::max((double)root.half_area(), 1e-30));
    return 0;
}

// The host builder's 4-wide records and leaf order, as rt_ploc_build gives the twin's.  out4: [records, stack bound, depth of the
// 4-wide tree, leaves].  Returns 1 if the build failed (a leaf that cannot be referenced).
int rt_bvh_export(const float *verts, int n, void *quads_out, int64_t cap_records, int32_t *order_out, int64_t *out4) {
    memset(out4, 0, 4 * sizeof(int64_t));
    const rtbvh::Result r = rtbvh::build(verts, n);
    if (!r.ok) return 1;
    out4[0] = (int64_t)r.quads.size();
    out4[1] = r.stack_bound;
    out4[2] = r.max_depth;
    out4[3] = r.num_leaves;
    if (quads_out && cap_records >= (int64_t)r.quads.size()) memcpy(quads_out, r.quads.data(), sizeof(rtbvh::Pair) * r.quads.size());
    if (order_out && n > 0) memcpy(order_out, r.order.data(), sizeof(int32_t) * (size_t)n);
    return 0;
}

// The PLOC twin's records and leaf order.  out4: [records, iterations, depth of the 4-wide tree, leaves].  The records (64 bytes
// each) and the order are copied out when the buffers are given and large enough.  Returns 1 if the build failed.
int rt_ploc_build(const float *verts, int n, void *quads_out, int64_t cap_records, int32_t *order_out, int64_t *out4) {
    memset(out4, 0, 4 * sizeof(int64_t));
    const PlocTwin t = ploc_build(verts, n);
    if (!t.ok) return 1;
    out4[0] = (int64_t)t.r.quads.size();
    out4[1] = t.iterations;
    out4[2] = t.r.max_depth;
    out4[3] = t.r.num_leaves;
    if (quads_out && cap_records >= (int64_t)t.r.quads.size()) memcpy(quads_out, t.r.quads.data(), sizeof(rtbvh::Pair) * t.r.quads.size());
    if (order_out && n > 0) memcpy(order_out, t.r.order.data(), sizeof(int32_t) * (size_t)n);
    return 0;
}

// The PLOC twin checked as rt_bvh_selfcheck checks the host builder.
// out8: [records, structural errors (as built and as padded for this call's ray origins; leaf order not a permutation),
//        walk mismatches against exhaustive search (4-wide walk, closest hit), rays walked, the twin's surface-area cost x 10^6,
//        rtbvh::build's x 10^6 (when with_host), iterations, largest leaf]
int rt_ploc_check(const float *verts, int n, int n_rays, const float *o3, const float *d3, int with_host, int64_t *out8) {
    memset(out8, 0, 8 * sizeof(int64_t));
    const PlocTwin t = ploc_build(verts, n);
    if (!t.ok || n <= 0) return 1;
    const rtbvh::Result &r = t.r;
    out8[0] = (int64_t)r.quads.size();
    std::vector<char> seen((size_t)n, 0);
    for (int k = 0; k < n; k++) {
        const int i = r.order[(size_t)k];
        if (i < 0 || i >= n || seen[(size_t)i]) out8[1]++;
        else seen[(size_t)i] = 1;
    }
    if (out8[1]) return 0;
    int max_leaf = 0;
    const std::vector<rtbvh::Pair> padded = padded_quads(r, n_rays, o3);
    out8[1] = validate(r, r.quads, true, verts, n, max_leaf) + validate(r, padded, true, verts, n, max_leaf);
    out8[7] = max_leaf;
    if (out8[1]) return 0;
    const std::vector<Tri> tris = leaf_order_triangles(verts, r, n);
    for (int i = 0; i < n_rays; i++) {
        V3 o{o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]}, d{d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]};
        float bt = FLT_MAX, tt;
        int bb = -1;
        for (int k = 0; k < n; k++)
            if (tri_hit(tris[k], o, d, bt, tt) && (!(tt == bt && bb >= 0) || r.order[k] > r.order[bb])) { bt = tt; bb = k; }
        WalkResult w = walk_ray(padded, true, tris, r.order, r.stack_bound, 0, o, d, FLT_MAX, -1);
        if (w.failed || w.best != bb || (bb >= 0 && w.t != bt)) out8[2]++;
        out8[3]++;
    }
    out8[4] = (int64_t)llround(1e6 * quads_sah_host(r.quads));
    if (with_host) out8[5] = (int64_t)llround(1e6 * quads_sah_host(rtbvh::build(verts, n).quads));
    out8[6] = t.iterations;
    return 0;
}

// ---- CPU walk of the product's tree for arbitrary rays.  The format follows the product's choice: 4-wide unless
// RT_BVH_WIDE=0 (rt_scene_create reads the same variable).
struct HostWalk {
    rtbvh::Result r;
    std::vector<Tri> tris;     // leaf order
    std::vector<int> inverse;  // original index -> leaf-order index
    bool wide = true;
    int n = 0;
    RefView ref;               // the reference's own tree (rt_ref_tree.h), for the verified walks
};
// Bvh::traverse (bvh.cuh:251-303 / :306-357) over the reference's tree, as reference_walk in rt_walk.inc: left child
// before right child, a leaf child intersected on the spot, near inner child first by fp32 entry distance, the later
// tested triangle wins t <= tmax.  best / excl: leaf-order indices of the product (as everywhere in this file).
void literal_walk(const HostWalk &hw, int mode, V3 o, V3 d, float tmax, int excl, WalkResult &w) {
    const rtref::Tree &t = hw.ref.tree;
    w.best = -1;
    w.occluded = false;
    if (hw.n == 0) return;
    auto leaf = [&](const rtref::Node &nd) -> bool {
        for (int i = nd.link; i < nd.link + nd.count; i++) {
            const int k = hw.inverse[(size_t)t.prims[(size_t)i]];
            float tt;
            if (tri_hit(hw.tris[(size_t)k], o, d, tmax, tt)) {
                if (mode == 1) {
                    if (k != excl) { w.occluded = true; return true; }
                } else {
                    tmax = tt;
                    w.best = k;
                }
            }
        }
        return false;
    };
    if (t.nodes[0].count > 0) {
        leaf(t.nodes[0]);
    } else {
        const RefSlab s = ref_slab(o, d);
        int stk[64], sp = 0, left = t.nodes[0].link;
        while (true) {
            const rtref::Node &a = t.nodes[(size_t)left], &b = t.nodes[(size_t)left + 1];
            float el, er;
            bool gl = ref_box(s, a.box.b, el);
            if (gl && a.count > 0) { if (leaf(a)) break; gl = false; }
            bool gr = ref_box(s, b.box.b, er);
            if (gr && b.count > 0) { if (leaf(b)) break; gr = false; }
            if (gl && gr) {
                const bool right_first = el > er;
                stk[sp++] = right_first ? a.link : b.link;
                left = right_first ? b.link : a.link;
            } else if (gl) left = a.link;
            else if (gr) left = b.link;
            else { if (sp == 0) break; left = stk[--sp]; }
        }
    }
    w.t = w.best >= 0 ? tmax : 0.f;
}
void *rt_hostwalk_create(const float *verts, int n) {
    HostWalk *w = new HostWalk();
    w->n = n;
    w->r = rtbvh::build(verts, n);
    if (!w->r.ok) { delete w; return nullptr; }
    if (const char *e = rtbvh::knob("RT_BVH_WIDE")) w->wide = atoi(e) != 0;
    w->tris = leaf_order_triangles(verts, w->r, n);
    w->inverse.assign(n, 0);
    for (int k = 0; k < n; k++) w->inverse[w->r.order[k]] = k;
    w->ref.tree = rtref::build(verts, n);
    w->ref.root_leaf = w->ref.tree.nodes[0].count > 0 || n == 0;
    w->ref.leaf_of.assign((size_t)std::max(n, 1), 0);
    w->ref.parent.assign(w->ref.tree.nodes.size(), -1);
    for (size_t k = 0; k < w->ref.tree.nodes.size(); k++) {
        const rtref::Node &nd = w->ref.tree.nodes[k];
        for (int i = nd.link; nd.count > 0 && i < nd.link + nd.count; i++) w->ref.leaf_of[(size_t)w->ref.tree.prims[(size_t)i]] = (int)k;
        if (nd.count == 0 && n > 0) w->ref.parent[(size_t)nd.link] = w->ref.parent[(size_t)nd.link + 1] = (int)k;
    }
    return w;
}
void rt_hostwalk_destroy(void *h) { delete (HostWalk *)h; }
// work counters of the walks since the last reset: [0] rays [1] node steps [2] triangle tests [3] leaves visited
static long long g_walk_stats[4] = {0, 0, 0, 0};
static long long g_sp_hist[32] = {0};
// node steps of the walks since the last reset, by stack size at the step (what an LDS stack of a given depth would hold)
void rt_hostwalk_sp_hist(long long *out32, int reset) {
    for (int k = 0; k < 32; k++) {
        out32[k] = g_sp_hist[k];
        if (reset) g_sp_hist[k] = 0;
    }
}
void rt_hostwalk_stats(long long *out4, int reset) {
    for (int k = 0; k < 4; k++) {
        out4[k] = g_walk_stats[k];
        if (reset) g_walk_stats[k] = 0;
    }
}
// mode 0: closest hit -> out_i = original triangle index or -1, out_t = t;  mode 1: any hit excluding excluded[i]
// (original index or -1) -> out_i = 0 / 1.  Returns the number of rays whose walk failed (stack / step bound).
int rt_hostwalk_trace(void *h, int mode, int n_rays, const float *o3, const float *d3, const float *tmax_in, const int *excluded,
                      int *out_i, float *out_t) {
    const HostWalk &w = *(const HostWalk *)h;
    const rtbvh::Result &r = w.r;
    const std::vector<rtbvh::Pair> padded = w.wide ? padded_quads(r, n_rays, o3) : std::vector<rtbvh::Pair>();
    const std::vector<rtbvh::Pair> &rec = w.wide ? padded : r.pairs;
    const int stack_entries = w.wide ? r.stack_bound : r.pair_depth + 1;
    int failures = 0;
    long long st_nodes = 0, st_tris = 0, st_leaves = 0;
#pragma omp parallel for schedule(dynamic, 1024) reduction(+ : failures, st_nodes, st_tris, st_leaves)
    for (int i = 0; i < n_rays; i++) {
        V3 o{o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]}, d{d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]};
        const int excl = (mode == 1 && excluded[i] >= 0 && excluded[i] < w.n) ? w.inverse[excluded[i]] : -1;
        WalkResult res = walk_ray(rec, w.wide, w.tris, r.order, stack_entries, mode, o, d, tmax_in[i], excl);
        failures += res.failed ? 1 : 0;
        st_nodes += res.nodes; st_tris += res.tris; st_leaves += res.leaves;
#pragma omp critical
        for (int k = 0; k < 32; k++) g_sp_hist[k] += res.sp_hist[k];
        if (mode == 1) {
            out_i[i] = res.occluded ? 1 : 0;
        } else {
            out_i[i] = res.best >= 0 ? r.order[res.best] : -1;
            out_t[i] = res.t;
        }
    }
    g_walk_stats[0] += n_rays;
    g_walk_stats[1] += st_nodes;
    g_walk_stats[2] += st_tris;
    g_walk_stats[3] += st_leaves;
    return failures;
}
// The DEFAULT kernels' decision procedure on the CPU (k_paths / k_trace with VERIFY): the product's own walk, then
//   closest hit: the hit stands if the reference's walk can see its triangle (ref_visible) and no exact tie occurred at
//                the final distance; otherwise -- about one ray in 10^7 -- the ray is re-traced by the literal walk;
//   any hit:     the first accepted hit occludes if the reference's walk can see its triangle; if it cannot (~1 in 10^7),
//                that hit says nothing about the rest of the ray, and the literal walk decides;
//   (a ray with a -0.0 direction component: ref_visible tests every ancestor, see RefView).
// The result must equal the reference's literal walk on EVERY ray (tests/test_traversal_audit.py).
// stats6 += [rays, hits whose own box failed, hits whose leaf box failed (= hits the reference loses), exact ties at the
// final distance, -0.0 rays, literal re-traces]
int rt_hostwalk_trace_verified(void *h, int mode, int n_rays, const float *o3, const float *d3, const float *tmax_in,
                               const int *excluded, int *out_i, float *out_t, long long *stats6) {
    const HostWalk &w = *(const HostWalk *)h;
    const rtbvh::Result &r = w.r;
    const std::vector<rtbvh::Pair> padded = w.wide ? padded_quads(r, n_rays, o3) : std::vector<rtbvh::Pair>();
    const std::vector<rtbvh::Pair> &rec = w.wide ? padded : r.pairs;
    const int stack_entries = w.wide ? r.stack_bound : r.pair_depth + 1;
    int failures = 0;
    long long own = 0, leafb = 0, ties = 0, negz = 0, lit = 0;
#pragma omp parallel for schedule(dynamic, 1024) reduction(+ : failures, own, leafb, ties, negz, lit)
    for (int i = 0; i < n_rays; i++) {
        V3 o{o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]}, d{d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]};
        const int excl = (mode == 1 && excluded[i] >= 0 && excluded[i] < w.n) ? w.inverse[excluded[i]] : -1;
        const RefSlab s = ref_slab(o, d);
        WalkResult res;
        negz += s.neg_zero ? 1 : 0;
        if (mode == 1) {
            res = walk_ray(rec, w.wide, w.tris, r.order, stack_entries, 1, o, d, tmax_in[i], excl, &w.ref);
            if (res.unseen_occluder) {
                lit++;
                const bool failed = res.failed;
                const long long of = res.own_fail, lf = res.leaf_fail;
                literal_walk(w, 1, o, d, tmax_in[i], excl, res);
                res.failed = failed; res.own_fail = of; res.leaf_fail = lf;
            }
        } else {
            res = walk_ray(rec, w.wide, w.tris, r.order, stack_entries, 0, o, d, tmax_in[i], -1);
            if (res.best >= 0) {
                const bool tie = res.tie_t == res.t;
                const bool seen = ref_visible(w.ref, s, w.tris[(size_t)res.best], r.order[(size_t)res.best], res);
                ties += tie ? 1 : 0;
                if (tie || !seen) {
                    lit++;
                    const bool failed = res.failed;
                    literal_walk(w, 0, o, d, tmax_in[i], -1, res);
                    res.failed = failed;
                }
            }
        }
        failures += res.failed ? 1 : 0;
        own += res.own_fail; leafb += res.leaf_fail;
        if (mode == 1) {
            out_i[i] = res.occluded ? 1 : 0;
        } else {
            out_i[i] = res.best >= 0 ? r.order[res.best] : -1;
            out_t[i] = res.t;
        }
    }
    if (stats6) { stats6[0] += n_rays; stats6[1] += own; stats6[2] += leafb; stats6[3] += ties; stats6[4] += negz; stats6[5] += lit; }
    return failures;
}
// The reference's own tree as the product builds it for RT_FLAG_REFERENCE_WALK (rt_ref_tree.h), for a node-by-node
// comparison with the oracle's restatement of Bvh::Bvh (tests/test_host_logic.py).  Call with bounds6 == nullptr for the
// sizes: returns the node count; *depth receives the tree depth.  prims: reference position -> caller's triangle index.
int rt_ref_tree_export(const float *tri9, int n, float *bounds6, int *count, int *link, int *prims, int *depth) {
    const rtref::Tree t = rtref::build(tri9, n);
    if (depth) *depth = t.depth;
    if (bounds6) {
        for (size_t i = 0; i < t.nodes.size(); i++) {
            memcpy(bounds6 + 6 * i, t.nodes[i].box.b, 24);
            count[i] = t.nodes[i].count;
            link[i] = t.nodes[i].link;
        }
        for (size_t i = 0; i < t.prims.size(); i++) prims[i] = t.prims[i];
    }
    return (int)t.nodes.size();
}
// The persistent launch as render_shard_impl plans it (tests/test_launch_plan_host.py); out10: PathsLaunch's fields in order.
void rt_plan_paths_launch(int n, int cus, int wide, int n_nodes, int paths_cap, int lattice, int width, int spp, int64_t fixed_lds_bytes, int64_t *out10) {
    const rtplan::PathsLaunch p = rtplan::plan_paths_launch(n, cus, wide != 0, n_nodes, paths_cap, lattice != 0, width, spp, (size_t)fixed_lds_bytes);
    const int64_t v[10] = {p.blocks, p.few_blocks, (int64_t)p.lds_bytes, p.top_n, p.adv_batch, p.gen_batch, p.tri_follow, p.prio_rotate, p.rot_wave, p.rot_set};
    memcpy(out10, v, sizeof(v));
}
// The chunked deal (tests/test_slot_chunks_host.py).  Tasks t0 .. t0 + count - 1 of workgroup `block`: the slot and the level of each.
void rt_slot_chunk_tasks(int block, int sets, int lanes_in_grid, int rot_wave, int rot_set, uint32_t t0, int count, int32_t *slots, int32_t *levels) {
    for (int k = 0; k < count; k++) {
        const rtchunks::Entry e = rtchunks::task_entry(t0 + (uint32_t)k, (unsigned)sets);
        slots[k] = rtchunks::slot_of(e.set, (unsigned)block * rtchunks::kLanes + e.lane, (unsigned)lanes_in_grid, (unsigned)rot_wave, (unsigned)rot_set);
        levels[k] = (int32_t)e.level;
    }
}
// the static deal: the slot of (set, lane of the grid)
int rt_slot_chunk_static_slot(int set, int lane_in_grid, int lanes_in_grid, int rot_wave, int rot_set) {
    return rtchunks::slot_of((unsigned)set, (unsigned)lane_in_grid, (unsigned)lanes_in_grid, (unsigned)rot_wave, (unsigned)rot_set);
}
uint32_t rt_slot_chunk_levels(uint32_t rays, uint32_t G) { return rtchunks::levels(rays, G); }
uint32_t rt_slot_chunk_task_count(uint32_t sets, uint32_t rays, uint32_t G) { return rtchunks::task_count(sets, rays, G); }
int rt_slot_chunk_ends(uint32_t gen, uint32_t G, int fresh) { return rtchunks::chunk_ends(gen, rtchunks::multiple_of(G), fresh != 0); }
// the limit of a run over background pixels in k_paths<PathsBg>'s GEN block (tests/test_chunk_limit_host.py)
uint32_t rt_slot_chunk_next_multiple(uint32_t gen, uint32_t G) { return rtchunks::next_multiple(gen, G, rtchunks::next_multiple_mul(G)); }
uint32_t rt_slot_chunk_run_limit(uint32_t gen, uint32_t g_stop, int dealt, int can_loop, uint32_t G) {
    return rtchunks::run_limit(gen, g_stop, dealt != 0, can_loop != 0, G, rtchunks::next_multiple_mul(G));
}
// Every run the GEN block can be asked for with G in [g_lo, g_hi]: gen in 0 .. 2 047, g_stop in {gen + 1, the next multiple of
// G above gen - 1, that multiple, that multiple + 1, 2 047} (where gen < g_stop: only such a lane runs), dealt and not, can_loop
// and not.  Over background pixels only, a run is walked twice: with the stop tests made turn by turn -- can_loop, gen < g_stop,
// chunk_ends(gen, multiple_of(G), false) -- and against run_limit, fixed before the first turn.  out4: [runs walked, runs whose
// two walks stop at different generations, G and gen of the first such run].  (The multiple in g_stop is found by counting.)
void rt_slot_chunk_run_limit_check(uint32_t g_lo, uint32_t g_hi, int64_t *out4) {
    int64_t runs = 0, bad = 0, first_G = -1, first_gen = -1;
#pragma omp parallel for schedule(dynamic, 8) reduction(+ : runs, bad)
    for (int64_t G = g_lo; G <= (int64_t)g_hi; G++) {
        const rtchunks::Multiple m = rtchunks::multiple_of((uint32_t)G);
        const uint32_t mul = rtchunks::next_multiple_mul((uint32_t)G);
        uint32_t next = 0;  // the smallest multiple of G above gen
        for (uint32_t gen = 0; gen <= 2047u; gen++) {
            if (next <= gen) next += (uint32_t)G;
            const uint32_t stops[5] = {gen + 1u, next - 1u, next, next + 1u, 2047u};
            for (uint32_t g_stop : stops) {
                if (!(gen < g_stop)) continue;
                for (int dealt = 0; dealt < 2; dealt++)
                    for (int can_loop = 0; can_loop < 2; can_loop++) {
                        uint32_t a = gen, b = gen;
                        do a++;
                        while (can_loop && a < g_stop && !(dealt && rtchunks::chunk_ends(a, m, false)));
                        const uint32_t limit = rtchunks::run_limit(gen, g_stop, dealt != 0, can_loop != 0, (uint32_t)G, mul);
                        do b++;
                        while (b < limit);
                        runs++;
                        if (a != b) {
                            bad++;
#pragma omp critical
                            if (first_G < 0 || G < first_G) {
                                first_G = G;
                                first_gen = gen;
                            }
                        }
                    }
            }
        }
    }
    out4[0] = runs;
    out4[1] = bad;
    out4[2] = first_G;
    out4[3] = first_gen;
}
int rt_slot_chunk_taker_runs(int old_sem) { return rtchunks::taker_runs(old_sem); }
int rt_slot_chunk_runner_keeps(int old_sem) { return rtchunks::runner_keeps(old_sem); }
// G as the launch plan picks it for a frame whose slots run `chain` camera rays in k_paths (0: the static deal)
int rt_plan_slot_chunk(int n, int cus, int chain) {
    return rtplan::slot_chunk_for(rtplan::plan_paths_launch(n, cus, true, 70000, 10, true, 1920, 256, 0), chain);
}
// The static head and the packed semaphores of the chunked deal (tests/test_slot_chunks_head_host.py).
// the head the plan picks for a shard of n slots (n / (workgroups x 256) slot sets per lane); *sets_out: those sets
int rt_plan_slot_head(int n, int cus, int *sets_out) {
    const rtplan::PathsLaunch p = rtplan::plan_paths_launch(n, cus, true, 70000, 10, true, 1920, 256, 0);
    const int sets = n / (p.blocks * rtplan::kBlock);
    if (sets_out) *sets_out = sets;
    return rtplan::slot_head_for(p, sets);
}
int rt_plan_slot_chunk_if_resident(int chunk, int workgroups_per_cu) { return rtplan::slot_chunk_if_resident(chunk, workgroups_per_cu); }
// the dealt entry (head + set, lane) of a task, as k_paths<PathsChunked> maps it: the slot, the level and the entry's index
void rt_slot_chunk_head_tasks(int block, int sets, int head, int lanes_in_grid, int rot_wave, int rot_set, uint32_t t0, int count, int32_t *slots, int32_t *levels, int32_t *idx) {
    for (int k = 0; k < count; k++) {
        const rtchunks::Entry e = rtchunks::task_entry(t0 + (uint32_t)k, (unsigned)(sets - head));
        slots[k] = rtchunks::slot_of(e.set + (unsigned)head, (unsigned)block * rtchunks::kLanes + e.lane, (unsigned)lanes_in_grid, (unsigned)rot_wave, (unsigned)rot_set);
        levels[k] = (int32_t)e.level;
        idx[k] = (int32_t)(e.set * rtchunks::kLanes + e.lane);
    }
}
// the inverse of the static deal: out2 = {slot set, lane of the grid}
void rt_slot_chunk_owner(int slot, int lanes_in_grid, int rot_wave, int rot_set, int32_t *out2) {
    const rtchunks::Owner o = rtchunks::owner_of((unsigned)slot, (unsigned)lanes_in_grid, (unsigned)rot_wave, (unsigned)rot_set);
    out2[0] = (int32_t)o.set;
    out2[1] = (int32_t)o.lane_in_grid;
}
uint32_t rt_slot_chunk_sem_word(uint32_t idx) { return rtchunks::sem_word(idx); }
uint32_t rt_slot_chunk_sem_unit(uint32_t idx) { return rtchunks::sem_unit(idx); }
int rt_slot_chunk_sem_value(uint32_t word, uint32_t idx) { return rtchunks::sem_value(word, idx); }
uint32_t rt_slot_chunk_sem_init() { return rtchunks::kSemWordInit; }
// The pixel rectangle outside which k_paths makes no camera ray (rt_background.h, tests/test_background_rect_host.py), as
// render_shard_impl computes it from the bounds lo / hi of the scene's records; out4 = {x0, y0, x1, y1}.  Returns 0, or 1
// (and writes nothing) for a null argument or a frame without pixels.
int rt_background_rect(const float cam12[12], int width, int height, const float lo[3], const float hi[3], int out4[4]) {
    if (!cam12 || !lo || !hi || !out4 || width <= 0 || height <= 0) return 1;
    const rtbg::Rect r = rtbg::background_rect(cam12, width, height, lo, hi);
    out4[0] = r.x0;
    out4[1] = r.y0;
    out4[2] = r.x1;
    out4[3] = r.y1;
    return 0;
}
// The CPU twin of rt_denoise_fixed (tests/test_denoise_host.py): a plain serial loop over the arithmetic the kernels use
// (rt_denoise.h), host buffers throughout, the same checks of the parameters.  Returns 0, or 1 and writes nothing.
int hc_denoise(const int64_t *sum_fixed, int num_samples, const int64_t *aov_fixed, int aov_samples, int width, int height, int passes,
               float sigma_color, float sigma_depth, int normal_power_log2, float *rgb_out) {
    if (!sum_fixed || !aov_fixed || !rgb_out || width < 1 || height < 1 || num_samples < 1 || aov_samples < 1) return 1;
    if (passes < 0 || passes > DN_MAX_PASSES || normal_power_log2 < 0 || normal_power_log2 > DN_MAX_NORMAL_POWER_LOG2) return 1;
    if (!(std::isfinite(sigma_color) && sigma_color > 0.f && std::isfinite(sigma_depth) && sigma_depth > 0.f)) return 1;
    const float sc2 = sigma_color * sigma_color, sd2 = sigma_depth * sigma_depth;
    const float kz = 1.f / sd2;
    float kc[DN_MAX_PASSES];
    for (int i = 0; i < passes; i++) {
        kc[i] = (float)(1 << (2 * i)) / sc2;
        if (!(std::isfinite(kc[i]) && kc[i] > 0.f)) return 1;
    }
    if (!(std::isfinite(kz) && kz > 0.f)) return 1;
    const size_t n = (size_t)width * (size_t)height;
    const float inv_spp = 1.f / (float)num_samples, inv_aov = 1.f / (float)aov_samples;
    std::vector<DnPixel> px(n);
    std::vector<float> uv(4 * n, 0.f);
    for (size_t p = 0; p < n; p++) {
        dn_prepare(sum_fixed + 3 * p, aov_fixed + DN_AOV_CHANNELS * p, inv_spp, inv_aov, &px[p]);
        for (int k = 0; k < 3; k++) uv[4 * p + k] = px[p].u[k];
    }
    dn_walk<false>(uv, px, width, height, passes, kc, kz, normal_power_log2);
    for (size_t p = 0; p < n; p++) dn_finish(&uv[4 * p], px[p].d, px[p].e, rgb_out + 3 * p);
    return 0;
}
// rt_expnegf on n values (tests/test_denoise_host.py holds it to its numpy restatement and to exp)
void hc_expnegf(const float *x, float *y, int n) {
    for (int k = 0; k < n; k++) y[k] = rt_expnegf(x[k]);
}
// The CPU twin of rt_denoise_dual_fixed (tests/test_denoise_dual_host.py, tools/denoise_dual_quality.py): a serial loop over
// rt_denoise.h, host buffers throughout, the same checks of the parameters.  var_out (may be null): the final v per pixel.
// Returns 0, or 1 and writes nothing.
int hc_denoise_dual(const int64_t *sum_a, int samples_a, const int64_t *sum_b, int samples_b, const int64_t *aov_fixed, int aov_samples,
                    int width, int height, int passes, float sigma_variance, float sigma_depth, int normal_power_log2, float *rgb_out,
                    float *var_out) {
    if (!sum_a || !sum_b || !aov_fixed || !rgb_out || width < 1 || height < 1 || samples_a < 1 || samples_b < 1 || aov_samples < 1) return 1;
    if ((long long)samples_a + samples_b > 0x7fffffffll) return 1;
    if (passes < 0 || passes > DN_MAX_PASSES || normal_power_log2 < 0 || normal_power_log2 > DN_MAX_NORMAL_POWER_LOG2) return 1;
    if (!(std::isfinite(sigma_variance) && sigma_variance > 0.f && std::isfinite(sigma_depth) && sigma_depth > 0.f)) return 1;
    const float ks = sigma_variance * sigma_variance, sd2 = sigma_depth * sigma_depth;
    const float kz = 1.f / sd2;
    if (!(std::isfinite(ks) && ks > 0.f && std::isfinite(kz) && kz > 0.f)) return 1;
    const int ns = samples_a + samples_b;
    const float kv = (float)((double)samples_a * (double)samples_b / ((double)ns * (double)ns));
    const float inv_a = 1.f / (float)samples_a, inv_b = 1.f / (float)samples_b, inv_n = 1.f / (float)ns, inv_aov = 1.f / (float)aov_samples;
    const size_t n = (size_t)width * (size_t)height;
    std::vector<DnPixel> px(n);
    std::vector<float> uv(4 * n);
    for (size_t p = 0; p < n; p++) {
        uv[4 * p + 3] = dn_prepare_dual(sum_a + 3 * p, sum_b + 3 * p, aov_fixed + DN_AOV_CHANNELS * p, inv_a, inv_b, inv_n, inv_aov, kv, &px[p]);
        for (int k = 0; k < 3; k++) uv[4 * p + k] = px[p].u[k];
    }
    const float k[DN_MAX_PASSES] = {ks, ks, ks, ks, ks, ks, ks, ks};
    dn_walk<true>(uv, px, width, height, passes, k, kz, normal_power_log2);
    for (size_t p = 0; p < n; p++) {
        dn_finish(&uv[4 * p], px[p].d, px[p].e, rgb_out + 3 * p);
        if (var_out) var_out[p] = uv[4 * p + 3];
    }
    return 0;
}
// The CPU twin of k_motion's finish (tests/test_temporal_host.py, tools/temporal_quality.py): the previous position and the
// projection of rt_render_motion on GIVEN hits -- tri (the caller's order, < 0: a miss), u, v per pixel; the hits themselves are
// the walk's and are pinned elsewhere.  prev_tris: n_tris x 9, the vertices of one frame ago (pass the current ones when nothing
// moved: tri_point on a row is the operations of the scene's stored record).  Returns 0, or 1 and writes nothing.
int hc_motion_records(int n, const int32_t *tri, const float *u, const float *v, const float *prev_tris, int n_tris, const float *prev_cam12,
                      int width, int height, float *motion4) {
    if (n < 0 || !tri || !u || !v || !prev_tris || !prev_cam12 || !motion4 || width < 1 || height < 1) return 1;
    for (int p = 0; p < n; p++)
        if (tri[p] >= n_tris) return 1;
    TmCamera c;
    tm_camera(prev_cam12, width, height, &c);
    for (int p = 0; p < n; p++) {
        float *rec = motion4 + 4 * (size_t)p;
        const int32_t k = tri[p] < 0 ? -1 : tri[p];
        rec[0] = rec[1] = rec[2] = 0.f;
        if (k >= 0) {
            float P[3];
            tm_point_of_vertices(prev_tris + 9 * (size_t)k, u[p], v[p], P);
            tm_project(&c, P, rec);
        }
        memcpy(rec + 3, &k, 4);
    }
    return 0;
}
// The CPU twin of rt_temporal_accumulate_moments_fixed (tests/test_temporal_moments_host.py, tools/temporal_moments_quality.py):
// a serial loop over rt_temporal.h's tm_accumulate_moments_pixel, host buffers throughout, the same checks of the parameters and
// of which pointers go together (not the alignment and overlap checks: the caller's).  Returns 0, or 1 and writes nothing.
int hc_temporal_accumulate_moments(const int64_t *sum_a, int samples_a, const int64_t *sum_b, int samples_b, const int64_t *aov_fixed,
                                   int aov_samples, const float *motion4, const int64_t *hist_a_in, const int64_t *hist_b_in,
                                   const int32_t *len_in, const int64_t *prev_aov_fixed, int prev_aov_samples, const float *prev_motion4,
                                   const float *moments_in, int width, int height, int max_history, float alpha_min, float depth_tolerance,
                                   float normal_cos_min, float emission_tolerance, int variance_min_history, int64_t *hist_a_out,
                                   int64_t *hist_b_out, int32_t *len_out, float *moments_out, float *variance_out) {
    if (!sum_a || !aov_fixed || !motion4 || !hist_a_out || !len_out || width < 1 || height < 1 || samples_a < 1 || aov_samples < 1) return 1;
    const bool two = sum_b != nullptr, history = hist_a_in != nullptr, moments = moments_out != nullptr;
    if (two != (hist_b_out != nullptr) || (two && samples_b < 1)) return 1;
    if (!history && (hist_b_in || len_in || prev_aov_fixed || moments_in || prev_motion4)) return 1;
    if (history && (!len_in || !prev_aov_fixed || prev_aov_samples < 1 || two != (hist_b_in != nullptr))) return 1;
    if (moments != (variance_out != nullptr) || (moments_in && !moments)) return 1;
    if (moments && two && (long long)samples_a + samples_b > 0x7fffffffll) return 1;
    if (max_history < 1 || !(alpha_min > 0.f && alpha_min <= 1.f) || !(std::isfinite(depth_tolerance) && depth_tolerance > 0.f)) return 1;
    if (!(normal_cos_min >= -1.f && normal_cos_min <= 1.f) || !(emission_tolerance >= 0.f) || variance_min_history < 1) return 1;
    TmMoments t{};
    tm_moments_fill(&t, sum_a, samples_a, sum_b, samples_b, aov_fixed, aov_samples, motion4, hist_a_in, hist_b_in, len_in, prev_aov_fixed,
                    prev_aov_samples, prev_motion4, moments_in, width, height, 0, max_history, alpha_min, depth_tolerance, normal_cos_min,
                    emission_tolerance, variance_min_history, hist_a_out, hist_b_out, len_out, moments_out, variance_out);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) tm_accumulate_moments_pixel(&t, x, y, motion4 + 4 * ((size_t)y * width + x));
    return 0;
}
// The CPU twin of rt_temporal_accumulate_fixed (tests/test_temporal_host.py, tools/temporal_quality.py), as the entry point is: the
// twin above with the emission stop, the triangle stop and the moments off.
int hc_temporal_accumulate(const int64_t *sum_a, int samples_a, const int64_t *sum_b, int samples_b, const int64_t *aov_fixed, int aov_samples,
                           const float *motion4, const int64_t *hist_a_in, const int64_t *hist_b_in, const int32_t *len_in,
                           const int64_t *prev_aov_fixed, int prev_aov_samples, int width, int height, int max_history, float alpha_min,
                           float depth_tolerance, float normal_cos_min, int64_t *hist_a_out, int64_t *hist_b_out, int32_t *len_out) {
    return hc_temporal_accumulate_moments(sum_a, samples_a, sum_b, samples_b, aov_fixed, aov_samples, motion4, hist_a_in, hist_b_in, len_in,
                                          prev_aov_fixed, prev_aov_samples, nullptr, nullptr, width, height, max_history, alpha_min,
                                          depth_tolerance, normal_cos_min, INFINITY, 1, hist_a_out, hist_b_out, len_out, nullptr, nullptr);
}
// The CPU twin of rt_denoise_variance_fixed (tests/test_denoise_variance_host.py, tools/temporal_moments_quality.py): hc_denoise_dual's
// walk on one frame's sums and the caller's variance.  var_out (may be null): the final v per pixel.  Returns 0, or 1 and writes nothing.
int hc_denoise_variance(const int64_t *sum_fixed, int num_samples, const float *variance, const int64_t *aov_fixed, int aov_samples, int width,
                        int height, int passes, float sigma_variance, float sigma_depth, int normal_power_log2, float *rgb_out, float *var_out) {
    if (!sum_fixed || !variance || !aov_fixed || !rgb_out || width < 1 || height < 1 || num_samples < 1 || aov_samples < 1) return 1;
    if (passes < 0 || passes > DN_MAX_PASSES || normal_power_log2 < 0 || normal_power_log2 > DN_MAX_NORMAL_POWER_LOG2) return 1;
    if (!(std::isfinite(sigma_variance) && sigma_variance > 0.f && std::isfinite(sigma_depth) && sigma_depth > 0.f)) return 1;
    const float ks = sigma_variance * sigma_variance, sd2 = sigma_depth * sigma_depth;
    const float kz = 1.f / sd2;
    if (!(std::isfinite(ks) && ks > 0.f && std::isfinite(kz) && kz > 0.f)) return 1;
    const float inv_spp = 1.f / (float)num_samples, inv_aov = 1.f / (float)aov_samples;
    const size_t n = (size_t)width * (size_t)height;
    std::vector<DnPixel> px(n);
    std::vector<float> uv(4 * n);
    for (size_t p = 0; p < n; p++) {
        uv[4 * p + 3] = dn_prepare_var(sum_fixed + 3 * p, aov_fixed + DN_AOV_CHANNELS * p, variance[p], inv_spp, inv_aov, &px[p]);
        for (int k = 0; k < 3; k++) uv[4 * p + k] = px[p].u[k];
    }
    const float k[DN_MAX_PASSES] = {ks, ks, ks, ks, ks, ks, ks, ks};
    dn_walk<true>(uv, px, width, height, passes, k, kz, normal_power_log2);
    for (size_t p = 0; p < n; p++) {
        dn_finish(&uv[4 * p], px[p].d, px[p].e, rgb_out + 3 * p);
        if (var_out) var_out[p] = uv[4 * p + 3];
    }
    return 0;
}
// The CPU twin of rt_upsample_fixed (sum_lo) and rt_upsample_rgb (rgb_lo; exactly one of the two is given) (tests/test_upsample_host.py,
// tools/upsample_quality.py): a serial loop over rt_upsample.h, host buffers throughout, the same checks of the parameters.
// rgb_out, out_fixed: at least one; form_out (may be null): UP_GUIDED / UP_TENT / UP_SHORTCUT per full pixel.  Returns 0, or 1 and
// writes nothing.
int hc_upsample(const int64_t *sum_lo, const float *rgb_lo, int num_samples, const int64_t *aov_lo, int aov_samples_lo, int low_width,
                int low_height, int factor, const int64_t *aov_hi, int aov_samples_hi, float sigma_depth, int normal_power_log2, float *rgb_out,
                int64_t *out_fixed, uint8_t *form_out) {
    if ((sum_lo != nullptr) == (rgb_lo != nullptr) || !aov_lo || !aov_hi || (!rgb_out && !out_fixed)) return 1;
    if (factor < UP_MIN_FACTOR || factor > UP_MAX_FACTOR || low_width < 1 || low_height < 1) return 1;
    if ((long long)low_width * low_height > (0x7fffffff / 3) / ((long long)factor * factor)) return 1;
    if ((sum_lo && num_samples < 1) || aov_samples_lo < 1 || aov_samples_hi < 1) return 1;
    if (normal_power_log2 < 0 || normal_power_log2 > DN_MAX_NORMAL_POWER_LOG2 || !(std::isfinite(sigma_depth) && sigma_depth > 0.f)) return 1;
    const float sd2 = sigma_depth * sigma_depth;
    const float kz = 1.f / sd2;
    if (!(std::isfinite(kz) && kz > 0.f)) return 1;
    const float inv_spp = 1.f / (float)num_samples, inv_lo = 1.f / (float)aov_samples_lo, inv_hi = 1.f / (float)aov_samples_hi;
    const size_t n_lo = (size_t)low_width * (size_t)low_height;
    std::vector<UpLow> lo(n_lo);
    for (size_t q = 0; q < n_lo; q++) {
        if (sum_lo)
            up_low_of_sums(sum_lo + 3 * q, aov_lo + DN_AOV_CHANNELS * q, inv_spp, inv_lo, &lo[q]);
        else
            up_low_of_rgb(rgb_lo + 3 * q, aov_lo + DN_AOV_CHANNELS * q, inv_lo, &lo[q]);
    }
    const int width = factor * low_width, height = factor * low_height;
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t p = (size_t)y * (size_t)width + (size_t)x;
            float out[3];
            const int form = up_full_pixel(x, y, factor, low_width, low_height, aov_hi + DN_AOV_CHANNELS * p, inv_hi, kz, normal_power_log2,
                                           [&](int qx, int qy, UpLow *q) { *q = lo[(size_t)qy * (size_t)low_width + (size_t)qx]; }, out);
            for (int k = 0; k < 3; k++) {
                if (rgb_out) rgb_out[3 * p + k] = out[k];
                if (out_fixed) out_fixed[3 * p + k] = tm_to_fixed(out[k]);
            }
            if (form_out) form_out[p] = (uint8_t)form;
        }
    return 0;
}
// The stats of a frame from its n shards' (rt_stats_merge.h), as RT_SPLIT (sub_shards != 0) and rt_render_multi merge them
void hc_merge_shard_stats(const rt_stats *sub, int n, int sub_shards, rt_stats *out) { *out = merge_shard_stats(sub, n, sub_shards != 0); }
}
