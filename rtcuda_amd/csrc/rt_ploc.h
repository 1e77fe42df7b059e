// rt_ploc.h -- the arithmetic of the device BVH builder (PLOC, parallel locally-ordered clustering, Meister & Bittner 2018),
// shared by its kernels (k_ploc_* in rt_build_kernels.inc) and its sequential host twin (rt_host_check.cpp).  Both are built with
// -ffp-contract=off, so every expression below is rounded operation by operation in the order written, on the device as on
// the host: the same bits.  (fminf / fmaxf may disagree on the sign of a zero; no result below depends on it.)
//
// The build, a deterministic function of the vertices:
//   1. keys: centroid c = 0.5 (lo + hi) of every triangle's box, quantised within the centroids' bounds to 13 bits per axis;
//      key = (39-bit Morton code << 24) | original triangle index (unique: scenes have fewer than 2^24 triangles), sorted.
//   2. clusters (exact fp32 box + node id) in key order.  Per iteration every cluster i picks its nearest neighbour j in
//      [i - kRadius, i + kRadius], j != i, by the half surface area of the union of the two boxes (ties: the smaller j; after
//      kTieIterations iterations: the neighbour i ^ 1, see nearer());
//      mutual nearest neighbours merge into a new inner node at the smaller position; survivors are compacted in order and
//      new node ids come from the prefix sum of the merges.  Until one cluster is left.
//   3. leaves, bottom up at merge time: a node of at most max_leaf triangles is a leaf when n * A <= trav * A + C(l) + C(r).
//   4. collapse to 4-wide top down, breadth first: while a node has fewer than four children, its inner child with the
//      largest half area (the first of equals) is replaced by that child's two children, appended at the end; leaf
//      triangles in depth-first order, the lower position first.
#ifndef RT_PLOC_H
#define RT_PLOC_H

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RT_PLOC_HD __host__ __device__ inline
#else
#define RT_PLOC_HD inline
#endif

namespace rtploc {

constexpr int kRadius = 16;        // search window of the nearest-neighbour step
constexpr int kQuantBits = 13;     // per axis: 39 Morton bits + 24 index bits in a 64-bit key
constexpr int kIndexBits = 24;
constexpr int kMaxIterations = 4096;
constexpr int kTieIterations = 64;  // iterations after which equal distances are broken by position parity (see nearer())

// A float's bits as an unsigned integer in the float's order (min / max of the centroid bounds as integer atomics)
RT_PLOC_HD uint32_t ordered_bits(float f) {
    union { float f; uint32_t u; } c;
    c.f = f;
    return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}
RT_PLOC_HD float from_ordered_bits(uint32_t u) {
    union { float f; uint32_t u; } c;
    c.u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return c.f;
}

RT_PLOC_HD void tri_box(const float *v, float b[6]) {
    for (int a = 0; a < 3; a++) {
        b[a] = fminf(v[a], fminf(v[3 + a], v[6 + a]));
        b[3 + a] = fmaxf(v[a], fmaxf(v[3 + a], v[6 + a]));
    }
}
RT_PLOC_HD float centroid(const float b[6], int a) { return (b[a] + b[3 + a]) * 0.5f; }
// scale of the quantisation of one axis from the centroids' bounds (host side, passed to the key kernel)
inline float quant_scale(float lo, float hi) { return hi > lo ? 8191.f / (hi - lo) : 0.f; }
RT_PLOC_HD uint32_t quantise(float c, float lo, float s) { return (uint32_t)fminf(fmaxf((c - lo) * s, 0.f), 8191.f); }
RT_PLOC_HD uint64_t spread3(uint32_t v) {  // 13 bits -> every third bit of 39
    uint64_t x = v & 0x1fffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
RT_PLOC_HD uint64_t key(const float *v, int index, const float lo[3], const float s[3]) {
    float b[6];
    tri_box(v, b);
    const uint64_t m = (spread3(quantise(centroid(b, 0), lo[0], s[0])) << 2) | (spread3(quantise(centroid(b, 1), lo[1], s[1])) << 1) |
                       spread3(quantise(centroid(b, 2), lo[2], s[2]));
    return (m << kIndexBits) | (uint64_t)(uint32_t)index;
}
RT_PLOC_HD int key_index(uint64_t k) { return (int)(k & ((1ull << kIndexBits) - 1)); }

RT_PLOC_HD float half_area(const float b[6]) {
    const float e0 = b[3] - b[0], e1 = b[4] - b[1], e2 = b[5] - b[2];
    return (e0 + e1) * e2 + e0 * e1;
}
RT_PLOC_HD void unite(const float a[6], const float b[6], float u[6]) {
    for (int k = 0; k < 3; k++) {
        u[k] = fminf(a[k], b[k]);
        u[3 + k] = fmaxf(a[3 + k], b[3 + k]);
    }
}
RT_PLOC_HD float distance(const float a[6], const float b[6]) {
    float u[6];
    unite(a, b, u);
    return half_area(u);
}
// The nearest-neighbour choice of cluster i, candidates j in ascending order: does j at distance d replace best_j at `best`?
// A smaller distance does, so ties go to the smaller j.  On a run of EQUAL boxes (duplicated triangles, triangles that fp32
// collapsed to points) every distance is the same, every cluster but the first names the start of its window, and one pair
// merges per iteration.  From iteration kTieIterations + 1 on (`pair_ties`) a tie goes to the neighbour i ^ 1, which names i
// in turn: half of a run merges per iteration.  Builds that end earlier never see the rule, and those are the builds of
// distinct boxes: the iterations grow by about 1.5 per doubling of the scene -- 47 for 69 463 triangles, 50 for 277 816,
// 51 for 1.1 million and 60 for 8.9 million (the bunny tiled 16 and 128 times), and the key holds fewer than 2^24 = 16.8
// million.  A scene that does pass 64 without a run of equal boxes is changed only where two candidates of a cluster lie at
// EXACTLY the same distance and one of them is i ^ 1; either choice is a nearest neighbour, and the tree stays a function of
// the vertices, the same on the device and in the twin.
RT_PLOC_HD bool nearer(float d, int j, int i, float best, int best_j, bool pair_ties) {
    return best_j < 0 || d < best || (pair_ties && d == best && j == (i ^ 1));
}
// A new inner node of `count` triangles and box area `area` over children of cost cl, cr: its cost, and whether it is a leaf
RT_PLOC_HD bool node_cost(float area, int count, float cl, float cr, float trav, int max_leaf, float &cost) {
    const float c_leaf = area * (float)count;
    const float c_split = area * trav + (cl + cr);
    const bool leaf = count <= max_leaf && c_split >= c_leaf;
    cost = leaf ? c_leaf : c_split;
    return leaf;
}

// The binary tree both sides build, seen through `Nodes`: node ids 0 .. n - 1 are the triangles in key order, n .. 2n - 2 the
// merges in the order they were made (the last one the root).  Nodes provides is_leaf(i) (a leaf of the final tree: a
// triangle, or a node the cost model keeps whole), is_tri(i), tri(i) (original index), left(i), right(i), count(i), box(i).
//
// The children of the 4-wide node made from binary node `node` whose triangles start at `first` in leaf order: the binary
// node's two children, then the inner child with the largest surface area is opened (removed, its two children appended)
// until there are four.  A node that is itself a leaf has that leaf as its one child (a tree of one leaf).  Returns the count.
template <class Nodes>
RT_PLOC_HD int expand(const Nodes &nd, int node, int first, int kids[4], int firsts[4]) {
    if (nd.is_leaf(node)) {
        kids[0] = node;
        firsts[0] = first;
        return 1;
    }
    kids[0] = nd.left(node);
    kids[1] = nd.right(node);
    firsts[0] = first;
    firsts[1] = first + nd.count(kids[0]);
    int nk = 2;
    while (nk < 4) {
        int best = -1;
        float best_area = 0.f;
        for (int k = 0; k < nk; k++)
            if (!nd.is_leaf(kids[k])) {
                const float a = half_area(nd.box(kids[k]));
                if (best < 0 || a > best_area) {
                    best = k;
                    best_area = a;
                }
            }
        if (best < 0) break;
        const int opened = kids[best], f = firsts[best];
        for (int k = best; k + 1 < nk; k++) {
            kids[k] = kids[k + 1];
            firsts[k] = firsts[k + 1];
        }
        kids[nk - 1] = nd.left(opened);
        firsts[nk - 1] = f;
        kids[nk] = nd.right(opened);
        firsts[nk] = f + nd.count(nd.left(opened));
        nk++;
    }
    return nk;
}
// The triangles of a leaf of the final tree in depth-first order, the lower position first (at most 7: a leaf reference
// carries its count in 3 bits).  Returns the count, or -1 if the subtree does not fit.
template <class Nodes>
RT_PLOC_HD int leaf_tris(const Nodes &nd, int node, int out[8]) {
    int stack[16], sp = 0, c = 0;
    stack[sp++] = node;
    while (sp > 0) {
        const int x = stack[--sp];
        if (nd.is_tri(x)) {
            if (c >= 8) return -1;
            out[c++] = nd.tri(x);
        } else {
            if (sp + 2 > 16) return -1;
            stack[sp++] = nd.right(x);
            stack[sp++] = nd.left(x);
        }
    }
    return c;
}

}  // namespace rtploc
#endif  // RT_PLOC_H
