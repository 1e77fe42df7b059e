// rt_build_kernels.inc -- the device side of a scene's BVH: the leaf-order arrays, the refit and the PLOC build.  Included by
// rtcuda_amd.hip, once.
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
