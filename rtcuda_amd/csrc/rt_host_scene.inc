// ============================================================================ host side
// The scene side of the host code is one path.  Whoever makes or replaces a tree -- rt_scene_create* with the host or the device
// builder, rt_scene_set_triangles*, rt_scene_rebuild* -- does the same four things: a builder fills a TreeBuild
// (build_sah_host, build_ploc_device), emit_tree allocates the leaf-order arrays for it and writes them (emit_scene),
// adopt_tree waits and hands arrays, tree and host state to the scene.  The table edits (rt_scene_set_materials,
// rt_scene_set_lights) fill the subset they replace and hand it over the same way: rt_scene::adopt is the one place where
// the scene's device arrays change hands, FreshArrays the one owner of what is not adopted yet.
//
// What the kernels read in leaf order, and the tree: a scene's own arrays (rt_scene_update) or new ones that replace them
// once they are complete (FreshArrays).  Written by emit_scene.
struct SceneArrays {
    const int *order;          // leaf order -> caller's triangle index
    const rtbvh::Pair *recs;   // 4-wide: the builder's unpadded records
    int n_records;
    float4 *nodes, *tris, *shade;
    int2 *info;
    Light *lights;
    float *tables;
};
// The arrays for a tree, or the subset an edit replaces, until the scene adopts them (rt_scene::adopt): freed here on every
// early return, and after the adoption what is freed here is what the scene gave back.
struct FreshArrays {
    rtbvh::Pair *recs = nullptr;
    int *order = nullptr;
    float4 *nodes = nullptr, *tris = nullptr, *shade = nullptr;
    int2 *info = nullptr;
    Material *mats = nullptr;
    Light *lights = nullptr;
    float *tables = nullptr;
    FreshArrays() = default;
    FreshArrays(const FreshArrays &) = delete;
    FreshArrays &operator=(const FreshArrays &) = delete;
    ~FreshArrays() {
        for (void *q : {(void *)recs, (void *)order, (void *)nodes, (void *)tris, (void *)shade, (void *)info, (void *)mats, (void *)lights, (void *)tables})
            (void)hipFree(q);
    }
    template <typename T>
    int alloc(T *&ptr, size_t count) {  // (ptr: one of the members)
        HIP_TRY(hipMalloc((void **)&ptr, std::max<size_t>(count, 1) * sizeof(T)));
        return 0;
    }
    SceneArrays view(int n_records) const { return {order, recs, n_records, nodes, tris, shade, info, lights, tables}; }
};

struct rt_scene {
    int device = 0;
    int n_tris = 0, n_nodes = 0, max_depth = 0, stack_bound = 1, n_leaves = 0, n_lights = 0, n_mats = 0;
    float4 *d_nodes = nullptr;
    bool wide = false;  // node records: 4-wide (two pair-style records per node, rtbvh::Result::quads) or 2-wide (rtbvh::Pair)
    // 4-wide: the builder's unpadded records on the device (links fixed by the build, boxes refit by rt_scene_update) and on
    // the host; d_nodes holds them padded for the ray origins that will be traced (rt_bvh.h, pad_quads_for_origins) within
    // origin_radius, which only grows (k_refit_emit reports it in d_radius).  pad_mutex serialises every writer of these.
    rtbvh::Pair *d_recs = nullptr;
    std::vector<rtbvh::Pair> h_quads;
    float *d_radius = nullptr;
    mutable float origin_radius[3] = {0.f, 0.f, 0.f};
    mutable std::mutex pad_mutex;
    double build_seconds = 0.0;  // BVH build time (host wall clock, or device events for PLOC)
    int builder = 0;             // 0 host SAH, 2 device PLOC (RT_SCENE_DEVICE_BVH, rt_scene_rebuild): TreeBuild::builder
    float4 *d_tris = nullptr;
    int2 *d_tri_info = nullptr;
    float4 *d_tri_shade = nullptr;
    Material *d_mats = nullptr;
    Light *d_lights = nullptr;
    float *d_tables = nullptr;    // shading tables (see DScene)
    int tab_dwords = 0;
    int *d_order = nullptr;       // leaf order -> original
    std::vector<int> h_order;     // leaf order -> original
    std::vector<int> h_inverse;   // original -> leaf order
    // RT_FLAG_REFERENCE_WALK: the reference's own tree (rt_ref_tree.h), built and uploaded by the first render that asks
    // for it (ensure_ref_tree) from the caller's triangles kept here
    std::vector<float> h_tri9;
    // rt_render_multi: what a replica of this scene on another device is created from, and the replicas made so far
    // (emit_scene also reads the materials of the triangles and the lights from here)
    std::vector<int32_t> h_tri_material, h_tri_light;
    std::vector<rt_material> h_materials;
    std::vector<rt_light> h_lights;
    mutable std::mutex replica_mutex;
    mutable std::vector<rt_scene *> replicas;  // owned; at most one per device
    mutable std::mutex ref_mutex;
    mutable bool ref_ready = false;
    mutable float4 *d_ref_nodes = nullptr;
    mutable int *d_ref_prims = nullptr;
    mutable int *d_ref_leaf_of = nullptr;  // leaf-order triangle index -> node of its leaf in the reference's tree (ref_visible)
    mutable int *d_ref_parent = nullptr;   // node -> parent node (root: -1)
    mutable int ref_nodes_count = 0, ref_depth = 0;
    mutable bool ref_root_leaf = true;
    mutable double build_seconds_ref = 0.0;  // host time of the reference-tree build + upload (one-off, first render that needs it)
    // rt_scene_update (4-wide only): the tree's nodes grouped by level, deepest level first (refit_level_end[l] = end of level
    // l's span) and the exact box of every node (scratch between the level launches) -- set up by the first update
    std::vector<int> refit_level_end;
    int *d_refit_nodes = nullptr;
    float *d_refit_exact = nullptr;
    int64_t refits = 0;
    double refit_seconds = 0.0;                 // device time of the last refit (HIP events)
    double sah_build = 0.0, sah_now = 0.0;      // surface-area cost of the 4-wide tree at build time / now
    // rt_query_*_device: what a query call needs besides the caller's buffers, made by the first query and reused -- the
    // scratch words on the device and their pinned host copy, the overflow part of the traversal stacks (ensure_overflow),
    // the inverse leaf order on the device (rt_query_any_device; dropped with the leaf order it belongs to: adopt_tree) and
    // the rare-path counters of the last query.  `mutex`: queries of one scene take turns (they share these).
    struct QueryState {
        std::mutex mutex;
        QueryWords *d_words = nullptr, *h_words = nullptr;
        int *d_over = nullptr, over_levels = 0;
        int *d_inverse = nullptr;
        int cus = 0;
        int64_t counters[3] = {0, 0, 0};  // re-traced, lost, tied
        hipEvent_t ev_a = nullptr, ev_b = nullptr;  // rt_render_aov_*: the kernel's bracket (made by the scene's first AOV call)
    };
    mutable QueryState query;
    rt_scene() = default;
    rt_scene(const rt_scene &) = delete;
    rt_scene &operator=(const rt_scene &) = delete;
    ~rt_scene() {  // (every early return of rt_scene_create goes through here: nothing leaks on an error path)
        drop_replicas();
        drop_ref_tree();
        drop_refit();
        drop_query_inverse();
        for (void *q : {(void *)d_nodes, (void *)d_recs, (void *)d_radius, (void *)d_tris, (void *)d_tri_info, (void *)d_tri_shade,
                        (void *)d_mats, (void *)d_lights, (void *)d_order, (void *)d_tables, (void *)query.d_words, (void *)query.d_over})
            (void)hipFree(q);
        if (query.h_words) (void)hipHostFree(query.h_words);
        if (query.ev_a) (void)hipEventDestroy(query.ev_a);
        if (query.ev_b) (void)hipEventDestroy(query.ev_b);
    }
    // the inverse leaf order belongs to one tree: the next rt_query_any_device makes it for the scene's
    void drop_query_inverse() {
        (void)hipFree(query.d_inverse);
        query.d_inverse = nullptr;
    }
    // the reference's tree is a function of the triangles: the next render that needs it builds it again from h_tri9
    void drop_ref_tree() {
        std::lock_guard<std::mutex> lock(ref_mutex);
        for (void *q : {(void *)d_ref_nodes, (void *)d_ref_prims, (void *)d_ref_leaf_of, (void *)d_ref_parent}) (void)hipFree(q);
        d_ref_nodes = nullptr;
        d_ref_prims = d_ref_leaf_of = d_ref_parent = nullptr;
        ref_nodes_count = ref_depth = 0;
        ref_root_leaf = true;
        ref_ready = false;
    }
    // replicas on other devices (rt_render_multi) hold the old geometry or tree: recreated from the host copies on next use
    void drop_replicas() {
        std::lock_guard<std::mutex> lock(replica_mutex);
        for (rt_scene *r : replicas) delete r;
        replicas.clear();
    }
    // the refit's levels belong to one tree: the next rt_scene_update sets them up for the scene's (caller holds pad_mutex)
    void drop_refit() {
        (void)hipFree(d_refit_nodes);
        (void)hipFree(d_refit_exact);
        d_refit_nodes = nullptr;
        d_refit_exact = nullptr;
        refit_level_end.clear();
    }
    // the largest material and light index a triangle names (-1: none), for rt_scene_set_materials / rt_scene_set_lights
    int max_tri_material = -1, max_tri_light = -1;
    void note_index_maxima() {
        max_tri_material = max_tri_light = -1;
        for (int32_t m : h_tri_material) max_tri_material = std::max(max_tri_material, (int)m);
        for (int32_t l : h_tri_light) max_tri_light = std::max(max_tri_light, (int)l);
    }
    void set_order(const std::vector<int32_t> &order) {
        h_order.assign(order.begin(), order.end());
        h_inverse.assign(h_order.size(), 0);
        for (size_t k = 0; k < h_order.size(); k++) h_inverse[(size_t)h_order[k]] = (int)k;
    }
    SceneArrays arrays() const { return {d_order, d_recs, n_nodes, d_nodes, d_tris, d_tri_shade, d_tri_info, d_lights, d_tables}; }
    // The one place where the scene's device arrays change hands: it takes what `f` holds, and `f` releases what it got back.
    // (The caller has waited for the device work that wrote them, holds pad_mutex, and brings the host state along.)
    void adopt(FreshArrays &f) {
        auto take = [](auto *&mine, auto *&fresh) {
            if (fresh) std::swap(mine, fresh);
        };
        take(d_recs, f.recs);
        take(d_order, f.order);
        take(d_nodes, f.nodes);
        take(d_tris, f.tris);
        take(d_tri_shade, f.shade);
        take(d_tri_info, f.info);
        take(d_mats, f.mats);
        take(d_lights, f.lights);
        take(d_tables, f.tables);
    }
    DScene dev() const {
        DScene s;
        s.nodes = d_nodes;
        s.tris = d_tris;
        s.tri_info = d_tri_info;
        s.tri_shade = d_tri_shade;
        s.order = d_order;
        s.mats = d_mats;
        s.lights = d_lights;
        s.num_lights = n_lights;
        s.num_mats = n_mats;
        s.tables = d_tables;
        s.tab_dwords = tab_dwords;
        s.ref_nodes = d_ref_nodes;
        s.ref_prims = d_ref_prims;
        s.ref_n_prims = ref_ready ? n_tris : 0;
        s.ref_leaf_of = d_ref_leaf_of;
        s.ref_parent = d_ref_parent;
        s.ref_root_leaf = ref_root_leaf ? 1 : 0;
        return s;
    }
};

namespace {

// ---- XORWOW host pieces: seed scramble and the 2^67 jump matrices J^(2^k)
Rng xorwow_seed(uint64_t seed) {  // curand_init's scramble (curand_kernel.h; SURVEY Appendix A.6)
    uint32_t s0 = ((uint32_t)seed) ^ 0xaad26b49u;
    uint32_t s1 = ((uint32_t)(seed >> 32)) ^ 0xf7dcefddu;
    uint32_t t0 = 1099087573u * s0;
    uint32_t t1 = 2591861531u * s1;
    Rng st;
    st.d = 6615241u + t1 + t0;
    st.v0 = 123456789u + t0;
    st.v1 = 362436069u ^ t0;
    st.v2 = 521288629u + t1;
    st.v3 = 88675123u ^ t1;
    st.v4 = 5783321u + t0;
    return st;
}
typedef uint32_t Mat160[160][5];
void mat160_apply(const Mat160 &m, const uint32_t in[5], uint32_t out[5]) {
    uint32_t r[5] = {0, 0, 0, 0, 0};
    for (int w = 0; w < 5; w++)
        for (int b = 0; b < 32; b++)
            if (in[w] & (1u << b))
                for (int k = 0; k < 5; k++) r[k] ^= m[w * 32 + b][k];
    memcpy(out, r, sizeof(r));
}
void mat160_square(Mat160 &m) {
    static Mat160 tmp;
    for (int i = 0; i < 160; i++) mat160_apply(m, m[i], tmp[i]);
    memcpy(m, tmp, sizeof(Mat160));
}
// host table: 20 matrices J^(2^k), J = (one xorwow step)^(2^67)
const std::vector<uint32_t> &jump_powers() {
    static std::vector<uint32_t> table;
    static std::once_flag once;
    std::call_once(once, [] {
        static Mat160 a;
        for (int w = 0; w < 5; w++)
            for (int b = 0; b < 32; b++) {
                uint32_t v[5] = {0, 0, 0, 0, 0};
                v[w] = 1u << b;
                uint32_t t = v[0] ^ (v[0] >> 2);
                v[0] = v[1];
                v[1] = v[2];
                v[2] = v[3];
                v[3] = v[4];
                v[4] = (v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1));
                memcpy(a[w * 32 + b], v, sizeof(v));
            }
        for (int s = 0; s < 67; s++) mat160_square(a);
        table.resize((size_t)20 * 160 * 5);
        for (int k = 0; k < 20; k++) {
            memcpy(table.data() + (size_t)k * 800, a, sizeof(Mat160));
            mat160_square(a);
        }
    });
    return table;
}

// 2-wide nodes (RT_BVH_WIDE=0, or a host tree too deep for the 4-wide walk's stack): a 64-byte record with the two children's
// bounds INTERLEAVED --
//   (l.lo.x, r.lo.x, l.lo.y, r.lo.y | l.lo.z, r.lo.z, l.hi.x, r.hi.x | l.hi.y, r.hi.y, l.hi.z, r.hi.z | llink, rlink, spare, spare)
// -- so that every (left, right) pair of bounds arrives in an aligned register pair and the slab arithmetic of both children
// runs as packed fp32, see inner_step.  (The 4-wide layout is k_refit_emit's.)
int upload_pairs(const std::vector<rtbvh::Pair> &pairs, float4 *d_nodes) {
    std::vector<float> inter(16 * pairs.size());
    for (size_t k = 0; k < pairs.size(); k++) {
        const rtbvh::Pair &pr = pairs[k];
        float *r = &inter[16 * k];
        for (int a = 0; a < 6; a++) {
            r[2 * a] = pr.lbox[a];
            r[2 * a + 1] = pr.rbox[a];
        }
        memcpy(&r[12], &pr.llink, 4);
        memcpy(&r[13], &pr.rlink, 4);
        r[14] = r[15] = 0.f;
    }
    HIP_TRY(hipMemcpy(d_nodes, inter.data(), 64 * pairs.size(), hipMemcpyHostToDevice));
    return 0;
}

// Structural check of 4-wide records before they are uploaded (a malformed tree would hang the GPU): every node reachable
// from the root exactly once (two consecutive records per node; inner links are even record indices), every triangle
// position in exactly one leaf, plus the invariant the kernels' box test rests on: a child is absent (link kNoChild) if and
// only if its box is all +inf -- the one-comparison slab test of inner_step<true> never looks at links.
bool validate_quads(const std::vector<rtbvh::Pair> &quads, int n_tris) {
    const int nr = (int)quads.size();
    if (nr < 2 || (nr & 1)) return false;
    std::vector<char> seen_node((size_t)nr / 2, 0), seen_tri((size_t)std::max(n_tris, 1), 0);
    std::vector<int> todo{0};
    seen_node[0] = 1;
    int visited = 0, tris = 0;
    while (!todo.empty()) {
        const int rec = todo.back();
        todo.pop_back();
        visited++;
        for (int k = 0; k < 4; k++) {
            const rtbvh::Pair &p = quads[(size_t)rec + (k >> 1)];
            const int l = (k & 1) ? p.rlink : p.llink;
            const float *b = (k & 1) ? p.rbox : p.lbox;
            bool all_inf = true, finite = true;
            for (int a = 0; a < 6; a++) {
                all_inf = all_inf && b[a] == INFINITY;
                finite = finite && std::isfinite(b[a]);
            }
            if (l == rtbvh::kNoChild) {
                if (!all_inf) return false;
                continue;
            }
            if (!finite || b[0] > b[3] || b[1] > b[4] || b[2] > b[5]) return false;
            if (l >= 0) {
                if ((l & 1) || l >= nr || seen_node[l / 2]) return false;
                seen_node[l / 2] = 1;
                todo.push_back(l);
            } else {
                const int ref = ~l, first = ref >> 3, count = ref & 7;
                if (count <= 0 || first < 0 || first + count > n_tris) return false;
                for (int t = first; t < first + count; t++) {
                    if (seen_tri[t]) return false;
                    seen_tri[t] = 1;
                    tris++;
                }
            }
        }
    }
    return visited == nr / 2 && tris == n_tris;
}

// RT_FLAG_REFERENCE_WALK: build the reference's tree from the caller's triangles, check its structure (a malformed tree
// would hang the walk: every node reached exactly once, children adjacent, every primitive position in exactly one
// leaf, depth within the walk's private stack) and upload it.  Once per scene, on the scene's device.
// `built` (may be null): whether THIS call built the tree, decided under the lock (two first renders may race to it).
int ensure_ref_tree(const rt_scene *scene, bool *built = nullptr) {
    std::lock_guard<std::mutex> lock(scene->ref_mutex);
    if (built) *built = false;
    if (scene->ref_ready) return 0;
    const auto t_begin = std::chrono::steady_clock::now();
    const int n = scene->n_tris;
    if ((int)scene->h_tri9.size() != 9 * n) return fail("RT_FLAG_REFERENCE_WALK: the scene holds no triangle copy");
    const rtref::Tree t = rtref::build(scene->h_tri9.data(), n);
    const int nn = (int)t.nodes.size();
    if (n > 0) {
        std::vector<char> seen_node((size_t)nn, 0), seen_prim((size_t)n, 0);
        std::vector<std::pair<int, int>> todo{{0, 0}};  // (node, depth)
        int visited = 0, prims = 0;
        seen_node[0] = 1;
        while (!todo.empty()) {
            const auto [k, dep] = todo.back();
            todo.pop_back();
            visited++;
            const rtref::Node &nd = t.nodes[(size_t)k];
            if (nd.count > 0) {
                if (nd.link < 0 || nd.link + nd.count > n) return fail("RT_FLAG_REFERENCE_WALK: malformed leaf");
                for (int i = nd.link; i < nd.link + nd.count; i++) {
                    if (seen_prim[i]) return fail("RT_FLAG_REFERENCE_WALK: primitive in two leaves");
                    seen_prim[i] = 1;
                    prims++;
                }
            } else {
                if (nd.count < 0 || nd.link <= 0 || nd.link + 1 >= nn || seen_node[nd.link] || seen_node[nd.link + 1] || dep >= rtref::kMaxDepth)
                    return fail("RT_FLAG_REFERENCE_WALK: malformed inner node");
                seen_node[nd.link] = seen_node[nd.link + 1] = 1;
                todo.push_back({nd.link, dep + 1});
                todo.push_back({nd.link + 1, dep + 1});
            }
        }
        if (visited != nn || prims != n) return fail("RT_FLAG_REFERENCE_WALK: tree does not cover the scene");
        for (int i = 0; i < n; i++)
            if (t.prims[i] < 0 || t.prims[i] >= n) return fail("RT_FLAG_REFERENCE_WALK: bad primitive order");
    }
    std::vector<int> prim_leaf((size_t)std::max(n, 1), 0);  // reference primitive position -> this scene's leaf-order index
    for (int i = 0; i < n; i++) prim_leaf[i] = scene->h_inverse[t.prims[i]];
    // what ref_visible reads: the leaf of every triangle (leaf-order index -> node) and the way up from there
    std::vector<int> leaf_of((size_t)std::max(n, 1), 0), parent((size_t)std::max(nn, 1), -1);
    for (int k = 0; k < nn; k++) {
        const rtref::Node &nd = t.nodes[(size_t)k];
        if (nd.count > 0) {
            for (int i = nd.link; i < nd.link + nd.count; i++) leaf_of[(size_t)prim_leaf[(size_t)i]] = k;
        } else if (n > 0) {
            parent[(size_t)nd.link] = parent[(size_t)nd.link + 1] = k;
        }
    }
    float4 *dn = nullptr;
    int *dp = nullptr, *dl = nullptr, *dpar = nullptr;
    if (hipMalloc((void **)&dn, sizeof(rtref::Node) * (size_t)std::max(nn, 1)) != hipSuccess ||
        hipMalloc((void **)&dp, sizeof(int) * prim_leaf.size()) != hipSuccess ||
        hipMalloc((void **)&dl, sizeof(int) * leaf_of.size()) != hipSuccess ||
        hipMalloc((void **)&dpar, sizeof(int) * parent.size()) != hipSuccess ||
        hipMemcpy(dn, t.nodes.data(), sizeof(rtref::Node) * (size_t)nn, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dp, prim_leaf.data(), sizeof(int) * prim_leaf.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dl, leaf_of.data(), sizeof(int) * leaf_of.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dpar, parent.data(), sizeof(int) * parent.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(dn);
        (void)hipFree(dp);
        (void)hipFree(dl);
        (void)hipFree(dpar);
        return fail("reference tree: device allocation or upload failed");
    }
    scene->d_ref_nodes = dn;
    scene->d_ref_prims = dp;
    scene->d_ref_leaf_of = dl;
    scene->d_ref_parent = dpar;
    scene->ref_root_leaf = n == 0 || t.nodes[0].count > 0;
    scene->ref_nodes_count = nn;
    scene->ref_depth = t.depth;
    scene->build_seconds_ref = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    scene->ref_ready = true;
    if (built) *built = true;
    return 0;
}

// The argument checks of rt_scene_create, shared with the entry points that edit a scene (`w`: whose message it is):
// the counts and the table pointers ...
int check_scene_counts(const std::string &w, int n_tris, bool have_tri_arrays, const rt_material *materials, int n_materials,
                       const rt_light *lights, int n_lights) {
    if (n_tris < 0 || n_materials < 0 || n_lights < 0) return fail(w + ": negative count");
    if (n_tris >= (1 << 24)) return fail(w + ": more than 2^24 - 1 triangles (24-bit triangle addressing)");
    if (n_tris > 0 && !have_tri_arrays) return fail(w + ": null triangle arrays");
    if (n_tris > 0 && (n_materials == 0 || !materials)) return fail(w + ": no materials");
    if (n_lights > 0 && !lights) return fail(w + ": null lights");
    if (n_materials > 65535 || n_lights > 32766) return fail(w + ": at most 65535 materials and 32766 lights");
    return 0;
}
// ... the index ranges of the per-triangle HOST arrays (tri_light may be null; device arrays: k_index_prepass) ...
int check_tri_indices(const std::string &w, int n_tris, const int32_t *tri_material, const int32_t *tri_light, int n_materials, int n_lights) {
    for (int i = 0; i < n_tris; i++) {
        if (tri_material && (tri_material[i] < 0 || tri_material[i] >= n_materials))
            return fail(w + ": tri_material[" + std::to_string(i) + "] out of range");
        if (tri_light && (tri_light[i] < -1 || tri_light[i] >= n_lights))
            return fail(w + ": tri_light[" + std::to_string(i) + "] out of range");
    }
    return 0;
}
// ... and the tables themselves
int check_scene_tables(const std::string &w, int n_tris, const rt_material *materials, int n_materials, const rt_light *lights, int n_lights) {
    for (int i = 0; i < n_materials; i++)
        if (materials[i].type < RT_MATTE || materials[i].type > RT_GLASS)
            return fail(w + ": unknown material type");
    for (int i = 0; i < n_lights; i++) {
        if (lights[i].type != RT_POINT_LIGHT && lights[i].type != RT_AREA_LIGHT)
            return fail(w + ": unknown light type");
        if (lights[i].type == RT_AREA_LIGHT && (lights[i].triangle < 0 || lights[i].triangle >= n_tris))
            return fail(w + ": area light triangle out of range");
    }
    return 0;
}

// Device temporaries and events of one host call: released on EVERY return path (HIP_TRY returns early on errors)
struct DevScope {
    std::vector<void *> ptrs;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~DevScope() {
        for (void *q : ptrs) (void)hipFree(q);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    template <typename T>
    int alloc(T *&ptr, size_t count) {
        void *raw = nullptr;
        HIP_TRY(hipMalloc(&raw, std::max<size_t>(count, 1) * sizeof(T)));
        ptrs.push_back(raw);
        ptr = (T *)raw;
        return 0;
    }
};
// A host array into a temporary device buffer, ordered on `st`.  (The copy may still be reading `host` on return: a caller
// whose `host` is not its own waits for `st` before it returns.)
template <typename T>
int stage(DevScope &tmp, const T *host, size_t count, hipStream_t st, const T *&d_out) {
    T *d = nullptr;
    if (tmp.alloc(d, count)) return 1;
    HIP_TRY(hipMemcpyAsync(d, host, sizeof(T) * count, hipMemcpyHostToDevice, st));
    d_out = d;
    return 0;
}
// Is `p` device memory on `device`?  A host pointer is an error, not a fault.
bool on_device(const void *p, int device) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess || (attr.type != hipMemoryTypeDevice && !attr.isManaged) || attr.device != device) {
        (void)hipGetLastError();  // (the failed query leaves its error behind)
        return false;
    }
    return true;
}
// The scene's device made current for the rest of a host call; the caller's is restored on every return path
struct DeviceGuard {
    int saved = 0, current = 0;
    int enter(int device) {
        HIP_TRY(hipGetDevice(&saved));
        current = saved;
        if (device != saved) HIP_TRY(hipSetDevice(device));
        current = device;
        return 0;
    }
    int select(int device) {  // (after enter: a call that works on several devices in turn, rt_render_multi)
        HIP_TRY(hipSetDevice(device));
        current = device;
        return 0;
    }
    ~DeviceGuard() {
        if (current != saved) (void)hipSetDevice(saved);
    }
};

// The 4-wide nodes the kernels walk, from the builder's unpadded records: padded for ray origins within `radius`, grown to
// the records' bounds (k_refit_emit, which leaves the radius it used in sc->d_radius).  Ordered on `st`; the caller holds
// pad_mutex and has made the scene's device current.
void emit_nodes(const rt_scene *sc, const rtbvh::Pair *d_recs, int n_records, float4 *d_nodes, const float radius[3], hipStream_t st) {
    const int n = n_records / 2;
    hipLaunchKernelGGL(k_refit_emit, dim3((n + 255) / 256), dim3(256), 0, st, d_recs, n, radius[0], radius[1], radius[2],
                       (float *)d_nodes, sc->d_radius);
}

// Before rays are traced whose origins may lie outside the radius the 4-wide records are padded for (a camera outside the
// scene's bounds; the rays of the test hooks): re-pad, generously, on the null stream, and wait for it.  Renders of the same
// scene that are in flight on other streams read a mix of the old and the new bounds meanwhile -- both are conservative for
// THEIR rays.
int ensure_origin_radius(const rt_scene *sc, const float need[3]) {
    if (!sc->wide) return 0;
    std::lock_guard<std::mutex> lock(sc->pad_mutex);
    bool grow = false;
    float radius[3];
    for (int a = 0; a < 3; a++) {
        const float want = std::isfinite(need[a]) ? std::fabs(need[a]) * 1.001f : 0.f;  // (a non-finite origin hits nothing anyway)
        grow = grow || want > sc->origin_radius[a];
        radius[a] = want > sc->origin_radius[a] ? 2.f * want : sc->origin_radius[a];
    }
    if (!grow) return 0;
    DeviceGuard dev;
    if (dev.enter(sc->device)) return 1;
    emit_nodes(sc, sc->d_recs, sc->n_nodes, sc->d_nodes, radius, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(sc->origin_radius, sc->d_radius, sizeof(float) * 3, hipMemcpyDeviceToHost));
    return 0;
}

// ---- what the entry points that take rays share (frames, queries, trace hooks, ray tables, AOVs): each written once
// The definition of a hit.  `literal` (RT_FLAG_REFERENCE_WALK): every ray through the reference's own tree.  `verify`, the
// default: the reference's decisions on the product's own walk.  Neither (RT_FLAG_WATERTIGHT; per-sample): the triangle list's.
struct HitMode {
    bool literal, verify;
    bool ref_tree() const { return literal || verify; }  // (ensure_ref_tree)
};
HitMode hit_mode(uint32_t flags, bool per_sample = false) {
    const bool literal = (flags & RT_FLAG_REFERENCE_WALK) != 0;
    return {literal, !literal && !per_sample && (flags & RT_FLAG_WATERTIGHT) == 0};
}
int refuse_both_hit_flags(const std::string &w, uint32_t flags) {
    if ((flags & RT_FLAG_REFERENCE_WALK) && (flags & RT_FLAG_WATERTIGHT)) return fail(w + ": RT_FLAG_REFERENCE_WALK and RT_FLAG_WATERTIGHT exclude each other");
    return 0;
}

// The scene's query scratch, made by the first call that needs it.  (Here and in validate_table: under scene->query.mutex.)
int ensure_query_state(const rt_scene *scene, bool with_events) {
    rt_scene::QueryState &q = scene->query;
    if (!q.d_words) {
        HIP_TRY(hipDeviceGetAttribute(&q.cus, hipDeviceAttributeMultiprocessorCount, scene->device));
        HIP_TRY(hipHostMalloc((void **)&q.h_words, sizeof(QueryWords), hipHostMallocDefault));
        HIP_TRY(hipMalloc((void **)&q.d_words, sizeof(QueryWords)));
    }
    if (with_events && !q.ev_a) HIP_TRY(hipEventCreate(&q.ev_a));
    if (with_events && !q.ev_b) HIP_TRY(hipEventCreate(&q.ev_b));
    return 0;
}

// A table's validation on the device, ordered on `st`, under the entry point's name `w`: the scratch words zeroed, the
// prepasses (directions and origin radius; pixel indices if any), one wait, the 4-wide records padded.  Writes nothing else.
int validate_table(const rt_scene *scene, const std::string &w, int n, const float *d_o, const float *d_d, const int32_t *d_pixel,
                   int n_pixels, hipStream_t st) {
    rt_scene::QueryState &q = scene->query;
    const dim3 grid(std::min((n + kBlock - 1) / kBlock, 8 * std::max(q.cus, 1)));
    HIP_TRY(hipMemsetAsync(q.d_words, 0, sizeof(QueryWords), st));
    hipLaunchKernelGGL(k_query_prepass, grid, dim3(kBlock), 0, st, d_o, d_d, n, q.d_words);
    if (d_pixel) hipLaunchKernelGGL(k_pixel_prepass, grid, dim3(kBlock), 0, st, d_pixel, n, n_pixels, q.d_words);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(q.h_words, q.d_words, 6 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (q.h_words->bad_dirs != 0)
        return fail(w + ": " + std::to_string(q.h_words->bad_dirs) + " of " + std::to_string(n) + " directions are not finite or reach 2^126");
    if (q.h_words->short_dirs != 0)
        return fail(w + ": " + std::to_string(q.h_words->short_dirs) + " of " + std::to_string(n) + " directions are shorter than 2^-60 in every component");
    if (q.h_words->bad_pixels != 0)
        return fail(w + ": " + std::to_string(q.h_words->bad_pixels) + " of " + std::to_string(n) + " pixel indices are outside 0 .. " + std::to_string(n_pixels - 1));
    float need[3];
    memcpy(need, q.h_words->radius_bits, sizeof(need));
    return ensure_origin_radius(scene, need);
}

// The host-side checks of a table (the entry points' flag checks come between the two); wordings that differ are passed in.
int check_table_pointers(const std::string &w, const rt_scene *scene, const float *d_o, const float *d_d, const void *d_out, const char *out_name) {
    if (!scene) return fail(w + ": null scene");
    if (!d_o || !d_d || !d_out) return fail(w + ": null " + (!d_o ? "d_origin_xyz" : !d_d ? "d_dir_xyz" : out_name));
    return 0;
}
int check_table_args(const std::string &w, int64_t n_rays, const char *ray_range, int n_pixels, const int *max_bounces) {
    if (n_rays < 1) return fail(w + ": n_rays = " + std::to_string((long long)n_rays) + " (at least 1)");
    if (n_rays + 13LL * kW >= (1LL << 31)) return fail(w + ": n_rays exceeds " + ray_range);
    if (n_pixels < 1 || n_pixels > 0x7fffffff / 3) return fail(w + ": n_pixels = " + std::to_string(n_pixels) + " is outside 1 .. 715827882");
    if (max_bounces && (*max_bounces < 0 || *max_bounces > (1 << 24))) return fail(w + ": max_bounces is outside 0 .. 16777216");
    return 0;
}
// The keys key_first + c * key_stride and the last one's pixel, then the table as the kernels take it.  `noun`: "key", or
// "ray" for a plain table, whose row c has the key c.
int check_key_range(const std::string &w, const char *noun, int64_t n_rays, uint64_t key_first, uint32_t key_stride, const float *d_o,
                    const float *d_d, const int32_t *d_pixel, int rays_per_pixel, int n_pixels, KeyedRayTable *table) {
    if (key_stride < 1) return fail(w + ": key_stride = 0 (at least 1)");
    // the last key, key_first + (n_rays - 1) * key_stride: the product is below 2^63, the sum must not wrap 2^64
    const unsigned long long span = (unsigned long long)(n_rays - 1) * key_stride;
    if (span > ~0ull - (unsigned long long)key_first)
        return fail(w + ": the key of the last ray, " + std::to_string((unsigned long long)key_first) + " + " + std::to_string(span) + ", wraps 2^64");
    const unsigned long long key_last = (unsigned long long)key_first + span;
    if (!d_pixel) {
        if (rays_per_pixel < 1) return fail(w + ": rays_per_pixel = " + std::to_string(rays_per_pixel) + " (at least 1 when d_pixel is null)");
        if (key_last / (unsigned)rays_per_pixel >= (unsigned long long)n_pixels)
            return fail(w + ": " + noun + " " + std::to_string(key_last) + " falls on pixel " + std::to_string(key_last / (unsigned)rays_per_pixel) + " of " +
                        std::to_string(n_pixels));
    }
    const uint32_t rpp = d_pixel ? 1u : (uint32_t)rays_per_pixel;
    *table = KeyedRayTable{d_o, d_d, d_pixel, (unsigned long long)key_first, key_stride, rpp,
                           d_pixel ? 0 : (int)(key_first / rpp), d_pixel ? 0u : (uint32_t)(key_first % rpp)};
    return 0;
}

// The rare-path counters of a call (rt_stats::reserved[4..6], rt_query_last_counters): re-traced, lost, tied
void rare_path_counters(const unsigned long long *vstat, int64_t out[3]) {
    out[0] = (int64_t)vstat[V_LITERAL];
    out[1] = (int64_t)vstat[V_LOST];
    out[2] = (int64_t)vstat[V_TIE];
}

// What emit_scene reads besides the vertices: the counts, the material table on the device (null: none there yet, emit_tree
// uploads h_mats), the lights on the host and -- for a new leaf order -- the caller's per-triangle indices on the device, in
// the caller's order (tri_light null: -1 everywhere).  The scene's own (scene_source: rt_scene_create, rt_scene_update,
// rt_scene_rebuild) or those it is about to adopt (rt_scene_set_triangles).
struct EmitSource {
    int n_tris = 0, n_mats = 0, n_lights = 0;
    const Material *d_mats = nullptr;
    const rt_material *h_mats = nullptr;
    const rt_light *h_lights = nullptr;
    const int *d_tri_material = nullptr, *d_tri_light = nullptr;
    const float *radius = nullptr;  // the origin radius the 4-wide nodes are padded for at least (3 floats)
};

// The shading tables of `n_mats` materials and `n_lights` lights (k_build_tables), ordered on `st`
void launch_build_tables(const Material *d_mats, int n_mats, const Light *d_lights, int n_lights, const float4 *d_tris, float *d_tables,
                         hipStream_t st) {
    const int nt = std::max(std::max(n_mats, n_lights), 1);
    hipLaunchKernelGGL(k_build_tables, dim3((nt + 63) / 64), dim3(64), 0, st, d_mats, n_mats, d_lights, n_lights, d_tris, d_tables);
}

// The one writer of the scene's leaf-order arrays, ordered on `st`, from the caller's vertices on the device (d_verts) and
// the leaf order out.order: the triangle records (k_leaf_tris), the shading records and tables, and -- 4-wide -- the nodes
// from out.recs, padded for src.radius (emit_nodes).  For a new leaf order `d_inverse` (n ints of scratch) receives its
// inverse, and the triangles' (material, light), from the two device arrays of `src`, and the lights, their triangles
// renumbered, are written too.  Null for a refit: the leaf order is the scene's, and so are tri_info and the lights; the boxes of
// the scene's records are refit to the vertices before they are padded (k_refit_level, one launch per level, deepest first;
// launched after k_leaf_tris, which reads the same vertices: 5 us less per refit of the bunny than before it).
int emit_scene(const rt_scene *sc, const EmitSource &src, const float *d_verts, const SceneArrays &out, int *d_inverse, hipStream_t st) {
    const int n = src.n_tris, n_lights = src.n_lights;
    const dim3 blk(256), grid((n + 255) / 256);
    if (d_inverse && n > 0) {
        hipLaunchKernelGGL(k_leaf_inverse, grid, blk, 0, st, out.order, n, d_inverse);
        hipLaunchKernelGGL(k_leaf_tri_info, grid, blk, 0, st, src.d_tri_material, src.d_tri_light, out.order, n, out.info);
    }
    if (d_inverse && n_lights > 0) {
        HIP_TRY(hipMemcpyAsync(out.lights, src.h_lights, sizeof(Light) * (size_t)n_lights, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_leaf_lights, dim3((n_lights + 255) / 256), blk, 0, st, out.lights, n_lights, d_inverse);
    }
    if (n > 0) {
        hipLaunchKernelGGL(k_leaf_tris, grid, blk, 0, st, d_verts, out.order, n, out.tris);
        hipLaunchKernelGGL(k_build_tri_shade, grid, blk, 0, st, out.tris, out.info, n, out.shade);
    }
    launch_build_tables(src.d_mats, src.n_mats, out.lights, n_lights, out.tris, out.tables, st);
    if (!d_inverse)
        for (size_t l = 0; l < sc->refit_level_end.size(); l++) {
            const int begin = l ? sc->refit_level_end[l - 1] : 0, count = sc->refit_level_end[l] - begin;
            hipLaunchKernelGGL(k_refit_level, dim3((count + 255) / 256), blk, 0, st, d_verts, sc->d_order, sc->d_refit_nodes + begin,
                               count, sc->d_recs, sc->d_refit_exact);
        }
    if (sc->wide) emit_nodes(sc, out.recs, out.n_records, out.nodes, src.radius, st);
    HIP_TRY(hipGetLastError());
    return 0;
}
// The scene's own source.  For a new leaf order (`with_indices`) its per-triangle indices go to the device first, staged on
// `st` into `tmp` from the host copies: every caller of emit_scene hands it device arrays, there is one emit path.
int scene_source(const rt_scene *sc, bool with_indices, hipStream_t st, DevScope &tmp, EmitSource &src) {
    src = EmitSource{sc->n_tris, sc->n_mats, sc->n_lights, sc->d_mats, sc->h_materials.data(), sc->h_lights.data(), nullptr, nullptr,
                     sc->origin_radius};
    if (!with_indices || sc->n_tris < 1) return 0;
    const size_t n = (size_t)sc->n_tris;
    if (stage(tmp, sc->h_tri_material.data(), n, st, src.d_tri_material)) return 1;
    return sc->h_tri_light.empty() ? 0 : stage(tmp, sc->h_tri_light.data(), n, st, src.d_tri_light);
}

// The start of rt_scene_update and rt_scene_rebuild: a device buffer of the caller's checked (on the scene's device), the
// scene's device made current (until `dev` goes), and the vertices on it in d_verts -- the caller's buffer, or the host
// array (null: the scene's own copy) staged on `st` into `tmp`.
int stage_vertices(const rt_scene *sc, const float *verts, bool device_ptr, hipStream_t st, const std::string &w, DeviceGuard &dev,
                   DevScope &tmp, const float *&d_verts) {
    if (device_ptr && verts && !on_device(verts, sc->device))
        return fail(w + ": d_tri_p0p1p2 is not device memory on the scene's device " + std::to_string(sc->device));
    if (dev.enter(sc->device)) return 1;
    d_verts = verts;
    if (sc->n_tris > 0 && (!verts || !device_ptr)) return stage(tmp, verts ? verts : sc->h_tri9.data(), 9 * (size_t)sc->n_tris, st, d_verts);
    return 0;
}

// Surface-area cost of the 4-wide tree (the form of rtbvh::sah_cost): child box areas weighted by the triangles of a leaf
// child or one node step, relative to the area of the root's bounds.  Advisory (rt_scene_refit_info).
double quads_sah(const std::vector<rtbvh::Pair> &quads) {
    auto half_area = [](const float *b) {
        const double e0 = (double)b[3] - b[0], e1 = (double)b[4] - b[1], e2 = (double)b[5] - b[2];
        return (e0 + e1) * e2 + e0 * e1;
    };
    double cost = 0.0, root[6] = {DBL_MAX, DBL_MAX, DBL_MAX, -DBL_MAX, -DBL_MAX, -DBL_MAX};
    for (size_t r = 0; r < quads.size(); r++)
        for (int side = 0; side < 2; side++) {
            const int32_t l = side ? quads[r].rlink : quads[r].llink;
            if (l == rtbvh::kNoChild) continue;
            const float *b = side ? quads[r].rbox : quads[r].lbox;
            cost += half_area(b) * (l < 0 ? (double)((~l) & 7) : 1.0);
            if (r < 2)
                for (int a = 0; a < 3; a++) {
                    root[a] = std::min(root[a], (double)b[a]);
                    root[3 + a] = std::max(root[3 + a], (double)b[3 + a]);
                }
        }
    const double e0 = root[3] - root[0], e1 = root[4] - root[1], e2 = root[5] - root[2];
    return quads.size() < 2 || !(e0 >= 0.0) ? 0.0 : cost / std::max((e0 + e1) * e2 + e0 * e1, 1e-30);
}

// rt_scene_update / rt_scene_update_device: refit the 4-wide tree on the scene's device (emit_scene), then
// bring the host state along -- the builder records, the radius they are padded for, the triangle copy the reference's tree
// and the replicas are made from.  `verts` is a host array or (device_ptr) a buffer on the scene's device.
int scene_update_impl(rt_scene *sc, const float *verts, int n_tris, bool device_ptr, hipStream_t st, const char *what) {
    const std::string w(what);
    if (!sc || !verts) return fail(w + ": null argument");
    if (n_tris != sc->n_tris) return fail(w + ": " + std::to_string(n_tris) + " triangles, the scene was created with " + std::to_string(sc->n_tris));
    if (!sc->wide) return fail(w + ": the scene uses the 2-wide experiment format (RT_BVH_WIDE=0), which cannot be refit");
    std::lock_guard<std::mutex> pad_lock(sc->pad_mutex);  // (the records, h_quads and origin_radius change)
    DeviceGuard dev;
    DevScope tmp;
    const float *d_verts = nullptr;
    if (stage_vertices(sc, verts, device_ptr, st, w, dev, tmp, d_verts)) return 1;
    const int n = n_tris;
    const int n_nodes = sc->n_nodes / 2;  // 4-wide nodes: two records each
    if (n > 0 && !sc->d_refit_nodes) {
        // the levels of the tree, fixed at creation: breadth-first from the root, then deepest level first
        std::vector<int> depth((size_t)n_nodes, -1), queue{0};
        depth[0] = 0;
        for (size_t h = 0; h < queue.size(); h++)
            for (int k = 0; k < 4; k++) {
                const rtbvh::Pair &p = sc->h_quads[2 * (size_t)queue[h] + (k >> 1)];
                const int32_t l = (k & 1) ? p.rlink : p.llink;
                if (l >= 0) {
                    depth[(size_t)l / 2] = depth[(size_t)queue[h]] + 1;
                    queue.push_back(l / 2);
                }
            }
        if ((int)queue.size() != n_nodes) return fail(w + ": the tree does not reach every node");
        const int levels = depth[(size_t)queue.back()] + 1;
        std::vector<int> nodes;
        nodes.reserve((size_t)n_nodes);
        std::vector<int> level_end;
        for (int d = levels - 1; d >= 0; d--) {
            for (int j : queue)
                if (depth[(size_t)j] == d) nodes.push_back(j);
            level_end.push_back((int)nodes.size());
        }
        int *dn = nullptr;
        float *de = nullptr;
        if (hipMalloc((void **)&dn, sizeof(int) * nodes.size()) != hipSuccess ||
            hipMalloc((void **)&de, sizeof(float) * 6 * (size_t)n_nodes) != hipSuccess ||
            hipMemcpy(dn, nodes.data(), sizeof(int) * nodes.size(), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(dn);
            (void)hipFree(de);
            return fail(w + ": device allocation or upload failed");
        }
        sc->d_refit_nodes = dn;
        sc->d_refit_exact = de;
        sc->refit_level_end = level_end;
        sc->sah_build = sc->sah_now = quads_sah(sc->h_quads);
    }
    double seconds = 0.0;
    if (n > 0) {
        HIP_TRY(hipEventCreate(&tmp.e0));
        HIP_TRY(hipEventCreate(&tmp.e1));
        HIP_TRY(hipEventRecord(tmp.e0, st));
        EmitSource src;
        if (scene_source(sc, false, st, tmp, src)) return 1;
        if (emit_scene(sc, src, d_verts, sc->arrays(), nullptr, st)) return 1;
        HIP_TRY(hipEventRecord(tmp.e1, st));
        HIP_TRY(hipEventSynchronize(tmp.e1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, tmp.e0, tmp.e1));
        seconds = ms * 1e-3;
        // the host's view of the new geometry: the unpadded records, the radius the device copy is padded for, the caller's
        // triangles (the reference's tree and the replicas are made from them)
        HIP_TRY(hipMemcpy(sc->h_quads.data(), sc->d_recs, sizeof(rtbvh::Pair) * sc->h_quads.size(), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(sc->origin_radius, sc->d_radius, sizeof(float) * 3, hipMemcpyDeviceToHost));
        if (device_ptr) HIP_TRY(hipMemcpy(sc->h_tri9.data(), verts, sizeof(float) * 9 * (size_t)n, hipMemcpyDeviceToHost));
        else memcpy(sc->h_tri9.data(), verts, sizeof(float) * 9 * (size_t)n);
        sc->sah_now = quads_sah(sc->h_quads);
    }
    sc->refit_seconds = seconds;
    sc->refits++;
    sc->drop_ref_tree();
    sc->drop_replicas();
    return 0;
}

// A built tree, whichever builder made it: the unpadded 4-wide records and the leaf order, on the device (a.recs, a.order)
// and on the host -- or, from the host builder only, the 2-wide records of the experiment format on the host (`pairs`: no
// a.recs then; emit_tree uploads them as the nodes).  `a` also receives the leaf-order arrays emitted for the tree (emit_tree)
// and owns all of them until the scene takes them (adopt_tree).
struct TreeBuild {
    FreshArrays a;
    std::vector<rtbvh::Pair> quads, pairs;
    std::vector<int32_t> order;
    int max_depth = 0, stack_bound = 1, leaves = 0, iterations = 0;
    int builder = 2;       // rt_scene::builder
    double seconds = 0.0;  // device time of the build (HIP events), or the host's wall clock
    bool wide() const { return pairs.empty(); }
    int n_records() const { return (int)(wide() ? quads.size() : pairs.size()); }  // 64-byte records
};

// The host SAH builder (rtbvh::build) of n >= 0 triangles, checked and uploaded to the current device.  `wide`: 4-wide
// wanted; a tree too deep for the 4-wide walk's stack comes out 2-wide.  `for_device`: what RT_SCENE_DEVICE_BVH gets for a scene
// of no triangles, where there is nothing to build -- reported as the device builder's, in 0 seconds.
int build_sah_host(const float *verts, int n, bool wide, bool for_device, TreeBuild &out) {
    const auto t0 = std::chrono::steady_clock::now();
    rtbvh::Result bvh = rtbvh::build(verts, n);
    out.seconds = for_device ? 0.0 : std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    out.builder = for_device ? 2 : 0;
    if (!bvh.ok) return fail("rt_scene_create: BVH build produced an unreferenceable leaf");
    if (n > 0 && !bvh.quads.empty() && !validate_quads(bvh.quads, n))
        return fail("rt_scene_create: the 4-wide BVH is malformed (structure, or an absent child without its +inf box)");
    // a tree too deep for the 4-wide walk's stack (up to 3 entries per level) may still fit the 2-wide walk's (1 per level):
    // a host tree the reinsertion pass deepened
    if (wide && bvh.stack_bound > kMaxStackBound) wide = false;
    if ((wide ? bvh.stack_bound : bvh.pair_depth + 1) > kMaxStackBound)
        return fail("rt_scene_create: BVH depth " + std::to_string(wide ? bvh.max_depth : bvh.pair_depth) + " exceeds the traversal stack");
    out.max_depth = wide ? bvh.max_depth : bvh.pair_depth;
    out.stack_bound = wide ? bvh.stack_bound : bvh.pair_depth + 1;
    out.leaves = bvh.num_leaves;
    out.order = std::move(bvh.order);
    if (out.a.alloc(out.a.order, (size_t)n)) return 1;
    if (n) HIP_TRY(hipMemcpy(out.a.order, out.order.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    if (!wide) {
        out.pairs = std::move(bvh.pairs);
        return 0;
    }
    out.quads = std::move(bvh.quads);
    if (out.a.alloc(out.a.recs, out.quads.size())) return 1;
    HIP_TRY(hipMemcpy(out.a.recs, out.quads.data(), sizeof(rtbvh::Pair) * out.quads.size(), hipMemcpyHostToDevice));
    return 0;
}

// Device PLOC build (k_ploc_*) of n >= 1 triangles from d_verts on the current device, ordered on `st`: the unpadded 4-wide
// records (breadth-first) and the leaf order, on the device and copied to the host.  The host reads the cluster
// count back after every iteration and the node count after every level.  Fails -- with nothing to undo -- if the tree does
// not fit the traversal stack.
int build_ploc_device(const float *d_verts, int n, hipStream_t st, TreeBuild &out, const std::string &w) {
    if (n < 1) return fail(w + ": the device builder needs at least one triangle");
    int n_pad = 1;
    while (n_pad < n) n_pad <<= 1;
    const size_t n_all = 2 * (size_t)n - 1, cap_nodes = std::max(n - 1, 1);  // binary nodes; 4-wide nodes at most
    const int nb = (n + 255) / 256;
    DevScope tmp;
    unsigned long long *d_keys = nullptr;
    unsigned *d_bits = nullptr;
    float *d_box = nullptr, *d_cost = nullptr;
    int2 *d_child = nullptr, *d_sums = nullptr, *d_lvl[2] = {nullptr, nullptr};
    int *d_cnt = nullptr, *d_leaf = nullptr, *d_nn = nullptr, *d_tot = nullptr;
    PlocCluster *d_cl[2] = {nullptr, nullptr};
    if (tmp.alloc(d_keys, (size_t)n_pad) || tmp.alloc(d_bits, 6) || tmp.alloc(d_box, 6 * n_all) || tmp.alloc(d_cost, n_all) ||
        tmp.alloc(d_child, n_all) || tmp.alloc(d_cnt, n_all) || tmp.alloc(d_leaf, n_all) || tmp.alloc(d_nn, (size_t)n) ||
        tmp.alloc(d_sums, (size_t)nb) || tmp.alloc(d_tot, 4) || tmp.alloc(d_cl[0], (size_t)n) || tmp.alloc(d_cl[1], (size_t)n) ||
        tmp.alloc(d_lvl[0], cap_nodes) || tmp.alloc(d_lvl[1], cap_nodes))
        return 1;
    if (out.a.alloc(out.a.recs, 2 * cap_nodes) || out.a.alloc(out.a.order, (size_t)n)) return 1;
    HIP_TRY(hipEventCreate(&tmp.e0));
    HIP_TRY(hipEventCreate(&tmp.e1));
    HIP_TRY(hipEventRecord(tmp.e0, st));
    const dim3 blk(256);
    // keys: centroid bounds, quantisation, sort
    HIP_TRY(hipMemsetAsync(d_bits, 0xff, 3 * sizeof(unsigned), st));
    HIP_TRY(hipMemsetAsync(d_bits + 3, 0, 3 * sizeof(unsigned), st));
    hipLaunchKernelGGL(k_ploc_bounds, dim3(std::min(nb, 1024)), blk, 0, st, d_verts, n, d_bits);
    unsigned bits[6];
    HIP_TRY(hipMemcpyAsync(bits, d_bits, sizeof(bits), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float lo[3], sc3[3];
    for (int a = 0; a < 3; a++) {
        lo[a] = rtploc::from_ordered_bits(bits[a]);
        sc3[a] = rtploc::quant_scale(lo[a], rtploc::from_ordered_bits(bits[3 + a]));
    }
    hipLaunchKernelGGL(k_ploc_keys, dim3((n_pad + 255) / 256), blk, 0, st, d_verts, n, n_pad, lo[0], lo[1], lo[2], sc3[0], sc3[1],
                       sc3[2], d_keys);
    for (int k2 = 2; k2 <= n_pad; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1)
            hipLaunchKernelGGL(k_bitonic_step, dim3((n_pad + 255) / 256), blk, 0, st, d_keys, n_pad, j, k2);
    PlocNodes nd{d_box, d_child, d_cnt, d_cost, d_leaf, n};
    hipLaunchKernelGGL(k_ploc_leaves, dim3(nb), blk, 0, st, d_verts, d_keys, n, nd, d_cl[0]);
    HIP_TRY(hipGetLastError());
    // clustering: until one cluster is left
    const float trav = rtbvh::trav_cost();
    const int max_leaf = rtbvh::max_leaf();
    int m = n, inner = 0, cur = 0;
    while (m > 1) {
        if (++out.iterations > rtploc::kMaxIterations) return fail(w + ": the clustering does not converge");
        const int mb = (m + 255) / 256;
        hipLaunchKernelGGL(k_ploc_nearest, dim3(mb), blk, 0, st, d_cl[cur], m, out.iterations > rtploc::kTieIterations ? 1 : 0, d_nn);
        hipLaunchKernelGGL(k_ploc_count, dim3(mb), blk, 0, st, d_nn, m, d_sums);
        hipLaunchKernelGGL(k_ploc_scan, dim3(1), dim3(1024), 0, st, d_sums, mb, d_tot);
        hipLaunchKernelGGL(k_ploc_merge, dim3(mb), blk, 0, st, d_cl[cur], d_nn, m, d_sums, inner, trav, max_leaf, nd, d_cl[cur ^ 1]);
        HIP_TRY(hipGetLastError());
        int tot[2];
        HIP_TRY(hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (tot[1] < 1 || tot[0] != m - tot[1] || inner + tot[1] > n - 1)
            return fail(w + ": the clustering made no progress (non-finite vertices?)");
        m = tot[0];
        inner += tot[1];
        cur ^= 1;
    }
    // collapse to 4-wide, one level per step, breadth first from the root (node 2n - 2, or the one triangle)
    const int2 root = make_int2(n > 1 ? (int)n_all - 1 : 0, 0);
    HIP_TRY(hipMemcpyAsync(d_lvl[0], &root, sizeof(int2), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_tot + 2, 0, sizeof(int), st));
    int count = 1, base = 0, lv = 0;
    while (count > 0) {
        out.max_depth++;
        if (3 * out.max_depth + 1 > kMaxStackBound)
            return fail(w + ": the device-built tree is deeper than the traversal stack allows (" + std::to_string(out.max_depth) + " levels)");
        const int cb = (count + 255) / 256;
        hipLaunchKernelGGL(k_ploc_level_count, dim3(cb), blk, 0, st, d_lvl[lv], count, nd, d_sums);
        hipLaunchKernelGGL(k_ploc_scan, dim3(1), dim3(1024), 0, st, d_sums, cb, d_tot);
        int tot[2];
        HIP_TRY(hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const int next_base = base + count;
        if (tot[0] < 0 || (size_t)next_base + (size_t)tot[0] > cap_nodes) return fail(w + ": the 4-wide collapse overran its node count");
        hipLaunchKernelGGL(k_ploc_level_emit, dim3(cb), blk, 0, st, d_lvl[lv], count, base, next_base, d_sums, nd, out.a.recs,
                           d_lvl[lv ^ 1], out.a.order, d_tot + 2);
        HIP_TRY(hipGetLastError());
        base = next_base;
        count = tot[0];
        lv ^= 1;
    }
    HIP_TRY(hipEventRecord(tmp.e1, st));
    HIP_TRY(hipEventSynchronize(tmp.e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, tmp.e0, tmp.e1));
    out.seconds = ms * 1e-3;
    int err = 0;
    HIP_TRY(hipMemcpy(&err, d_tot + 2, sizeof(int), hipMemcpyDeviceToHost));
    if (err) return fail(w + ": the device-built tree has a leaf that cannot be referenced");
    out.quads.resize(2 * (size_t)base);
    out.order.resize((size_t)n);
    HIP_TRY(hipMemcpy(out.quads.data(), out.a.recs, sizeof(rtbvh::Pair) * out.quads.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out.order.data(), out.a.order, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    out.stack_bound = 3 * out.max_depth + 1;
    out.leaves = 0;
    for (const rtbvh::Pair &p : out.quads) out.leaves += (p.llink < 0 && p.llink != rtbvh::kNoChild) + (p.rlink < 0 && p.rlink != rtbvh::kNoChild);
    return 0;
}
// What the scene may adopt from a device build: a well-formed tree over a permutation of its triangles, within the stack
bool ploc_result_ok(const TreeBuild &b, int n) {
    if (b.stack_bound > kMaxStackBound || !validate_quads(b.quads, n) || (int)b.order.size() != n) return false;
    std::vector<char> seen((size_t)n, 0);
    for (int32_t i : b.order) {
        if (i < 0 || i >= n || seen[(size_t)i]) return false;
        seen[(size_t)i] = 1;
    }
    return true;
}

// ---- the one tail after "a tree exists", in two halves (rt_scene_rebuild launches its own kernel between them)
// The emit half: the leaf-order arrays for the tree `b`, allocated for its size into b.a and written from `src` and the
// vertices on the device (emit_scene; 2-wide: the nodes are the builder's pairs), ordered on `st`.  A scene that has no
// material table on the device yet gets the host's.  `d_inverse`: the inverse of the new leaf order, scratch in `tmp`.  The
// caller holds pad_mutex and has made the scene's device current; the scene still renders its old bits.
int emit_tree(rt_scene *sc, TreeBuild &b, EmitSource &src, const float *d_verts, hipStream_t st, DevScope &tmp, int *&d_inverse) {
    FreshArrays &a = b.a;
    const size_t n = (size_t)src.n_tris;
    if (a.alloc(a.nodes, 4 * (size_t)b.n_records()) || a.alloc(a.tris, 3 * n) || a.alloc(a.shade, n) || a.alloc(a.info, n) ||
        a.alloc(a.lights, (size_t)src.n_lights) || a.alloc(a.tables, (size_t)tab_dwords(src.n_mats, src.n_lights)) || tmp.alloc(d_inverse, n))
        return 1;
    if (!src.d_mats) {
        if (a.alloc(a.mats, (size_t)src.n_mats)) return 1;
        if (src.n_mats) HIP_TRY(hipMemcpyAsync(a.mats, src.h_mats, sizeof(Material) * (size_t)src.n_mats, hipMemcpyHostToDevice, st));
        src.d_mats = a.mats;
    }
    if (!sc->d_radius) HIP_TRY(hipMalloc((void **)&sc->d_radius, sizeof(float) * 3));  // (scratch of emit_nodes: a scene just made)
    if (!b.wide() && upload_pairs(b.pairs, a.nodes)) return 1;
    return emit_scene(sc, src, d_verts, a.view(b.n_records()), d_inverse, st);
}
// The adopt half: wait for `st`, then the scene takes the arrays, the tree and what the host knows of both -- the counts of
// `src`, the radius the 4-wide nodes were padded for.  What belongs to the old tree goes (the refit levels, the queries'
// inverse order); the SAH baselines are the new tree's.  Until the wait has succeeded the scene is untouched.
int adopt_tree(rt_scene *sc, TreeBuild &b, const EmitSource &src, hipStream_t st) {
    float radius[3] = {0.f, 0.f, 0.f};
    if (b.wide()) HIP_TRY(hipMemcpyAsync(radius, sc->d_radius, sizeof(radius), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    sc->adopt(b.a);
    sc->n_nodes = b.n_records();
    sc->h_quads = std::move(b.quads);
    sc->set_order(b.order);
    sc->drop_query_inverse();
    sc->max_depth = b.max_depth;
    sc->stack_bound = b.stack_bound;
    sc->n_leaves = b.leaves;
    sc->builder = b.builder;
    sc->build_seconds = b.seconds;
    sc->n_tris = src.n_tris;
    sc->n_mats = src.n_mats;
    sc->n_lights = src.n_lights;
    sc->tab_dwords = tab_dwords(src.n_mats, src.n_lights);
    for (int k = 0; k < 3; k++) sc->origin_radius[k] = radius[k];
    sc->drop_refit();
    sc->sah_build = sc->sah_now = quads_sah(sc->h_quads);
    return 0;
}

// A new, empty scene on the current device (RT_BVH_WIDE=0: the 2-wide experiment format)
int new_scene(std::unique_ptr<rt_scene> &sc) {
    sc = std::make_unique<rt_scene>();
    HIP_TRY(hipGetDevice(&sc->device));
    sc->wide = true;  // 4-wide nodes (two pair-style records each): half the dependent fetches per ray; RT_BVH_WIDE=0: 2-wide
    if (const char *e = knob("RT_BVH_WIDE")) sc->wide = atoi(e) != 0;
    return 0;
}

static_assert(sizeof(Light) == sizeof(rt_light), "light layout");
static_assert(sizeof(Material) == sizeof(rt_material), "material layout");
static_assert(sizeof(Camera) == sizeof(rt_camera), "camera layout");

// rt_scene_create / rt_scene_create_flags: a scene of any count of triangles from host arrays, its tree from the host SAH
// builder or (RT_SCENE_DEVICE_BVH) the device builder, on the current device and the null stream.  An error on the way
// frees the scene with everything it holds.
int scene_create_impl(const float *tri_p0p1p2, int n_tris, const int32_t *tri_material, const int32_t *tri_light, const rt_material *materials,
                      int n_materials, const rt_light *lights, int n_lights, uint32_t scene_flags, rt_scene **out_scene) {
    if (!out_scene) return fail("rt_scene_create: out_scene is null");
    if (scene_flags & ~(uint32_t)RT_SCENE_DEVICE_BVH) return fail("rt_scene_create_flags: unknown scene flags");
    const bool device_bvh = (scene_flags & RT_SCENE_DEVICE_BVH) != 0;
    *out_scene = nullptr;
    if (check_scene_counts("rt_scene_create", n_tris, n_tris <= 0 || (tri_p0p1p2 && tri_material), materials, n_materials, lights, n_lights) ||
        check_tri_indices("rt_scene_create", n_tris, tri_material, tri_light, n_materials, n_lights) ||
        check_scene_tables("rt_scene_create", n_tris, materials, n_materials, lights, n_lights))
        return 1;
    std::unique_ptr<rt_scene> sc;
    if (new_scene(sc)) return 1;
    if (device_bvh && !sc->wide) return fail("rt_scene_create_flags: the device builder writes the 4-wide format only (RT_BVH_WIDE=0 is set)");
    // the host mirrors first: the source of the emit is the scene's own (scene_source)
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
    const float *d_verts = nullptr;
    if (n_tris > 0 && stage(tmp, tri_p0p1p2, 9 * (size_t)n_tris, nullptr, d_verts)) return 1;
    TreeBuild b;
    if (device_bvh && n_tris > 0) {
        if (build_ploc_device(d_verts, n_tris, nullptr, b, "rt_scene_create_flags")) return 1;
        if (!ploc_result_ok(b, n_tris)) return fail("rt_scene_create_flags: the device-built tree is malformed");
    } else if (build_sah_host(tri_p0p1p2, n_tris, sc->wide, device_bvh, b)) {
        return 1;
    }
    sc->wide = b.wide();
    EmitSource src;
    int *d_inverse = nullptr;
    if (scene_source(sc.get(), true, nullptr, tmp, src) || emit_tree(sc.get(), b, src, d_verts, nullptr, tmp, d_inverse) ||
        adopt_tree(sc.get(), b, src, nullptr))
        return 1;
    HIP_TRY(hipDeviceSynchronize());
    *out_scene = sc.release();
    return 0;
}

// rt_render_multi: the scene as it exists on `device` -- the scene itself, or a replica created there from the host copies
// (once per device, under the scene's replica_mutex).  Null, with the error set, if that fails.
const rt_scene *scene_on_device(const rt_scene *scene, int device) {
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
    const int rc = scene_create_impl(scene->h_tri9.data(), scene->n_tris, scene->h_tri_material.data(),
                                     scene->h_tri_light.empty() ? nullptr : scene->h_tri_light.data(), scene->h_materials.data(),
                                     scene->n_mats, scene->h_lights.data(), scene->n_lights,
                                     scene->builder == 2 ? (uint32_t)RT_SCENE_DEVICE_BVH : 0u, &rep);
    if (rc != 0) return nullptr;
    scene->replicas.push_back(rep);
    return rep;
}

// rt_scene_rebuild / rt_scene_rebuild_device: a new tree for the scene's current or new vertices (build_ploc_device), and
// everything the kernels index in leaf order re-emitted on the device from the new order (emit_tree), into new buffers that
// replace the scene's only once the tree has passed its checks.  `verts`: null (the scene's own vertices), a host array or
// (device_ptr) a buffer on the scene's device.
int scene_rebuild_impl(rt_scene *sc, const float *verts, int n_tris, bool device_ptr, hipStream_t st, const char *what) {
    const std::string w(what);
    if (!sc) return fail(w + ": null scene");
    if (n_tris != sc->n_tris) return fail(w + ": " + std::to_string(n_tris) + " triangles, the scene was created with " + std::to_string(sc->n_tris));
    if (!sc->wide) return fail(w + ": the scene uses the 2-wide experiment format (RT_BVH_WIDE=0), which the device builder does not write");
    if (n_tris < 1) return fail(w + ": the scene has no triangles");
    std::lock_guard<std::mutex> pad_lock(sc->pad_mutex);  // (the records, h_quads and origin_radius change)
    DeviceGuard dev;
    DevScope tmp;
    const float *d_verts = nullptr;
    if (stage_vertices(sc, verts, device_ptr, st, w, dev, tmp, d_verts)) return 1;
    const int n = n_tris;
    std::vector<float> h_new;
    if (verts) {
        h_new.resize(9 * (size_t)n);
        if (device_ptr) {
            HIP_TRY(hipMemcpyAsync(h_new.data(), verts, sizeof(float) * h_new.size(), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        } else {
            memcpy(h_new.data(), verts, sizeof(float) * h_new.size());
        }
    }
    const bool moved = verts && memcmp(h_new.data(), sc->h_tri9.data(), sizeof(float) * h_new.size()) != 0;
    TreeBuild b;
    if (build_ploc_device(d_verts, n, st, b, w)) return 1;
    if (!ploc_result_ok(b, n)) return fail(w + ": the device-built tree is malformed; the scene is unchanged");
    // the reference's tree is a function of the triangles: kept (renumbered for the new leaf order) unless they moved
    const bool keep_ref = sc->ref_ready && !moved;
    int *d_inverse = nullptr, *d_ref_prims = nullptr, *d_ref_leaf_of = nullptr;
    DevScope ref;  // (released unless adopted below)
    if (keep_ref && (ref.alloc(d_ref_prims, (size_t)n) || ref.alloc(d_ref_leaf_of, (size_t)n))) return 1;
    EmitSource src;
    if (scene_source(sc, true, st, tmp, src) || emit_tree(sc, b, src, d_verts, st, tmp, d_inverse)) return 1;
    if (keep_ref)
        hipLaunchKernelGGL(k_ploc_remap_ref, dim3((n + 255) / 256), dim3(256), 0, st, sc->d_ref_prims, sc->d_ref_leaf_of, sc->d_order,
                           d_inverse, n, d_ref_prims, d_ref_leaf_of);
    HIP_TRY(hipGetLastError());
    if (adopt_tree(sc, b, src, st)) return 1;
    if (keep_ref) {
        std::lock_guard<std::mutex> lock(sc->ref_mutex);
        ref.ptrs.clear();
        std::swap(sc->d_ref_prims, d_ref_prims);
        std::swap(sc->d_ref_leaf_of, d_ref_leaf_of);
        (void)hipFree(d_ref_prims);
        (void)hipFree(d_ref_leaf_of);
    } else if (moved) {
        sc->drop_ref_tree();
    }
    if (moved) sc->h_tri9 = h_new;
    sc->drop_replicas();
    return 0;
}

// ---- editing a scene in place: rt_scene_set_materials, rt_scene_set_lights, rt_scene_set_triangles*, rt_scene_create_device
// Every one builds what changes into fresh buffers, waits for the device, and only then adopts them: an error on the way
// leaves the scene rendering its old bits.

// A new material table.  Nothing in leaf order depends on it: the table on the device and the shading tables are re-made
// (k_build_tables, for the new count), the tree, the records, the refit state and the reference's tree stay.
int scene_set_materials_impl(rt_scene *sc, const rt_material *materials, int n_materials) {
    const std::string w("rt_scene_set_materials");
    if (!sc) return fail(w + ": null scene");
    if (!materials) return fail(w + ": null materials");
    if (check_scene_counts(w, sc->n_tris, true, materials, n_materials, sc->h_lights.data(), sc->n_lights) ||
        check_scene_tables(w, sc->n_tris, materials, n_materials, nullptr, 0))
        return 1;
    if (sc->max_tri_material >= n_materials)
        return fail(w + ": the triangles name materials up to " + std::to_string(sc->max_tri_material) + ", the new table has " + std::to_string(n_materials));
    std::lock_guard<std::mutex> pad_lock(sc->pad_mutex);
    DeviceGuard dev;
    if (dev.enter(sc->device)) return 1;
    FreshArrays a;
    const int n_tab = tab_dwords(n_materials, sc->n_lights);
    if (a.alloc(a.mats, (size_t)n_materials) || a.alloc(a.tables, (size_t)n_tab)) return 1;
    if (n_materials) HIP_TRY(hipMemcpy(a.mats, materials, sizeof(Material) * (size_t)n_materials, hipMemcpyHostToDevice));
    launch_build_tables(a.mats, n_materials, sc->d_lights, sc->n_lights, sc->d_tris, a.tables, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    sc->adopt(a);
    sc->n_mats = n_materials;
    sc->tab_dwords = n_tab;
    sc->h_materials.assign(materials, materials + n_materials);
    sc->drop_replicas();
    return 0;
}

// New lights and, with `tri_light`, a new light assignment of the triangles.  The lights' triangles are renumbered to leaf
// order from the host's inverse order (what k_leaf_lights does after a build); a new assignment re-emits tri_info and the
// shading records (k_leaf_tri_light, k_build_tri_shade).  The tree, the triangle records and the reference's tree stay.
int scene_set_lights_impl(rt_scene *sc, const rt_light *lights, int n_lights, const int32_t *tri_light) {
    const std::string w("rt_scene_set_lights");
    if (!sc) return fail(w + ": null scene");
    if (check_scene_counts(w, sc->n_tris, true, sc->h_materials.data(), sc->n_mats, lights, n_lights) ||
        check_tri_indices(w, sc->n_tris, nullptr, tri_light, sc->n_mats, n_lights) ||
        check_scene_tables(w, sc->n_tris, nullptr, 0, lights, n_lights))
        return 1;
    if (!tri_light && sc->max_tri_light >= n_lights)
        return fail(w + ": the kept assignment names lights up to " + std::to_string(sc->max_tri_light) + ", the new table has " + std::to_string(n_lights));
    std::lock_guard<std::mutex> pad_lock(sc->pad_mutex);
    DeviceGuard dev;
    if (dev.enter(sc->device)) return 1;
    const int n = sc->n_tris;
    std::vector<rt_light> leaf_lights(lights, lights + n_lights);
    for (rt_light &l : leaf_lights)
        if (l.type == RT_AREA_LIGHT) l.triangle = sc->h_inverse[(size_t)l.triangle];
    FreshArrays a;
    DevScope tmp;
    const int n_tab = tab_dwords(sc->n_mats, n_lights);
    if (a.alloc(a.lights, (size_t)n_lights) || a.alloc(a.tables, (size_t)n_tab)) return 1;
    if (n_lights) HIP_TRY(hipMemcpy(a.lights, leaf_lights.data(), sizeof(Light) * (size_t)n_lights, hipMemcpyHostToDevice));
    if (tri_light && n > 0) {
        const int *d_tl = nullptr;
        if (a.alloc(a.info, (size_t)n) || a.alloc(a.shade, (size_t)n) || stage(tmp, tri_light, (size_t)n, nullptr, d_tl)) return 1;
        const dim3 blk(256), grid((n + 255) / 256);
        hipLaunchKernelGGL(k_leaf_tri_light, grid, blk, 0, nullptr, sc->d_tri_info, d_tl, sc->d_order, n, a.info);
        hipLaunchKernelGGL(k_build_tri_shade, grid, blk, 0, nullptr, sc->d_tris, a.info, n, a.shade);
    }
    launch_build_tables(sc->d_mats, sc->n_mats, a.lights, n_lights, sc->d_tris, a.tables, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    sc->adopt(a);
    sc->n_lights = n_lights;
    sc->tab_dwords = n_tab;
    sc->h_lights.assign(lights, lights + n_lights);
    if (tri_light) {
        sc->h_tri_light.assign(tri_light, tri_light + n);
        sc->note_index_maxima();
    }
    sc->drop_replicas();
    return 0;
}

// A new triangle set for the scene (or the first one of a scene just made: rt_scene_create_device): any count >= 1, with
// its per-triangle indices and the tables they index.  The three per-triangle arrays are host arrays, uploaded first, or
// (device_ptr) buffers on the scene's device, whose index ranges are then checked there (k_index_prepass); from then on
// there is one path: the device build, the tail every tree goes through (emit_tree, adopt_tree), the host mirrors.
int scene_set_triangles_impl(rt_scene *sc, const float *verts, int n_tris, const int32_t *tri_material, const int32_t *tri_light,
                             const rt_material *materials, int n_materials, const rt_light *lights, int n_lights, bool device_ptr,
                             hipStream_t st, const char *what) {
    const std::string w(what);
    if (!sc) return fail(w + ": null scene");
    if (check_scene_counts(w, n_tris, verts && tri_material, materials, n_materials, lights, n_lights)) return 1;
    if (n_tris < 1) return fail(w + ": the device builder needs at least one triangle (an empty scene is made by rt_scene_create)");
    if (!sc->wide) return fail(w + ": the scene uses the 2-wide experiment format (RT_BVH_WIDE=0), which the device builder does not write");
    if (!device_ptr && check_tri_indices(w, n_tris, tri_material, tri_light, n_materials, n_lights)) return 1;
    if (check_scene_tables(w, n_tris, materials, n_materials, lights, n_lights)) return 1;
    if (device_ptr) {
        const std::string where = " is not device memory on the scene's device " + std::to_string(sc->device);
        if (!on_device(verts, sc->device)) return fail(w + ": d_tri_p0p1p2" + where);
        if (!on_device(tri_material, sc->device)) return fail(w + ": d_tri_material" + where);
        if (tri_light && !on_device(tri_light, sc->device)) return fail(w + ": d_tri_light" + where);
    }
    std::lock_guard<std::mutex> pad_lock(sc->pad_mutex);  // (the records, h_quads and origin_radius change)
    DeviceGuard dev;
    if (dev.enter(sc->device)) return 1;
    DevScope tmp;
    const size_t n = (size_t)n_tris;
    const float none[3] = {0.f, 0.f, 0.f};  // the new tree's own radius, as at creation: the old triangles' says nothing
    const float *d_verts = verts;
    EmitSource src{n_tris, n_materials, n_lights, nullptr, materials, lights, tri_material, tri_light, none};  // (d_mats null: a new table)
    std::vector<float> h_tri9(9 * n);
    std::vector<int32_t> h_mat(n), h_light(tri_light ? n : 0);
    if (!device_ptr) {
        if (stage(tmp, verts, 9 * n, st, d_verts) || stage(tmp, tri_material, n, st, src.d_tri_material) ||
            (tri_light && stage(tmp, tri_light, n, st, src.d_tri_light)))
            return 1;
        memcpy(h_tri9.data(), verts, sizeof(float) * 9 * n);
        memcpy(h_mat.data(), tri_material, sizeof(int32_t) * n);
        if (tri_light) memcpy(h_light.data(), tri_light, sizeof(int32_t) * n);
        HIP_TRY(hipStreamSynchronize(st));  // (the caller's arrays are their own again on return whatever happens below)
    } else {
        unsigned *d_words = nullptr, words[2] = {0, 0};
        if (tmp.alloc(d_words, 2)) return 1;
        HIP_TRY(hipMemsetAsync(d_words, 0, sizeof(words), st));
        hipLaunchKernelGGL(k_index_prepass, dim3((unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, 1024)), dim3(kBlock), 0, st,
                           src.d_tri_material, src.d_tri_light, n_tris, n_materials, n_lights, d_words);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, st));
        // the host mirrors: what the reference's tree and rt_render_multi replicas are made from, one copy per array
        HIP_TRY(hipMemcpyAsync(h_tri9.data(), verts, sizeof(float) * 9 * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_mat.data(), tri_material, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        if (tri_light) HIP_TRY(hipMemcpyAsync(h_light.data(), tri_light, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (words[0] || words[1])
            return fail(w + ": " + std::to_string(words[0]) + " of " + std::to_string(n_tris) + " triangles have d_tri_material out of range and " +
                        std::to_string(words[1]) + " have d_tri_light out of range");
    }
    TreeBuild b;
    if (build_ploc_device(d_verts, n_tris, st, b, w)) return 1;
    if (!ploc_result_ok(b, n_tris)) return fail(w + ": the device-built tree is malformed; the scene is unchanged");
    int *d_inverse = nullptr;
    if (emit_tree(sc, b, src, d_verts, st, tmp, d_inverse) || adopt_tree(sc, b, src, st)) return 1;
    sc->drop_ref_tree();
    sc->h_tri9 = std::move(h_tri9);
    sc->h_tri_material = std::move(h_mat);
    sc->h_tri_light = std::move(h_light);
    sc->h_materials.assign(materials, materials + n_materials);
    sc->h_lights.assign(lights, lights + n_lights);
    sc->note_index_maxima();
    sc->drop_replicas();
    return 0;
}

// rt_scene_create_device: an empty scene on the current device that takes its first triangle set from device buffers
int scene_create_device_impl(const float *d_tri_p0p1p2, int n_tris, const int32_t *d_tri_material, const int32_t *d_tri_light,
                             const rt_material *materials, int n_materials, const rt_light *lights, int n_lights, hipStream_t st,
                             rt_scene **out_scene) {
    if (!out_scene) return fail("rt_scene_create_device: out_scene is null");
    *out_scene = nullptr;
    std::unique_ptr<rt_scene> sc;
    if (new_scene(sc) || scene_set_triangles_impl(sc.get(), d_tri_p0p1p2, n_tris, d_tri_material, d_tri_light, materials, n_materials, lights,
                                                  n_lights, true, st, "rt_scene_create_device"))
        return 1;
    *out_scene = sc.release();
    return 0;
}

