// rt_walk.inc -- the walk every ray kernel shares: the box test, the traversal stack, the node step, the literal reference walk
// and the VERIFY procedure (the reference's decisions on the product's walk).  Included by rtcuda_amd.hip, once.
// ============================================================================ traversal
// One wave-wide traversal engine serves every ray kernel (closest-hit over the path pools = ch(),
// render.cuh:297-328; any-hit over the shadow queue = ah(), :278-294; the queries and the trace
// hooks on top of them), so the parity tests exercise exactly the code the renderer runs.
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
// The box test only culls: it is conservative for the ray the triangle test sees (boxes padded by the builder, exit distance
// widened by 8 ulp, 1 / d of the true direction, distance limit widened for edge-on triangles: rt_bvh.h) and may use any
// arithmetic.  The triangle test is the reference's, bit for bit.
struct RayPrep {
    V3 o, d, inv;
};
__device__ __forceinline__ V3 inv_dir(V3 d) {
    // 1 / d of the TRUE direction: the cull must be conservative for the ray the triangle test sees, so a component is only kept
    // away from 0 far enough for 1 / d to stay finite (rt_bvh.h, kCullDirFloor) -- the reference's clamp to FLT_EPSILON
    // (aabb_intersector.cuh:17-19) is restated where its decisions are: ref_slab / ref_visible.  The reciprocal itself is the
    // hardware's v_rcp_f32 (1 ulp) rather than an IEEE division (11 instructions each, three per ray): 1 / d only feeds
    // the box test, which only culls -- box_hit / inner_step widen the exit distance by 8 ulps, which covers the 1 ulp
    // per axis this costs on top of the rounding of the slab arithmetic (the builder pads every box by 2 ulps)
    constexpr float f = rtbvh::kCullDirFloor;
    float ix = __builtin_amdgcn_rcpf((fabsf(d.x) < f) ? copysignf(f, d.x) : d.x);
    float iy = __builtin_amdgcn_rcpf((fabsf(d.y) < f) ? copysignf(f, d.y) : d.y);
    float iz = __builtin_amdgcn_rcpf((fabsf(d.z) < f) ? copysignf(f, d.z) : d.z);
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
    return t_in <= t_out && t_out >= 0.f && t_in <= tmax * rtbvh::kCullTmaxWiden;  // (see inner_step)
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
// exactly the same t (a shared edge) the one its BVH walk tests LAST wins (SURVEY Appendix A.10) -- a property of the
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
        // (tmax is widened: the entry distance carries a few ulps of rounding, and a shadow ray that ends ON a triangle
        // coplanar with an occluder -- light quads -- has entry = t = tmax to the last bit; unwidened, the full-size audit of
        // the sixteen-light scene lost 1 occluder in 9.8e8 shadow rays.  By more than the exit distance: the t of a triangle
        // seen edge-on is computed in FRONT of its box, rt_bvh.h kCullTmaxWiden)
        const float tmax_w = tmax * rtbvh::kCullTmaxWiden;
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
        const float tmax_w = fminf(tmax * rtbvh::kCullTmaxWiden, kFltMax);
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

// ---- the two hit rules and the closest hit's finalisation, as the stream walker (k_query, k_aov: rt_stream_kernels.inc) applies
// them.  k_trace and k_paths hold the hit rules in their own text: k_trace's lanes carry their ray kind at run time and
// k_paths' triangle block tests two triangles per step beside a speculated leaf, its finalisation sits between the ADV block's
// reloads of the slot state -- and with leaf_hits in place neither kernel's instances compile to the instructions they had
// (profiles/stream_walk.md), which is the bar for touching them.  k_trace, pool-only, does share verify_closest
// (profiles/trace_hooks.md).  A change to a rule is made here, in k_trace's leaf phase, and in the ADV and triangle blocks of
// rt_frame_kernels.inc.
// The triangles of leaf `ref` (= ~cur: first << 3 | count) against the lane's ray (triangle.cuh:39-58).  `tri` / `tmax`: best hit
// so far (closest) or the excluded triangle (any hit).  True: the ray is finished -- an any-hit ray found its occluder, hu = 1.
//   any hit: bvh.cuh:243, the first accepted hit that is not the excluded triangle (VERIFY: and that the reference's walk can
//            see at all: the walk goes on past an unseen occluder);
//   closest: bvh.cuh:227-231 (t <= tmax), ties by closest_hit_wins.  VERIFY: an exact tie is the reference's tree order to decide
//            (triangle.cuh:49): marked in the sign of hv for verify_closest (v >= 0 for an accepted hit; a closer hit later
//            overwrites the mark with its own v).
template <bool ANY, bool VERIFY>
__device__ __forceinline__ bool leaf_hits(const DScene &sc, V3 o, V3 d, int ref, float &tmax, int &tri, float &hu,
                                          float &hv, unsigned long long *vstat) {
    const int first = ref >> 3, count = ref & 7;
    for (int k = first; k < first + count; k++) {
        const Tri tr = load_tri(sc.tris, k);
        float t, u, v;
        if (tri_intersect(tr, o, d, tmax, t, u, v)) {
            if (ANY) {
                if (k != tri && (!VERIFY || ref_visible(sc, o, d, tr, k, vstat))) {
                    hu = 1.f;  // occluded
                    return true;
                }
            } else {
                const bool tie = t == tmax && tri >= 0;
                if (closest_hit_wins(sc, t, tmax, k, tri)) {
                    tmax = t;
                    hu = u;
                    hv = v;
                    tri = k;
                }
                if (VERIFY && tie) hv = __uint_as_float(__float_as_uint(hv) | 0x80000000u);
            }
        }
    }
    return false;
}
// VERIFY, a finished closest-hit ray that holds a hit (tri >= 0): the hit stands if the reference's walk can see its triangle
// and nothing tied with it at the final distance (the sign of hv: leaf_hits); otherwise (~2 rays in 10^7) the ray is re-traced
// literally, from `restart_tmax()` -- the limit the ray started with, asked for on the rare path only.
template <class RESTART>
__device__ __forceinline__ void verify_closest(const DScene &sc, V3 o, V3 d, RESTART restart_tmax, float &tmax, int &tri, float &hu,
                                               float &hv, unsigned long long *vstat, int *stack, int *over, int stack_cap) {
    bool bad = (__float_as_uint(hv) >> 31) != 0u;
    if (bad) {
        atomicAdd(&vstat[V_TIE], 1ull);
    } else {
        const Tri tr = load_tri(sc.tris, tri);
        bad = !ref_visible(sc, o, d, tr, tri, vstat);
    }
    if (bad) {
        atomicAdd(&vstat[V_LITERAL], 1ull);
        tmax = restart_tmax();
        tri = -1;
        hu = hv = 0.f;
        reference_walk<false>(sc, o, d, tmax, tri, hu, hv, stack, over, stack_cap);
    }
}
