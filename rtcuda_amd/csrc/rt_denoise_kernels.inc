// rt_denoise_fixed on the device (include/rtcuda_amd.h; DESIGN.md section 2.7).  The arithmetic is rt_denoise.h's, shared with
// the CPU twin; here is who walks the pixels and where the records live.
//
// Scratch: three arrays of one 16-byte record per pixel.  {u.x, u.y, u.z, z} twice -- a pass reads one and writes the other --
// and {n.x, n.y, n.z, 0} once.  A tap is two dwordx4 loads.  d and e are not kept: k_dn_finish forms them again from the sums
// (112 bytes per pixel read once, against 32 written and read back).
//
// k_atrous, the direct form: a workgroup is a 32 x 8 tile of pixels (kDnTileW x kDnTileH: a wave is two rows of 32, so a tap
// of the wave reads two runs of 512 contiguous bytes per array), a lane is a pixel and loads its 24 neighbours from global
// memory; neighbouring lanes' taps overlap, so all but the first touch of a record is served by L1 / L2.  The grid is
// one-dimensional (tiles in row order).
//
// k_atrous_lds, the LDS form: the pixels p = r (mod stride), per residue r = (rx, ry), form a sub-image on which the pass is a
// 5 x 5 filter of stride 1 (for stride 1 the sub-image is the image).  A workgroup takes a 32 x 8 tile of one sub-image, stages
// the tile plus its halo of 2 -- 36 x 12 records of each array, 13.5 KiB -- in LDS, and every lane filters its pixel from there:
// 3.4 global loads per pixel instead of 50, strided by 16 * stride bytes.  Workgroups that follow each other in the grid hold
// the SAME tile of neighbouring residues, so the lines a strided read leaves half used are used by the neighbours while
// they are still cached.  Tap order, skip rule and arithmetic are the direct form's: the same bits.
// Which form a pass runs: dn_lds_wins (rt_host_denoise.inc), from the timings of profiles/denoise_time.json.
constexpr int kDnTileW = 32, kDnTileH = 8;
static_assert(kDnTileW * kDnTileH == kBlock, "a tile is a workgroup");

__global__ void __launch_bounds__(kBlock) k_dn_prepare(const long long *__restrict__ sums, const long long *__restrict__ aov,
                                                        long long n_pixels, float inv_spp, float inv_aov,
                                                        float4 *__restrict__ uz, float4 *__restrict__ nrm) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    DnPixel px;
    dn_prepare((const int64_t *)sums + 3 * p, (const int64_t *)aov + DN_AOV_CHANNELS * p, inv_spp, inv_aov, &px);
    uz[p] = make_float4(px.u[0], px.u[1], px.u[2], px.z);
    nrm[p] = make_float4(px.n[0], px.n[1], px.n[2], 0.f);
}

// The one tap loop: pixel (x, y) of a pass, from its own two records c and cn and whatever `tap` hands back for a neighbour.
// kVar = false: rt_denoise_fixed, z rides in c.w / t.w and is passed on, k is the pass's kc.  kVar = true: rt_denoise_dual_fixed
// (below), z rides in cn.w / tn.w, c.w / t.w is v and is filtered with w * w, k is the pixel's r.
// tap(dx, dy, q, t, tn) fills in the two records of the neighbour (dx, dy), which is pixel q of the frame; x has the caller's type.
template <bool kVar, typename X, typename Tap>
__device__ __forceinline__ float4 dn_filter_pixel(X x, long long y, int width, int height, int stride, const float4 c, const float4 cn,
                                                  float k, float kz, int normal_power_log2, Tap tap) {
    const float up[3] = {c.x, c.y, c.z}, np[3] = {cn.x, cn.y, cn.z};
    float sw = 0.f, sv = 0.f, su[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const long long yy = y + (long long)stride * dy;
        if (yy < 0 || yy >= height) continue;
        const long long row = yy * width;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const long long xx = (long long)x + (long long)stride * dx;
            if (xx < 0 || xx >= width) continue;
            const float h = dn_kernel(dx) * dn_kernel(dy);
            float w = h, vq = c.w;
            float uq[3] = {up[0], up[1], up[2]};
            if (dx != 0 || dy != 0) {
                float4 t, tn;
                tap(dx, dy, row + xx, t, tn);
                const float nq[3] = {tn.x, tn.y, tn.z};
                uq[0] = t.x, uq[1] = t.y, uq[2] = t.z, vq = t.w;
                w = dn_tap_weight(h, up, kVar ? cn.w : c.w, np, uq, kVar ? tn.w : t.w, nq, k, kz, normal_power_log2);
            }
            sw = sw + w;
            for (int i = 0; i < 3; i++) su[i] = su[i] + w * uq[i];
            if (kVar) sv = sv + (w * w) * vq;
        }
    }
    return make_float4(su[0] / sw, su[1] / sw, su[2] / sw, kVar ? sv / (sw * sw) : c.w);
}

// What a pixel's colour distances are multiplied by: the pass's kc, or the pixel's r (kInlineG: see rt_denoise_dual_fixed below)
template <bool kVar, bool kInlineG, typename X>
__device__ __forceinline__ float dn_colour_scale(const float4 *src, const float *r_in, X x, long long y, int width, int height, float k) {
    if (!kVar) return k;
    return kInlineG ? dn_var_rcp(k, dn_var_blur((const float *)src, x, y, width, height)) : r_in[y * width + x];
}

template <bool kVar, bool kInlineG>
__device__ __forceinline__ void dn_pass_direct(const float4 *__restrict__ src, const float4 *__restrict__ nrm, const float *__restrict__ r_in,
                                               float4 *__restrict__ dst, int width, int height, int tiles_x, int stride, float k, float kz,
                                               int normal_power_log2) {
    const int tile_y = (int)(blockIdx.x / (unsigned)tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)tiles_x);
    const int x = tile_x * kDnTileW + (int)(threadIdx.x % kDnTileW);
    const long long y = (long long)tile_y * kDnTileH + (int)(threadIdx.x / kDnTileW);
    if (x >= width || y >= height) return;
    const long long p = y * width + x;
    const float4 c = src[p], cn = nrm[p];
    const float kp = dn_colour_scale<kVar, kInlineG>(src, r_in, x, y, width, height, k);
    dst[p] = dn_filter_pixel<kVar>(x, y, width, height, stride, c, cn, kp, kz, normal_power_log2,
                                   [&](int, int, long long q, float4 &t, float4 &tn) { t = src[q], tn = nrm[q]; });
}

constexpr int kDnHalo = 2, kDnLdsW = kDnTileW + 2 * kDnHalo, kDnLdsH = kDnTileH + 2 * kDnHalo;

template <bool kVar, bool kInlineG>
__device__ __forceinline__ void dn_pass_lds(const float4 *__restrict__ src, const float4 *__restrict__ nrm, const float *__restrict__ r_in,
                                            float4 *__restrict__ dst, int width, int height, int stride, int n_rx, int n_res, int lat_tiles_x,
                                            float k, float kz, int normal_power_log2) {
    __shared__ float4 s_a[kDnLdsH][kDnLdsW], s_b[kDnLdsH][kDnLdsW];  // src's and nrm's records of the tile and its halo
    const unsigned tile = blockIdx.x / (unsigned)n_res, res = blockIdx.x - tile * (unsigned)n_res;
    const int ry = (int)(res / (unsigned)n_rx), rx = (int)(res - (unsigned)ry * (unsigned)n_rx);
    const int tile_y = (int)(tile / (unsigned)lat_tiles_x), tile_x = (int)(tile - (unsigned)tile_y * (unsigned)lat_tiles_x);
    // lattice coordinates (lx, ly) of this residue's sub-image <-> pixel (rx + stride * lx, ry + stride * ly)
    const long long lx0 = (long long)tile_x * kDnTileW - kDnHalo, ly0 = (long long)tile_y * kDnTileH - kDnHalo;
    for (int i = (int)threadIdx.x; i < kDnLdsW * kDnLdsH; i += kBlock) {
        const int cy = i / kDnLdsW, cx = i - cy * kDnLdsW;
        const long long gx = rx + (long long)stride * (lx0 + cx), gy = ry + (long long)stride * (ly0 + cy);
        if (gx >= 0 && gx < width && gy >= 0 && gy < height) {  // (a cell outside the image is never read: its tap is skipped)
            const long long q = gy * width + gx;
            s_a[cy][cx] = src[q];
            s_b[cy][cx] = nrm[q];
        }
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x % kDnTileW), ty = (int)(threadIdx.x / kDnTileW);
    const long long x = rx + (long long)stride * (lx0 + kDnHalo + tx), y = ry + (long long)stride * (ly0 + kDnHalo + ty);
    if (x >= width || y >= height) return;
    const float4 *pa = &s_a[ty + kDnHalo][tx + kDnHalo], *pb = &s_b[ty + kDnHalo][tx + kDnHalo];  // the pixel's own cell
    const float4 c = *pa, cn = *pb;
    const float kp = dn_colour_scale<kVar, kInlineG>(src, r_in, x, y, width, height, k);
    dst[y * width + x] = dn_filter_pixel<kVar>(x, y, width, height, stride, c, cn, kp, kz, normal_power_log2,
                                               [&](int dx, int dy, long long, float4 &t, float4 &tn) {
                                                   t = pa[dy * kDnLdsW + dx], tn = pb[dy * kDnLdsW + dx];
                                               });
}

__global__ void __launch_bounds__(kBlock) k_atrous(const float4 *__restrict__ src, const float4 *__restrict__ nrm,
                                                    float4 *__restrict__ dst, int width, int height, int tiles_x, int stride,
                                                    float kc, float kz, int normal_power_log2) {
    dn_pass_direct<false, false>(src, nrm, nullptr, dst, width, height, tiles_x, stride, kc, kz, normal_power_log2);
}

__global__ void __launch_bounds__(kBlock) k_atrous_lds(const float4 *__restrict__ src, const float4 *__restrict__ nrm,
                                                        float4 *__restrict__ dst, int width, int height, int stride, int n_rx,
                                                        int n_res, int lat_tiles_x, float kc, float kz, int normal_power_log2) {
    dn_pass_lds<false, false>(src, nrm, nullptr, dst, width, height, stride, n_rx, n_res, lat_tiles_x, kc, kz, normal_power_log2);
}

__global__ void __launch_bounds__(kBlock) k_dn_finish(const float4 *__restrict__ uz, const long long *__restrict__ sums,
                                                       const long long *__restrict__ aov, long long n_pixels, float inv_spp,
                                                       float inv_aov, float *__restrict__ out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    DnPixel px;
    dn_prepare((const int64_t *)sums + 3 * p, (const int64_t *)aov + DN_AOV_CHANNELS * p, inv_spp, inv_aov, &px);
    const float4 r = uz[p];
    const float u[3] = {r.x, r.y, r.z};
    dn_finish(u, px.d, px.e, out + 3 * p);
}

// ---- rt_denoise_dual_fixed: the same machinery with a variance channel.  Scratch: {u.x, u.y, u.z, v} twice, {n.x, n.y, n.z, z}
// once (a tap is still two dwordx4 loads) and one float r per pixel.  Where a pixel's r = 1 / (ks * g + 2^-26) comes from is a
// template parameter of both pass forms.  kInlineG = true blurs the nine v around p in the pass itself, nine dword loads from
// the pass's input in global memory: lines the wave's taps touch anyway in the direct form and in the LDS form at stride 1; in
// the LDS form at larger strides the stride-1 neighbours are not in the residue's tile and each load touches a line per lane
// or two.  kInlineG = false reads the r that k_dn_var_blur wrote for the whole frame before the pass.  The same function of the
// same values: the same bits.  Which placement a pass runs: dn_dual_inline_g_wins (rt_host_denoise.inc), from
// profiles/denoise_dual_time.json.  (Not built: taking the nine v from the staged tile in the LDS form at stride 1.)
__global__ void __launch_bounds__(kBlock) k_dn_prepare_dual(const long long *__restrict__ sum_a, const long long *__restrict__ sum_b,
                                                             const long long *__restrict__ aov, long long n_pixels, float inv_a,
                                                             float inv_b, float inv_n, float inv_aov, float kv,
                                                             float4 *__restrict__ uv, float4 *__restrict__ nz) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    DnPixel px;
    const float v = dn_prepare_dual((const int64_t *)sum_a + 3 * p, (const int64_t *)sum_b + 3 * p,
                                    (const int64_t *)aov + DN_AOV_CHANNELS * p, inv_a, inv_b, inv_n, inv_aov, kv, &px);
    uv[p] = make_float4(px.u[0], px.u[1], px.u[2], v);
    nz[p] = make_float4(px.n[0], px.n[1], px.n[2], px.z);
}

// rt_denoise_variance_fixed: the same two records from one frame's sums and the caller's variance buffer; the passes are the dual
// filter's, the finish is k_dn_finish (it reads u and forms d and e from the one sum again).
__global__ void __launch_bounds__(kBlock) k_dn_prepare_var(const long long *__restrict__ sums, const float *__restrict__ variance,
                                                            const long long *__restrict__ aov, long long n_pixels, float inv_spp,
                                                            float inv_aov, float4 *__restrict__ uv, float4 *__restrict__ nz) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    DnPixel px;
    const float v = dn_prepare_var((const int64_t *)sums + 3 * p, (const int64_t *)aov + DN_AOV_CHANNELS * p, variance[p], inv_spp, inv_aov, &px);
    uv[p] = make_float4(px.u[0], px.u[1], px.u[2], v);
    nz[p] = make_float4(px.n[0], px.n[1], px.n[2], px.z);
}

__global__ void __launch_bounds__(kBlock) k_dn_var_blur(const float4 *__restrict__ src, float *__restrict__ r_out, int width, int height,
                                                         long long n_pixels, float ks) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const long long y = p / width, x = p - y * width;
    r_out[p] = dn_var_rcp(ks, dn_var_blur((const float *)src, x, y, width, height));
}

template <bool kInlineG>
__global__ void __launch_bounds__(kBlock) k_atrous_var(const float4 *__restrict__ src, const float4 *__restrict__ nz,
                                                        const float *__restrict__ r_in, float4 *__restrict__ dst, int width, int height,
                                                        int tiles_x, int stride, float ks, float kz, int normal_power_log2) {
    dn_pass_direct<true, kInlineG>(src, nz, r_in, dst, width, height, tiles_x, stride, ks, kz, normal_power_log2);
}

template <bool kInlineG>
__global__ void __launch_bounds__(kBlock) k_atrous_var_lds(const float4 *__restrict__ src, const float4 *__restrict__ nz,
                                                            const float *__restrict__ r_in, float4 *__restrict__ dst, int width,
                                                            int height, int stride, int n_rx, int n_res, int lat_tiles_x, float ks,
                                                            float kz, int normal_power_log2) {
    dn_pass_lds<true, kInlineG>(src, nz, r_in, dst, width, height, stride, n_rx, n_res, lat_tiles_x, ks, kz, normal_power_log2);
}

__global__ void __launch_bounds__(kBlock) k_dn_finish_dual(const float4 *__restrict__ uv, const long long *__restrict__ sum_a,
                                                            const long long *__restrict__ sum_b, const long long *__restrict__ aov,
                                                            long long n_pixels, float inv_n, float inv_aov, float *__restrict__ out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    int64_t s[3];
    for (int k = 0; k < 3; k++) s[k] = (int64_t)((uint64_t)sum_a[3 * p + k] + (uint64_t)sum_b[3 * p + k]);
    DnPixel px;
    dn_prepare(s, (const int64_t *)aov + DN_AOV_CHANNELS * p, inv_n, inv_aov, &px);
    const float4 r = uv[p];
    const float u[3] = {r.x, r.y, r.z};
    dn_finish(u, px.d, px.e, out + 3 * p);
}
