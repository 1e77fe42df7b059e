// rt_temporal_accumulate_fixed on the device (include/rtcuda_amd.h; DESIGN.md section 2.9).  The arithmetic is rt_temporal.h's,
// shared with the CPU twin (hc_temporal_accumulate); here is who walks the pixels.
//
// k_temporal_accumulate: a workgroup is a 32 x 8 tile of pixels, as k_atrous's (kDnTileW x kDnTileH: a wave is two rows of 32),
// a lane is a pixel.  Under a camera that moves by a few pixels the four taps of neighbouring lanes fall on neighbouring pixels
// of the previous frame, so a wave's tap reads runs of a few lines per array and all but the first touch of a line is served by
// L1 / L2.  The motion record is one 16-byte load; of the 88 bytes of an AOV pixel only normal, depth and hits are read (this
// frame's once, the previous frame's per tap); both colour buffers ride through one pass over the taps.  Nothing is staged in
// LDS: the taps' footprint is not known before the motion record is read.  The grid is one-dimensional (tiles in row order).
struct TemporalParams {
    const long long *sum_a, *sum_b, *aov, *hist_a_in, *hist_b_in, *prev_aov;
    const float4 *motion;
    const int *len_in;
    long long *out_a, *out_b;
    int *len_out;
    int width, height, tiles_x, max_history;
    float inv_a, inv_b, inv_aov, inv_prev_aov, alpha_min, depth_tolerance, normal_cos_min;
};
__global__ void __launch_bounds__(kBlock) k_temporal_accumulate(TemporalParams tp) {
    const int tile_y = (int)(blockIdx.x / (unsigned)tp.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)tp.tiles_x);
    const int x = tile_x * kDnTileW + (int)(threadIdx.x % kDnTileW);
    const long long y = (long long)tile_y * kDnTileH + (int)(threadIdx.x / kDnTileW);
    if (x >= tp.width || y >= tp.height) return;
    const float4 m4 = tp.motion[y * tp.width + x];
    const float mo[4] = {m4.x, m4.y, m4.z, m4.w};
    tm_accumulate_pixel(x, (int)y, tp.width, tp.height, (const int64_t *)tp.sum_a, tp.inv_a, (const int64_t *)tp.sum_b, tp.inv_b,
                        (const int64_t *)tp.aov, tp.inv_aov, mo, (const int64_t *)tp.hist_a_in, (const int64_t *)tp.hist_b_in, tp.len_in,
                        (const int64_t *)tp.prev_aov, tp.inv_prev_aov, tp.max_history, tp.alpha_min, tp.depth_tolerance, tp.normal_cos_min,
                        (int64_t *)tp.out_a, (int64_t *)tp.out_b, tp.len_out);
}

// k_temporal_accumulate_moments (rt_temporal_accumulate_moments_fixed): the same tiles, a lane is a pixel, a kernel of its own so
// that k_temporal_accumulate stays the code it was.  A tap reads, next to what the old kernel reads, the previous frame's
// emission sums (24 bytes of the AOV pixel it has open anyway), one dword of the previous motion buffer and one 16-byte moments
// record.  Every lane runs the pixel up to the spatial estimate (tm_accumulate_moments_front).  If no lane of the workgroup owes
// one -- no pixel of the tile has a history shorter than variance_min_history -- the workgroup is done: nothing was staged.
// Otherwise the workgroup stages the frame's moments and features of its tile and a halo of 2 -- 36 x 12 cells of {f}, {n, z}
// and the hit flag, 13.9 KiB, each cell demodulated ONCE (1.7 per lane instead of 24 per owing lane) -- and the owing lanes take
// their 5 x 5 window from there.  Tap order, skip rule and arithmetic are tm_spatial_variance_of's, which the CPU twin runs on
// global memory: the same bits.  A direct form (a kernel without LDS whose owing lanes read and demodulated their 24 neighbours
// through L1 / L2) was built first and lost at every share of owing pixels, none included; its times are kept in
// profiles/temporal_moments_resources.md and the kernel is gone.
__global__ void __launch_bounds__(kBlock) k_temporal_accumulate_moments(TmMoments tm) {
    __shared__ float4 s_f[kDnLdsH][kDnLdsW], s_nz[kDnLdsH][kDnLdsW];
    __shared__ unsigned char s_hit[kDnLdsH][kDnLdsW];
    const int tile_y = (int)(blockIdx.x / (unsigned)tm.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)tm.tiles_x);
    const int tx = (int)(threadIdx.x % kDnTileW), ty = (int)(threadIdx.x / kDnTileW);
    const int x = tile_x * kDnTileW + tx;
    const long long y = (long long)tile_y * kDnTileH + ty;
    float f[4] = {0.f, 0.f, 0.f, 0.f}, n_p[3] = {0.f, 0.f, 0.f}, z_p = 0.f;
    int32_t n = 1;
    bool owes = false;
    if (x < tm.width && y < tm.height) {
        const float4 m4 = ((const float4 *)tm.motion)[y * tm.width + x];
        const float mo[4] = {m4.x, m4.y, m4.z, m4.w};
        owes = tm_accumulate_moments_front(&tm, x, (int)y, mo, f, n_p, &z_p, &n);
    }
    if (!__syncthreads_or(owes)) return;  // (the same answer in every lane)
    const long long gx0 = (long long)tile_x * kDnTileW - kDnHalo, gy0 = (long long)tile_y * kDnTileH - kDnHalo;
    for (int i = (int)threadIdx.x; i < kDnLdsW * kDnLdsH; i += kBlock) {
        const int cy = i / kDnLdsW, cx = i - cy * kDnLdsW;
        const long long gx = gx0 + cx, gy = gy0 + cy;
        if (gx >= 0 && gx < tm.width && gy >= 0 && gy < tm.height) {  // (a cell outside the image is never read: its tap is skipped)
            float f_q[4], n_q[3], z_q;
            const bool hit = tm_frame_moments(&tm, gy * tm.width + gx, f_q, n_q, &z_q) > 0;
            s_f[cy][cx] = make_float4(f_q[0], f_q[1], f_q[2], f_q[3]);
            s_nz[cy][cx] = make_float4(n_q[0], n_q[1], n_q[2], z_q);
            s_hit[cy][cx] = hit ? 1 : 0;
        }
    }
    __syncthreads();
    if (!owes) return;
    const int cx0 = tx + kDnHalo, cy0 = ty + kDnHalo;  // the pixel's own cell
    tm.variance_out[y * tm.width + x] =
        tm_spatial_variance_of(&tm, x, (int)y, f, n_p, z_p, n, [&](int dx, int dy, long long, float *f_q, float *n_q, float *z_q) {
            const float4 a = s_f[cy0 + dy][cx0 + dx], b = s_nz[cy0 + dy][cx0 + dx];
            f_q[0] = a.x, f_q[1] = a.y, f_q[2] = a.z, f_q[3] = a.w;
            n_q[0] = b.x, n_q[1] = b.y, n_q[2] = b.z, *z_q = b.w;
            return s_hit[cy0 + dy][cx0 + dx] != 0;
        });
}
