// The temporal accumulator on the device: rt_temporal_accumulate_moments_fixed, and rt_temporal_accumulate_fixed, which is the same
// call with the emission stop, the triangle stop and the moments off (include/rtcuda_amd.h; DESIGN.md sections 2.9 and 2.10).
// The arithmetic is rt_temporal.h's ONE pixel body, shared with the CPU twin (hc_temporal_accumulate_moments); here is who walks
// the pixels: two instantiations of that body over one parameter block, one per entry point.
//
// k_temporal_accumulate_moments: a workgroup is a 32 x 8 tile of pixels, as k_atrous's (kDnTileW x kDnTileH: a wave is two rows of
// 32), a lane is a pixel; the grid is one-dimensional (tiles in row order).  Under a camera that moves by a few pixels the four
// taps of neighbouring lanes fall on neighbouring pixels of the previous frame, so a wave's tap reads runs of a few lines per
// array and all but the first touch of a line is served by L1 / L2.  The taps' footprint is not known before the motion record is
// read, so nothing of the previous frame is staged.  What a lane reads:
//   per pixel  the motion record (one 16-byte load), its colour sums (24 bytes a buffer) and, of the 88 bytes of its AOV pixel,
//              normal, depth and hits; with the emission stop the emission sums as well; with moments what dn_prepare demodulates
//              with
//   per tap    the history length, the previous frame's normal, depth and hits and 24 bytes of history a buffer; with the
//              emission stop the previous frame's emission sums (24 bytes of the AOV pixel it has open anyway); with a previous
//              motion buffer one dword of it; with previous moments one 16-byte record
// With everything off (use_emission 0, prev_motion and the moments pointers null: a uniform branch each) that is what
// k_temporal_accumulate below reads.
// Every lane runs the pixel up to the spatial estimate (tm_accumulate_moments_front).  If no lane of the workgroup owes one -- no
// moments asked for, or no pixel of the tile has a history shorter than variance_min_history -- the workgroup is done: nothing was
// staged.  Otherwise the workgroup stages the frame's moments and features of its tile and a halo of 2 -- 36 x 12 cells of {f},
// {n, z} and the hit flag, 13.9 KiB, each cell demodulated ONCE (1.7 per lane instead of 24 per owing lane) -- and the owing lanes
// take their 5 x 5 window from there.  Tap order, skip rule and arithmetic are tm_spatial_variance_of's, which the CPU twin runs
// on global memory: the same bits.  A direct form (a kernel without LDS whose owing lanes read and demodulated their 24 neighbours
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
        owes = tm_accumulate_moments_front<true>(&tm, x, (int)y, mo, f, n_p, &z_p, &n);
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

// k_temporal_accumulate (rt_temporal_accumulate_fixed): the same tiles and the same body with the three features compiled out, so
// no barrier, no LDS and the registers of the plain blend (eight waves per SIMD).  Timed taking turns, k_temporal_accumulate_moments
// with everything off is as fast on the same buffers, but through tools/temporal_time.py the older entry point's one-buffer call
// was a tenth slower on it than on this (profiles/temporal_one_kernel.md), so the older entry point keeps an instantiation.
__global__ void __launch_bounds__(kBlock) k_temporal_accumulate(TmMoments tm) {
    const int tile_y = (int)(blockIdx.x / (unsigned)tm.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)tm.tiles_x);
    const int x = tile_x * kDnTileW + (int)(threadIdx.x % kDnTileW);
    const long long y = (long long)tile_y * kDnTileH + (int)(threadIdx.x / kDnTileW);
    if (x >= tm.width || y >= tm.height) return;
    const float4 m4 = ((const float4 *)tm.motion)[y * tm.width + x];
    const float mo[4] = {m4.x, m4.y, m4.z, m4.w};
    float f[4], n_p[3], z_p;
    int32_t n;
    (void)tm_accumulate_moments_front<false>(&tm, x, (int)y, mo, f, n_p, &z_p, &n);
}
