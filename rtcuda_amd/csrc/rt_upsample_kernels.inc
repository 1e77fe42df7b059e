// rt_upsample_fixed / rt_upsample_rgb on the device (include/rtcuda_amd.h; DESIGN.md section 2.13).  The arithmetic is
// rt_upsample.h's, shared with the CPU twin; here is who walks the pixels and where the low pixels' records live.
//
// k_upsample<F, kRgb>: a workgroup is the denoisers' 32 x 8 tile of FULL pixels, a lane is a pixel.  The low pixels its 256 lanes
// tap are a small rectangle, the tile's footprint: step 3's X0 - 1 of the tile's first column to X0 + 2 of its last one, likewise
// in y.  X0 of two columns that are W - 1 apart differ by at most ceil((W - 1) / F), so the footprint has at most
// ceil(31 / F) + 4 by ceil(7 / F) + 4 cells: 20 x 8, 15 x 7, 12 x 6 for F = 2, 3, 4, never more than a workgroup has lanes.
// Lane i < cells forms cell i's {u, z, n} once (up_low_of_sums / up_low_of_rgb: the three divisions of a low pixel are paid once
// per footprint cell, not once per tap) and leaves it in LDS; after the barrier every lane filters its own pixel from there
// (up_full_pixel) and writes one or both outputs.  The footprint's first low pixel comes from up_position of the tile's first
// full pixel: at F = 3 a tile does not start on a multiple of F.
//
// LDS: seven arrays of one float per cell (4480 bytes at F = 2).  A tap is seven ds_read_b32 of consecutive cells for consecutive
// low pixels -- F neighbouring lanes read the same cell (a broadcast), a row of 32 lanes reads at most 17 consecutive dwords of
// an array, the wave's two rows are its two 32-lane halves: no two lanes of a half meet on a bank at different addresses.
// The staging writes are dword i of each array from lane i.
// Global memory: a lane reads the 88-byte AOV record of its full pixel (the wave two runs of 2816 contiguous bytes) as
// k_dn_finish does, and writes 12 and / or 24 bytes; the footprint's records (24 or 12, and 88 bytes per cell) are read by the
// first lanes, once per tile.
template <int F>
struct UpFootprint {
    static constexpr int kW = (kDnTileW - 1 + F - 1) / F + 4, kH = (kDnTileH - 1 + F - 1) / F + 4;
    static_assert(kW * kH <= kBlock, "one lane forms one cell");
};

template <int F, bool kRgb>
__global__ void __launch_bounds__(kBlock) k_upsample(const void *__restrict__ low, const long long *__restrict__ aov_lo,
                                                      const long long *__restrict__ aov_hi, int low_width, int low_height, int tiles_x,
                                                      float inv_spp, float inv_aov_lo, float inv_aov_hi, float kz, int normal_power_log2,
                                                      float *__restrict__ rgb_out, long long *__restrict__ fixed_out) {
    constexpr int kW = UpFootprint<F>::kW, kH = UpFootprint<F>::kH;
    __shared__ float s_low[UP_LOW_FLOATS][kW * kH];
    const int tile_y = (int)(blockIdx.x / (unsigned)tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)tiles_x);
    const int tx0 = tile_x * kDnTileW, ty0 = tile_y * kDnTileH;
    int fx0, fy0;  // the footprint's first low pixel (-2 or -1 at the frame's edge: those cells stay unwritten and are never read)
    float unused;
    up_position(tx0, F, &fx0, &unused);
    up_position(ty0, F, &fy0, &unused);
    fx0 -= 1, fy0 -= 1;
    const int i = (int)threadIdx.x;
    if (i < kW * kH) {
        const int cy = i / kW, cx = i - cy * kW;
        const int qx = fx0 + cx, qy = fy0 + cy;
        if (qx >= 0 && qx < low_width && qy >= 0 && qy < low_height) {
            const long long q = (long long)qy * low_width + qx;
            UpLow r;
            if (kRgb)
                up_low_of_rgb((const float *)low + 3 * q, (const int64_t *)aov_lo + DN_AOV_CHANNELS * q, inv_aov_lo, &r);
            else
                up_low_of_sums((const int64_t *)low + 3 * q, (const int64_t *)aov_lo + DN_AOV_CHANNELS * q, inv_spp, inv_aov_lo, &r);
            s_low[0][i] = r.u[0], s_low[1][i] = r.u[1], s_low[2][i] = r.u[2], s_low[3][i] = r.z;
            s_low[4][i] = r.n[0], s_low[5][i] = r.n[1], s_low[6][i] = r.n[2];
        }
    }
    __syncthreads();
    const int x = tx0 + (int)(threadIdx.x % kDnTileW), y = ty0 + (int)(threadIdx.x / kDnTileW);
    if (x >= F * low_width || y >= F * low_height) return;
    const long long p = (long long)y * (F * low_width) + x;
    float out[3];
    up_full_pixel(x, y, F, low_width, low_height, (const int64_t *)aov_hi + DN_AOV_CHANNELS * p, inv_aov_hi, kz, normal_power_log2,
                  [&](int qx, int qy, UpLow *q) {
                      const int c = (qy - fy0) * kW + (qx - fx0);
                      q->u[0] = s_low[0][c], q->u[1] = s_low[1][c], q->u[2] = s_low[2][c], q->z = s_low[3][c];
                      q->n[0] = s_low[4][c], q->n[1] = s_low[5][c], q->n[2] = s_low[6][c];
                  },
                  out);
    if (rgb_out)
        for (int k = 0; k < 3; k++) rgb_out[3 * p + k] = out[k];
    if (fixed_out)
        for (int k = 0; k < 3; k++) fixed_out[3 * p + k] = (long long)tm_to_fixed(out[k]);
}
