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
