// Compile-and-link check of the C++ wrappers of the dual-buffer denoiser (include/rtcuda/rtcuda.hpp: denoise_dual /
// denoise_dual_scratch_bytes) against the product library, and their error paths without a GPU: the library refuses a null
// buffer, a bad parameter, a bad sample count and a bad size before it touches a device, and the wrapper throws with that message.
//   denoise_dual_api_check : prints "scratch=<bytes of a 33 x 17 frame>", "defaults=<passes> <normal_power_log2>", one
//                            "<case>=<message>" per refusal and the untouched output, exit 0 if all five threw
#include <cstdio>
#include <stdexcept>

#include "rtcuda/rtcuda.hpp"

int main() {
    int threw = 0;
    int64_t a[3] = {7, 7, 7}, b[3] = {7, 7, 7}, aov[RT_AOV_CHANNELS];
    alignas(16) unsigned char scratch[64];
    float out[3] = {7.f, 7.f, 7.f};
    for (int k = 0; k < RT_AOV_CHANNELS; k++) aov[k] = 7;
    printf("scratch=%lld\n", (long long)denoise_dual_scratch_bytes(33, 17));
    rt_denoise_dual_params prm;
    if (rt_denoise_dual_default_params(&prm)) return 2;
    printf("defaults=%d %d\n", (int)prm.passes, (int)prm.normal_power_log2);
    try {
        denoise_dual(a, 1, b, 1, aov, 1, 1, 1, scratch, nullptr);
    } catch (const std::runtime_error &e) {
        printf("null_out=%s\n", e.what());
        threw++;
    }
    try {
        rt_denoise_dual_params bad = prm;
        bad.passes = 9;
        denoise_dual(a, 1, b, 1, aov, 1, 1, 1, scratch, out, &bad);
    } catch (const std::runtime_error &e) {
        printf("passes=%s\n", e.what());
        threw++;
    }
    try {
        rt_denoise_dual_params bad = prm;
        bad.sigma_variance = 0.f;
        denoise_dual(a, 1, b, 1, aov, 1, 1, 1, scratch, out, &bad);
    } catch (const std::runtime_error &e) {
        printf("sigma=%s\n", e.what());
        threw++;
    }
    try {
        denoise_dual(a, 1, b, 0, aov, 1, 1, 1, scratch, out);
    } catch (const std::runtime_error &e) {
        printf("samples=%s\n", e.what());
        threw++;
    }
    try {
        denoise_dual_scratch_bytes(0, 4);
    } catch (const std::runtime_error &e) {
        printf("size=%s\n", e.what());
        threw++;
    }
    printf("out=%d %d %d\n", (int)out[0], (int)out[1], (int)out[2]);
    return threw == 5 ? 0 : 1;
}
