// Compile-and-link check of the C++ denoiser wrappers (include/rtcuda/rtcuda.hpp: denoise / denoise_scratch_bytes) against the
// product library, and their error paths without a GPU: the library refuses a null buffer, a bad parameter and a bad size
// before it touches a device, and the wrapper throws with that message.
//   denoise_api_check : prints "scratch=<bytes of a 33 x 17 frame>", "defaults=<passes> <normal_power_log2>", one
//                       "<case>=<message>" per refusal and the untouched output, exit 0 if all four threw
#include <cstdio>
#include <stdexcept>

#include "rtcuda/rtcuda.hpp"

int main() {
    int threw = 0;
    int64_t sums[3] = {7, 7, 7}, aov[RT_AOV_CHANNELS];
    alignas(16) unsigned char scratch[48];
    float out[3] = {7.f, 7.f, 7.f};
    for (int k = 0; k < RT_AOV_CHANNELS; k++) aov[k] = 7;
    printf("scratch=%lld\n", (long long)denoise_scratch_bytes(33, 17));
    rt_denoise_params prm;
    if (rt_denoise_default_params(&prm)) return 2;
    printf("defaults=%d %d\n", (int)prm.passes, (int)prm.normal_power_log2);
    try {
        denoise(sums, 1, aov, 1, 1, 1, scratch, nullptr);
    } catch (const std::runtime_error &e) {
        printf("null_out=%s\n", e.what());
        threw++;
    }
    try {
        rt_denoise_params bad = prm;
        bad.passes = 9;
        denoise(sums, 1, aov, 1, 1, 1, scratch, out, &bad);
    } catch (const std::runtime_error &e) {
        printf("passes=%s\n", e.what());
        threw++;
    }
    try {
        rt_denoise_params bad = prm;
        bad.sigma_depth = 0.f;
        denoise(sums, 1, aov, 1, 1, 1, scratch, out, &bad);
    } catch (const std::runtime_error &e) {
        printf("sigma=%s\n", e.what());
        threw++;
    }
    try {
        denoise_scratch_bytes(0, 4);
    } catch (const std::runtime_error &e) {
        printf("size=%s\n", e.what());
        threw++;
    }
    printf("out=%d %d %d\n", (int)out[0], (int)out[1], (int)out[2]);
    return threw == 4 ? 0 : 1;
}
