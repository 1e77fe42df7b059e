// Compile-and-link check of the C++ wrappers of the upsampler (include/rtcuda/rtcuda.hpp: upsample / upsample_rgb /
// upsample_default_params) against the product library, and their error paths without a GPU: the library refuses a null buffer,
// both outputs null, a bad factor, a bad parameter and a bad sample count before it touches a device, and the wrapper throws with
// that message.
//   upsample_api_check : prints "defaults=<sigma_depth> <normal_power_log2>", one "<case>=<message>" per refusal and the untouched
//                        outputs, exit 0 if all six threw
#include <cstdio>
#include <stdexcept>

#include "rtcuda/rtcuda.hpp"

int main() {
    int threw = 0;
    int64_t sum[3] = {7, 7, 7}, aov_lo[RT_AOV_CHANNELS], aov_hi[4 * RT_AOV_CHANNELS], fixed[12];
    float rgb_lo[3] = {7.f, 7.f, 7.f}, out[12];
    for (int k = 0; k < RT_AOV_CHANNELS; k++) aov_lo[k] = 7;
    for (int k = 0; k < 4 * RT_AOV_CHANNELS; k++) aov_hi[k] = 7;
    for (int k = 0; k < 12; k++) out[k] = 7.f, fixed[k] = 7;
    const rt_upsample_params prm = upsample_default_params();
    printf("defaults=%g %d\n", (double)prm.sigma_depth, (int)prm.normal_power_log2);
    try {
        upsample(sum, 1, aov_lo, 1, 1, 1, 2, nullptr, 1, out, fixed);
    } catch (const std::runtime_error &e) {
        printf("null_aov_hi=%s\n", e.what());
        threw++;
    }
    try {
        upsample(sum, 1, aov_lo, 1, 1, 1, 2, aov_hi, 1, nullptr, nullptr);
    } catch (const std::runtime_error &e) {
        printf("no_output=%s\n", e.what());
        threw++;
    }
    try {
        upsample(sum, 1, aov_lo, 1, 1, 1, 5, aov_hi, 1, out, fixed);
    } catch (const std::runtime_error &e) {
        printf("factor=%s\n", e.what());
        threw++;
    }
    try {
        rt_upsample_params bad = prm;
        bad.sigma_depth = 0.f;
        upsample(sum, 1, aov_lo, 1, 1, 1, 2, aov_hi, 1, out, fixed, &bad);
    } catch (const std::runtime_error &e) {
        printf("sigma=%s\n", e.what());
        threw++;
    }
    try {
        upsample(sum, 0, aov_lo, 1, 1, 1, 2, aov_hi, 1, out, fixed);
    } catch (const std::runtime_error &e) {
        printf("samples=%s\n", e.what());
        threw++;
    }
    try {
        upsample_rgb(nullptr, aov_lo, 1, 1, 1, 2, aov_hi, 1, out, nullptr);
    } catch (const std::runtime_error &e) {
        printf("rgb_null=%s\n", e.what());
        threw++;
    }
    int same = 1;
    for (int k = 0; k < 12; k++) same &= out[k] == 7.f && fixed[k] == 7;
    printf("outputs_untouched=%d rgb_lo=%d\n", same, (int)rgb_lo[0]);
    return threw == 6 && same ? 0 : 1;
}
