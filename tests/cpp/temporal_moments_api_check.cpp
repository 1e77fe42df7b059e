// Compile-and-link check of the C++ wrappers of the single-buffer loop (include/rtcuda/rtcuda.hpp: temporal_accumulate_moments /
// temporal_moments_default_params / denoise_variance) against the product library, and their error paths without a GPU: both
// entry points refuse a bad argument before they touch a device, and the wrappers throw with the library's message.  The defaults
// the wrapper returns are the C-ABI's, byte for byte.
//   temporal_moments_api_check : prints "defaults=<the seven fields>", "same_bytes=1", one "<case>=<message>" per refusal and the
//                                untouched outputs, exit 0 if all seven threw
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>

#include "rtcuda/rtcuda.hpp"

int main() {
    int threw = 0;
    int64_t a[3] = {7, 7, 7}, aov[RT_AOV_CHANNELS], out_a[3] = {7, 7, 7};
    int32_t len[1] = {7};
    alignas(16) float motion[4] = {7.f, 7.f, 7.f, 7.f};
    alignas(16) float moments[8] = {7.f, 7.f, 7.f, 7.f, 7.f, 7.f, 7.f, 7.f};
    float variance[1] = {7.f}, rgb[3] = {7.f, 7.f, 7.f};
    alignas(16) unsigned char scratch[64];
    for (int k = 0; k < RT_AOV_CHANNELS; k++) aov[k] = 7;
    const rt_temporal_moments_params prm = temporal_moments_default_params();
    rt_temporal_moments_params raw;
    std::memset(&raw, 0x5a, sizeof raw);
    const int rc = rt_temporal_moments_default_params(&raw);
    printf("defaults=%d %.9g %.9g %.9g %.9g %d %u\n", (int)prm.max_history, prm.alpha_min, prm.depth_tolerance, prm.normal_cos_min,
           prm.emission_tolerance, (int)prm.variance_min_history, (unsigned)prm.flags);
    printf("same_bytes=%d\n", rc == 0 && std::memcmp(&raw, &prm, sizeof raw) == 0 ? 1 : 0);
    auto refuse = [&](const char *name, auto &&call) {
        try {
            call();
        } catch (const std::runtime_error &e) {
            printf("%s=%s\n", name, e.what());
            threw++;
        }
    };
    refuse("null_out", [&] {
        temporal_accumulate_moments(a, 1, nullptr, 0, aov, 1, motion, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 1, 1, out_a, nullptr,
                                    nullptr, moments, variance);
    });
    refuse("moments_without_history", [&] {
        temporal_accumulate_moments(a, 1, nullptr, 0, aov, 1, motion, nullptr, nullptr, nullptr, nullptr, 0, nullptr, moments + 4, 1, 1, out_a, nullptr,
                                    len, moments, variance);
    });
    refuse("misaligned", [&] {
        temporal_accumulate_moments(a, 1, nullptr, 0, aov, 1, motion, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 1, 1, out_a, nullptr, len,
                                    moments + 1, variance);
    });
    refuse("tolerance", [&] {
        rt_temporal_moments_params bad = prm;
        bad.emission_tolerance = std::numeric_limits<float>::quiet_NaN();
        temporal_accumulate_moments(a, 1, nullptr, 0, aov, 1, motion, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 1, 1, out_a, nullptr, len,
                                    moments, variance, &bad);
    });
    refuse("min_history", [&] {
        rt_temporal_moments_params bad = prm;
        bad.variance_min_history = 0;
        temporal_accumulate_moments(a, 1, nullptr, 0, aov, 1, motion, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 1, 1, out_a, nullptr, len,
                                    moments, variance, &bad);
    });
    refuse("overlap", [&] {
        temporal_accumulate_moments(a, 1, nullptr, 0, aov, 1, motion, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 1, 1, out_a, nullptr, len,
                                    moments, motion + 2);
    });
    refuse("denoise_variance", [&] { denoise_variance(a, 1, nullptr, aov, 1, 1, 1, scratch, rgb); });
    printf("out=%d %d %d %d %d %d\n", (int)out_a[0], (int)len[0], (int)motion[2], (int)moments[0], (int)variance[0], (int)rgb[1]);
    return threw == 7 ? 0 : 1;
}
