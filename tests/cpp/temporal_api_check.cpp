// Compile-and-link check of the C++ wrappers of temporal accumulation (include/rtcuda/rtcuda.hpp: render_motion /
// temporal_accumulate / temporal_default_params) against the product library, and their error paths without a GPU: a Scene that
// has no Bvh has no device scene, so rt_render_motion refuses the call ("null scene"); the accumulator refuses a null buffer, a
// bad parameter, mismatched buffers and an overlap before it touches a device; the wrappers throw with the library's message.
//   temporal_api_check : prints "defaults=<max_history>", one "<case>=<message>" per refusal and the untouched outputs, exit 0 if
//                        all six threw
#include <cstdio>
#include <stdexcept>

#include "rtcuda/rtcuda.hpp"

int main() {
    Scene scene{};  // no Bvh, no lights
    Camera camera(Vec3(0.5f, 0.5f, 1.5f), Vec3(0.5f, 0.5f, 0.f), Vec3(0.f, 1.f, 0.f), 37.8f, 1.f);
    int threw = 0;
    int64_t a[3] = {7, 7, 7}, b[3] = {7, 7, 7}, aov[RT_AOV_CHANNELS], out_a[3] = {7, 7, 7}, out_b[3] = {7, 7, 7};
    int32_t len[1] = {7};
    alignas(16) float motion[4] = {7.f, 7.f, 7.f, 7.f};
    for (int k = 0; k < RT_AOV_CHANNELS; k++) aov[k] = 7;
    const rt_temporal_params prm = temporal_default_params();
    printf("defaults=%d\n", (int)prm.max_history);
    try {
        render_motion(scene, camera, 1, 1, camera, nullptr, motion, RT_FLAG_WATERTIGHT);
    } catch (const std::runtime_error &e) {
        printf("render_motion=%s\n", e.what());
        threw++;
    }
    try {
        temporal_accumulate(a, 1, b, 1, aov, 1, motion, nullptr, nullptr, nullptr, nullptr, 0, 1, 1, out_a, out_b, nullptr);
    } catch (const std::runtime_error &e) {
        printf("null_out=%s\n", e.what());
        threw++;
    }
    try {
        rt_temporal_params bad = prm;
        bad.max_history = 0;
        temporal_accumulate(a, 1, b, 1, aov, 1, motion, nullptr, nullptr, nullptr, nullptr, 0, 1, 1, out_a, out_b, len, &bad);
    } catch (const std::runtime_error &e) {
        printf("max_history=%s\n", e.what());
        threw++;
    }
    try {
        temporal_accumulate(a, 1, nullptr, 0, aov, 1, motion, nullptr, nullptr, nullptr, nullptr, 0, 1, 1, out_a, out_b, len);
    } catch (const std::runtime_error &e) {
        printf("buffers=%s\n", e.what());
        threw++;
    }
    try {
        temporal_accumulate(a, 0, b, 1, aov, 1, motion, nullptr, nullptr, nullptr, nullptr, 0, 1, 1, out_a, out_b, len);
    } catch (const std::runtime_error &e) {
        printf("samples=%s\n", e.what());
        threw++;
    }
    try {
        temporal_accumulate(a, 1, b, 1, aov, 1, motion, nullptr, nullptr, nullptr, nullptr, 0, 1, 1, a, out_b, len);
    } catch (const std::runtime_error &e) {
        printf("overlap=%s\n", e.what());
        threw++;
    }
    printf("out=%d %d %d %d %d\n", (int)out_a[0], (int)out_b[2], (int)len[0], (int)motion[0], (int)a[1]);
    return threw == 6 ? 0 : 1;
}
