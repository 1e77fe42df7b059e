// Compile-and-link check of the C++ wrappers of the followed AOVs (include/rtcuda/rtcuda.hpp: render_aov_follow /
// render_aov_follow_rays) against the product library, and their error path without a GPU: a Scene that has no Bvh has no
// device scene, so the library refuses the call ("null scene") before it touches a device, and the wrapper throws with that
// message.
//   aov_follow_api_check : prints "render_aov_follow=<message>", "render_aov_follow_rays=<message>" and the untouched buffers,
//                          exit 0 if both threw
#include <cstdio>
#include <stdexcept>

#include "rtcuda/rtcuda.hpp"

int main() {
    Scene scene{};  // no Bvh, no lights
    Camera camera(Vec3(0.5f, 0.5f, 1.5f), Vec3(0.5f, 0.5f, 0.f), Vec3(0.f, 1.f, 0.f), 37.8f, 1.f);
    int threw = 0;
    float rays[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    int64_t sums[RT_AOV_CHANNELS];
    int32_t ids[2] = {7, 7};
    for (int k = 0; k < RT_AOV_CHANNELS; k++) sums[k] = 7;
    try {
        render_aov_follow(scene, camera, 1, 1, 1, RT_AOV_FOLLOW_MAX, sums, ids, 1, RT_FLAG_WATERTIGHT);
    } catch (const std::runtime_error &e) {
        printf("render_aov_follow=%s\n", e.what());
        threw++;
    }
    try {
        render_aov_follow_rays(scene, 1, rays, rays + 3, nullptr, 1, 1, 2, sums, ids, 9, (1ull << 40) + 5, 8);
    } catch (const std::runtime_error &e) {
        printf("render_aov_follow_rays=%s\n", e.what());
        threw++;
    }
    printf("out=%d %d %d\n", (int)sums[0], (int)sums[RT_AOV_HITS], (int)ids[1]);
    return threw == 2 ? 0 : 1;
}
