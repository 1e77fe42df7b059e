// Compile-and-link check of the C++ keyed ray-table render wrappers (include/rtcuda/rtcuda.hpp: render_rays_keyed /
// render_rays_keyed_fixed) against the product library, and their error path without a GPU: a Scene that has no Bvh has no
// device scene, so the library refuses the call ("null scene") before it touches a device, and the wrapper throws with that
// message.
//   render_rays_keyed_api_check : prints "render_rays_keyed=<message>" and "render_rays_keyed_fixed=<message>", exit 0 if
//                                 both threw
#include <cstdio>
#include <stdexcept>

#include "rtcuda/rtcuda.hpp"

int main() {
    Scene scene{};  // no Bvh, no lights
    int threw = 0;
    float rays[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float sum[3] = {7.f, 7.f, 7.f};
    int64_t fixed[3] = {7, 7, 7};
    try {
        render_rays_keyed(scene, 1, rays, rays + 3, nullptr, 1, 1, sum);
    } catch (const std::runtime_error &e) {
        printf("render_rays_keyed=%s\n", e.what());
        threw++;
    }
    try {
        render_rays_keyed_fixed(scene, 1, rays, rays + 3, nullptr, 1, 1, fixed, (1ull << 40) + 5, 8, 5, nullptr, RT_FLAG_RNG_PER_SAMPLE);
    } catch (const std::runtime_error &e) {
        printf("render_rays_keyed_fixed=%s\n", e.what());
        threw++;
    }
    printf("out=%d %d\n", (int)sum[0], (int)fixed[2]);
    return threw == 2 ? 0 : 1;
}
