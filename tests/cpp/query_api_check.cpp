// Compile-and-link check of the C++ ray-query wrappers (include/rtcuda/rtcuda.hpp: query_closest / query_any) against
// the product library, and their error path without a GPU: a Scene that has no Bvh has no device scene, so the library
// refuses the call ("null scene") before it touches a device, and the wrapper throws with that message.
//   query_api_check            : prints "query_closest=<message>" and "query_any=<message>", exit 0 if both threw
#include <cstdio>
#include <stdexcept>

#include "rtcuda/rtcuda.hpp"

int main() {
    Scene scene{};  // no Bvh, no lights
    int threw = 0;
    float rays[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    int32_t out = 7;
    try {
        query_closest(scene, 1, rays, rays + 3, nullptr, &out, nullptr, nullptr, nullptr);
    } catch (const std::runtime_error &e) {
        printf("query_closest=%s\n", e.what());
        threw++;
    }
    try {
        query_any(scene, 1, rays, rays + 3, nullptr, nullptr, &out, nullptr, RT_FLAG_WATERTIGHT);
    } catch (const std::runtime_error &e) {
        printf("query_any=%s\n", e.what());
        threw++;
    }
    printf("out=%d\n", (int)out);
    return threw == 2 ? 0 : 1;
}
