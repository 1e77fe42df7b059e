// Compile-and-link check of the C++ wrappers of the counted frames (include/rtcuda/rtcuda.hpp: render_counts / normalize_counts /
// post_process_counts / sample_allocate) against the product library, and their error paths without a GPU: a Scene that has no
// Bvh has no device scene, so the library refuses render_counts ("null scene") before it touches a device; the other three refuse
// a null pointer or a bad budget on the host.  Each wrapper throws with the library's message.
//   render_counts_api_check : prints "<wrapper>=<message>" for each and the untouched buffers, exit 0 if all five threw
#include <cstdio>
#include <stdexcept>

#include "rtcuda/rtcuda.hpp"

int main() {
    Scene scene{};  // no Bvh, no lights
    Camera camera(Vec3(0.5f, 0.5f, 1.5f), Vec3(0.5f, 0.5f, 0.f), Vec3(0.f, 1.f, 0.f), 37.8f, 1.f);
    int threw = 0;
    int32_t count[1] = {1}, samples[1] = {7};
    int64_t sums[3] = {7, 7, 7};
    float weight[1] = {1.f}, rgb[3] = {7.f, 7.f, 7.f};
    try {
        render_counts(scene, camera, 1, 1, 4, nullptr, count, sums, samples, 10, (1ull << 40) + 5, RT_FLAG_WATERTIGHT);
    } catch (const std::runtime_error &e) {
        printf("render_counts=%s\n", e.what());
        threw++;
    }
    try {
        normalize_counts(sums, nullptr, 1, sums);
    } catch (const std::runtime_error &e) {
        printf("normalize_counts=%s\n", e.what());
        threw++;
    }
    try {
        post_process_counts(sums, samples, 1, nullptr);
    } catch (const std::runtime_error &e) {
        printf("post_process_counts=%s\n", e.what());
        threw++;
    }
    try {
        sample_allocate(weight, 1, 2, 4, 1, count);  // budget below num_pixels * min_count
    } catch (const std::runtime_error &e) {
        printf("sample_allocate=%s\n", e.what());
        threw++;
    }
    try {
        sample_allocate(weight, 1, 3, 2, 8, count);  // max_count below min_count
    } catch (const std::runtime_error &e) {
        printf("sample_allocate=%s\n", e.what());
        threw++;
    }
    printf("out=%d %d %d %d\n", (int)sums[0], (int)samples[0], (int)count[0], (int)rgb[0]);
    return threw == 5 ? 0 : 1;
}
