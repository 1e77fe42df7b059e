// Compile-and-link check of the C++ scene-edit wrappers (include/rtcuda/rtcuda.hpp: set_materials, set_lights, set_triangles,
// set_triangles_device, create_scene_device) against the product library, and their behaviour without a GPU: on a Scene that
// is not yet realised on the device the host forms only change the host description; the device forms refuse a Scene
// without a Bvh ("null scene") or a null out-pointer before they touch a device, and the wrapper throws the library's message.
//   scene_edit_api_check : prints one "<name>=<result>" line per wrapper, exit 0 if all behaved
#include <cstdio>
#include <stdexcept>

#include "rtcuda/rtcuda.hpp"

int main() {
    int ok = 0;
    std::vector<Triangle> tris{Triangle(Vec3(0.f, 0.f, 0.f), Vec3(1.f, 0.f, 0.f), Vec3(0.f, 1.f, 0.f)),
                               Triangle(Vec3(0.f, 0.f, 1.f), Vec3(1.f, 0.f, 1.f), Vec3(0.f, 1.f, 1.f))};
    Material matte = Material::make_matte(Vec3(0.5f, 0.5f, 0.5f));
    Light lights[2] = {Light::make_point_light(Vec3(0.f, 1.f, 0.f), Vec3(1.f, 1.f, 1.f)), Light::make_area_light(&tris[1], Vec3(2.f, 2.f, 2.f))};
    std::vector<Primitive> prims{Primitive(&tris[0], &matte), Primitive(&tris[1], &matte, &lights[1])};
    Scene scene{Bvh(tris, prims), 1, lights};
    scene.bvh.triangle_base = &tris[0];
    // not realised: the host description follows, nothing reaches the library
    matte.albedo = Vec3(0.1f, 0.2f, 0.3f);
    set_materials(scene);
    set_lights(scene, lights, 2);
    printf("set_lights=%d\n", scene.num_lights);
    ok += scene.num_lights == 2;
    set_triangles(scene, std::vector<Triangle>(tris.begin(), tris.begin() + 1), std::vector<Primitive>(prims.begin(), prims.begin() + 1),
                  lights, 1);
    printf("set_triangles=%d\n", scene.bvh.num_primitives);
    ok += scene.bvh.num_primitives == 1 && scene.num_lights == 1;
    const rtcuda_detail::FlatScene f = rtcuda_detail::flatten(Scene{Bvh(tris, prims), 2, lights});
    (void)f;
    // the device forms: the library's message
    Scene none{};  // no Bvh
    rt_material m{};
    try {
        set_triangles_device(none, nullptr, 1, nullptr, nullptr, &m, 1, nullptr, 0);
    } catch (const std::runtime_error &e) {
        printf("set_triangles_device=%s\n", e.what());
        ok++;
    }
    if (rt_scene_create_device(nullptr, 1, nullptr, nullptr, &m, 1, nullptr, 0, nullptr, nullptr) != 0) {
        printf("create_scene_device=%s\n", rt_last_error());
        ok++;
    }
    Scene (*make)(const float *, int, const int32_t *, const int32_t *, const rt_material *, int, const rt_light *, int, void *) = create_scene_device;
    ok += make != nullptr;
    return ok == 5 ? 0 : 1;
}
