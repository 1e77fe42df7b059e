// ref_render_driver.cpp -- what the reference's OWN render() computes for a scene given as plain arrays.
//
// TEST INFRASTRUCTURE (oracle/): own code; nothing here is linked into, or run by, the product.
//
// The reference's device headers are included BY PATH and unmodified, after oracle/ref_shim.h (which names every
// substitution it makes); render.cuh is included as the launch-rewritten temporary copy oracle/_ref/render_cpu.h that the
// Makefile target _ref_render writes (kernel<<<G, B>>>(args) -> LAUNCH(kernel, G, B, args); the two jitter draws of gen()
// sequenced x then y).  This driver builds the scene the way the reference's driver does (main.cu:41-166: materials,
// triangles, lights, primitives, Bvh, Scene, Camera -- through the reference's own constructors and make_* functions),
// calls render(), and writes NUMBERS: the raw fp32 sums before post_process_framebuffer, the framebuffer after it, the
// per-iteration (mat, gen, ah, ch) queue counts, the emission / any-hit / closest-hit-shadow deposit counts and the Camera
// the reference's constructor made.  tests/golden/make_ref_render_fixture.py turns them into tests/golden/ref_render_fixture.npz.
//
//   ref_render <scene.bin> <out.bin> [<scene.bin> <out.bin> ...]      (one process: the RNG states are made once per seed)
//
// scene.bin (little endian): int32 {magic 0x52454652, n_tris, n_mats, n_lights, w, h, spp, max_bounces, seed};
//   float32 tris[n_tris][9]; int32 tri_material[n_tris]; int32 tri_light[n_tris] (-1: none);
//   materials[n_mats] {float32 albedo[3], ior; int32 type (0 matte, 1 mirror, 2 glass)};
//   lights[n_lights] {int32 type (0 point, 1 area); float32 pos[3]; int32 tri; float32 L[3]};
//   float32 lookfrom[3], lookat[3], up[3], vfov, aspect.
// out.bin: int32 {magic, w, h, n_iter}; float32 camera[12]; float32 sums[h][w][3]; float32 image[h][w][3];
//   int32 iter[n_iter][4]; int64 {emission_adds, ah_adds, ch_adds}.
#include "ref_shim.h"

// include order of main.cu:18-37 (happly.h, matrix4x4.hpp and transform.hpp serve its mesh loading only)
#include "constant.hpp"
#include "profiler.hpp"
#include "vec3.cuh"
#include "utility.cuh"
#include "ray.cuh"
#include "bounding_box.cuh"
#include "aabb_intersector.cuh"
#include "intersection.hpp"
#include "material.cuh"
#include "triangle.cuh"
#include "device_stack.cuh"
#include "light.cuh"
#include "primitive.cuh"
#include "bvh.cuh"
#include "scene.cuh"
#include "camera.cuh"
#include "render_cpu.h"  // oracle/_ref/render_cpu.h: render.cuh with its launches rewritten

namespace {

struct MaterialRec {
    float albedo[3], ior;
    int32_t type;
};
struct LightRec {
    int32_t type;
    float pos[3];
    int32_t tri;
    float L[3];
};
static_assert(sizeof(MaterialRec) == 20 && sizeof(LightRec) == 32, "record layouts of the scene file");

std::vector<float> g_sums;  // the framebuffer as post_process_framebuffer finds it

void on_launch(const char *kernel) {
    if (strcmp(kernel, "post_process_framebuffer") == 0) {
        g_sums.resize(3 * (size_t)d_width * d_height);
        memcpy(g_sums.data(), d_framebuffer, g_sums.size() * sizeof(float));
    }
}

template <typename T>
void get(FILE *f, T *p, size_t n) {
    if (fread(p, sizeof(T), n, f) != n) throw std::runtime_error("short read");
}
template <typename T>
void put(FILE *f, const T *p, size_t n) {
    if (fwrite(p, sizeof(T), n, f) != n) throw std::runtime_error("short write");
}

void one_frame(const char *in_path, const char *out_path) {
    FILE *f = fopen(in_path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + in_path);
    int32_t hd[9];
    get(f, hd, 9);
    if (hd[0] != 0x52454652) throw std::runtime_error("bad magic");
    const int n_tris = hd[1], n_mats = hd[2], n_lights = hd[3], w = hd[4], h = hd[5], spp = hd[6], max_bounces = hd[7];
    const int seed = hd[8];
    std::vector<float> tris(9 * (size_t)n_tris);
    std::vector<int32_t> tri_material(n_tris), tri_light(n_tris);
    std::vector<MaterialRec> mats(n_mats);
    std::vector<LightRec> lts(n_lights);
    float cam[11];
    get(f, tris.data(), tris.size());
    get(f, tri_material.data(), tri_material.size());
    get(f, tri_light.data(), tri_light.size());
    get(f, mats.data(), mats.size());
    get(f, lts.data(), lts.size());
    get(f, cam, 11);
    fclose(f);

    // main.cu:41-56
    std::vector<Material> materials;
    for (const MaterialRec &m : mats) {
        const Vec3 a(m.albedo[0], m.albedo[1], m.albedo[2]);
        if (m.type == 0) materials.push_back(Material::make_matte(a));
        else if (m.type == 1) materials.push_back(Material::make_mirror(a));
        else if (m.type == 2) materials.push_back(Material::make_glass(m.ior));
        else throw std::runtime_error("material type");
    }
    Material *d_materials;
    CHECK_CUDA(cudaMalloc(&d_materials, (size_t)n_mats * sizeof(Material)));
    CHECK_CUDA(cudaMemcpy(d_materials, materials.data(), (size_t)n_mats * sizeof(Material), cudaMemcpyHostToDevice));
    // main.cu:76-122
    std::vector<Triangle> triangles;
    std::vector<Material *> material_ptrs;
    for (int i = 0; i < n_tris; i++) {
        const float *q = &tris[9 * (size_t)i];
        triangles.emplace_back(Vec3(q[0], q[1], q[2]), Vec3(q[3], q[4], q[5]), Vec3(q[6], q[7], q[8]));
        material_ptrs.push_back(&d_materials[tri_material[i]]);
    }
    Triangle *d_triangles;
    CHECK_CUDA(cudaMalloc(&d_triangles, (size_t)n_tris * sizeof(Triangle)));
    CHECK_CUDA(cudaMemcpy(d_triangles, triangles.data(), (size_t)n_tris * sizeof(Triangle), cudaMemcpyHostToDevice));
    // main.cu:124-138, in the light table's order (the reference's own order is that of an unordered_map)
    std::vector<Light> lights;
    for (int k = 0; k < n_lights; k++) {
        const LightRec &l = lts[k];
        const Vec3 L(l.L[0], l.L[1], l.L[2]);
        if (l.type == 0) {
            // make_point_light leaves Light::d_triangle indeterminate (light.cuh:10,70-76), and mat() hands it to ah() as the
            // triangle a shadow ray may pass through (render.cuh:197): whatever the stack held.  The one defined reading --
            // a point light excludes no triangle -- is set here; without it the count of unoccluded shadow rays depends on
            // the order the lights were made in.
            Light pl = Light::make_point_light(Vec3(l.pos[0], l.pos[1], l.pos[2]), L);
            pl.d_triangle = nullptr;
            lights.push_back(pl);
        } else if (l.type == 1) lights.push_back(Light::make_area_light(&d_triangles[l.tri], L));
        else throw std::runtime_error("light type");
    }
    Light *d_lights;
    CHECK_CUDA(cudaMalloc(&d_lights, (size_t)n_lights * sizeof(Light)));
    CHECK_CUDA(cudaMemcpy(d_lights, lights.data(), (size_t)n_lights * sizeof(Light), cudaMemcpyHostToDevice));
    // main.cu:140-156
    std::vector<Primitive> primitives;
    for (int i = 0; i < n_tris; i++) {
        if (tri_light[i] >= 0) primitives.emplace_back(&d_triangles[i], material_ptrs[i], &d_lights[tri_light[i]]);
        else primitives.emplace_back(&d_triangles[i], material_ptrs[i]);
    }
    Bvh bvh(triangles, primitives);
    Scene scene = {bvh, n_lights, d_lights};
    // main.cu:162-166
    Camera camera(Vec3(cam[0], cam[1], cam[2]), Vec3(cam[3], cam[4], cam[5]), Vec3(cam[6], cam[7], cam[8]), cam[9], cam[10]);

    ref_shim::seed_override() = (uint64_t)seed;
    ref_shim::before_launch() = on_launch;
    ref_shim::select_counts().clear();
    ref_shim::atomic_adds().clear();
    g_sums.clear();
    std::vector<Vec3> framebuffer;
    render(w, h, spp, max_bounces, camera, scene, framebuffer);
    if (g_sums.size() != 3 * (size_t)w * h || framebuffer.size() != (size_t)w * h) throw std::runtime_error("no framebuffer");

    // the select calls of an iteration arrive in the order mat, gen, ah, ch; the last iteration ends after gen
    const std::vector<int> &sel = ref_shim::select_counts();
    if (sel.size() % 4 != 2) throw std::runtime_error("unexpected number of select calls");
    std::vector<int32_t> iter;
    for (size_t i = 0; i < sel.size(); i += 4)
        for (size_t k = 0; k < 4; k++) iter.push_back(i + k < sel.size() ? sel[i + k] : 0);
    auto &adds = ref_shim::atomic_adds();
    const int64_t deposits[3] = {adds["init"] / 3, adds["ah"] / 3, adds["ch"] / 3};
    if (adds["init"] % 3 || adds["ah"] % 3 || adds["ch"] % 3 || adds.size() > 3) throw std::runtime_error("unexpected atomicAdd calls");

    FILE *o = fopen(out_path, "wb");
    if (!o) throw std::runtime_error(std::string("cannot write ") + out_path);
    const int32_t oh[4] = {0x52454652, w, h, (int32_t)(iter.size() / 4)};
    put(o, oh, 4);
    static_assert(sizeof(Camera) == 48 && sizeof(Vec3) == 12, "Camera is 12 floats");
    put(o, (const float *)&camera, 12);
    put(o, g_sums.data(), g_sums.size());
    put(o, (const float *)framebuffer.data(), 3 * framebuffer.size());
    put(o, iter.data(), iter.size());
    put(o, deposits, 3);
    fclose(o);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3 || argc % 2 != 1) {
        fprintf(stderr, "usage: %s <scene.bin> <out.bin> [<scene.bin> <out.bin> ...]\n", argv[0]);
        return 2;
    }
    std::cout.setstate(std::ios_base::failbit);  // (the reference's profiler and BVH builder narrate on stdout)
    try {
        for (int i = 1; i + 1 < argc; i += 2) one_frame(argv[i], argv[i + 1]);
    } catch (const std::exception &e) {
        fprintf(stderr, "ref_render: %s\n", e.what());
        return 1;
    }
    return 0;
}
