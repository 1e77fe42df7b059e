// rtcuda.hpp -- the reference's host API for the render path, on top of the C-ABI (rtcuda_amd.h).
//
// Same names, constructor signatures and call sequence as lashhw/rtcuda's headers, so its driver
// (main.cu:41-173) compiles against this file with the CUDA allocation calls deleted:
//
//   Vec3 + operators, dot, cross, ...     vec3.cuh:4-147       (everything but the device-only atomic_add)
//   Matrix4x4, Transform                  matrix4x4.hpp, transform.hpp   (included below: rtcuda/matrix4x4.hpp, transform.hpp)
//   PLY ingest                            happly.h (vendored)  -> rtcuda/ply.hpp (own reader, happly's two accessor names)
//   Triangle(p0, p1, p2) + p1() p2() center() bounding_box() p(u, v), members p0 e1 e2 n    triangle.cuh:4-37
//   BoundingBox, Intersection, Ray        bounding_box.cuh:4-37, intersection.hpp:4-6, ray.cuh:4-25
//   Material::make_matte/mirror/glass     material.cuh:25-44
//   Light::make_point_light/area_light    light.cuh:70-84
//   Primitive(tri*, mat*, light* = NULL)  primitive.cuh:6-7
//   Bvh(triangles, primitives)            bvh.cuh:17,30        (asserts equal sizes, :33)
//   Scene{bvh, num_lights, d_lights}      scene.cuh:4-8
//   Camera(lookfrom, lookat, up, vfov, aspect)  camera.cuh:6,15
//   render(w, h, spp, max_bounces, camera, scene, framebuffer)  render.cuh:366-367
//
// Difference by design: the pointers handed to Light / Primitive are HOST pointers into the
// caller's own arrays (the reference hands out device pointers it cudaMalloc'ed and never frees);
// render() flattens them to indices and the library owns every device allocation.
// Errors throw std::runtime_error (the reference prints and exit()s, utility.cuh:6-13).
#ifndef RTCUDA_HPP
#define RTCUDA_HPP

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <cfloat>
#include <stdexcept>
#include <string>
#include <vector>

#include "../rtcuda_amd.h"
#include "matrix4x4.hpp"
#include "ply.hpp"
#include "profiler.hpp"
#include "transform.hpp"

// vec3.cuh:4-147, host side.  Arithmetic forms are the reference's where they round differently from the obvious
// spelling: division by a scalar multiplies by the fp32 reciprocal (vec3.cuh:56-59, :123-129), unit_vector multiplies
// by 1 / length (:131-134), Vec3 / Vec3 is a true per-component divide (:44-46), refract takes its ratio as double.
struct Vec3 {
    Vec3() {}
    constexpr Vec3(float x, float y, float z) : x(x), y(y), z(z) {}
    constexpr Vec3(float xyz) : x(xyz), y(xyz), z(xyz) {}
    static Vec3 make_zeros() { return Vec3(0.f, 0.f, 0.f); }
    static Vec3 make_ones() { return Vec3(1.f, 1.f, 1.f); }

    Vec3 operator-() const { return Vec3(-x, -y, -z); }
    Vec3 &operator+=(const Vec3 &b) { x += b.x; y += b.y; z += b.z; return *this; }
    Vec3 &operator-=(const Vec3 &b) { x -= b.x; y -= b.y; z -= b.z; return *this; }
    Vec3 &operator*=(const Vec3 &b) { x *= b.x; y *= b.y; z *= b.z; return *this; }
    Vec3 &operator/=(const Vec3 &b) { x /= b.x; y /= b.y; z /= b.z; return *this; }
    Vec3 &operator*=(float t) { x *= t; y *= t; z *= t; return *this; }
    Vec3 &operator/=(float t) { return *this *= 1.f / t; }

    float max() const { return fmaxf(fmaxf(x, y), z); }
    float length_squared() const { return x * x + y * y + z * z; }
    float length() const { return sqrtf(length_squared()); }
    Vec3 unit_vector() const { Vec3 r = *this; r.unit_vector_inplace(); return r; }
    void unit_vector_inplace() { *this *= 1.f / length(); }
    void sqrt_inplace() { x = sqrtf(x); y = sqrtf(y); z = sqrtf(z); }

    float x, y, z;
};
inline Vec3 operator+(const Vec3 &a, const Vec3 &b) { return Vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline Vec3 operator-(const Vec3 &a, const Vec3 &b) { return Vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline Vec3 operator*(const Vec3 &a, const Vec3 &b) { return Vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline Vec3 operator/(const Vec3 &a, const Vec3 &b) { return Vec3(a.x / b.x, a.y / b.y, a.z / b.z); }
inline Vec3 operator*(const Vec3 &v, float t) { return Vec3(v.x * t, v.y * t, v.z * t); }
inline Vec3 operator*(float t, const Vec3 &v) { return v * t; }
inline Vec3 operator/(const Vec3 &v, float t) { return v * (1.f / t); }
inline float dot(const Vec3 &a, const Vec3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline Vec3 cross(const Vec3 &a, const Vec3 &b) {
    return Vec3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
inline Vec3 reflect(const Vec3 &v, const Vec3 &unit_n) { return v - 2.f * dot(v, unit_n) * unit_n; }
// vec3.cuh:82-86 (the double ratio narrows to float at the scalar * Vec3 product); :76-80 derives cos_theta itself
inline Vec3 refract(const Vec3 &unit_v, const Vec3 &unit_n, double eta_ratio, float cos_theta) {
    const Vec3 parallel = (float)eta_ratio * (unit_v + cos_theta * unit_n);
    return parallel + -sqrtf(1.f - parallel.length_squared()) * unit_n;
}
inline Vec3 refract(const Vec3 &unit_v, const Vec3 &unit_n, double eta_ratio) {
    return refract(unit_v, unit_n, eta_ratio, (float)(double)-dot(unit_v, unit_n));
}

// bounding_box.cuh:4-37 -- bounds = [xmin, xmax, ymin, ymax, zmin, zmax]
struct BoundingBox {
    BoundingBox() {}
    BoundingBox(float xmin, float xmax, float ymin, float ymax, float zmin, float zmax) {
        const float b[6] = {xmin, xmax, ymin, ymax, zmin, zmax};
        for (int k = 0; k < 6; k++) bounds[k] = b[k];
    }
    static BoundingBox Empty() { BoundingBox b; b.reset(); return b; }
    void reset() {
        for (int a = 0; a < 3; a++) {
            bounds[2 * a] = FLT_MAX;
            bounds[2 * a + 1] = -FLT_MAX;
        }
    }
    void extend(const BoundingBox &other) {
        for (int a = 0; a < 3; a++) {
            bounds[2 * a] = fminf(bounds[2 * a], other.bounds[2 * a]);
            bounds[2 * a + 1] = fmaxf(bounds[2 * a + 1], other.bounds[2 * a + 1]);
        }
    }
    float half_area() const {  // (dx + dy) * dz + dx * dy, in that order (bounding_box.cuh:27-32)
        const float dx = bounds[1] - bounds[0], dy = bounds[3] - bounds[2], dz = bounds[5] - bounds[4];
        return (dx + dy) * dz + dx * dy;
    }
    float bounds[6];
};

// intersection.hpp:4-6
struct Intersection {
    float t, u, v;
};

// utility.cuh:31-47 on the host: the self-intersection offset of a spawned ray's origin (integer steps on the bit
// pattern, or n / 65536 near the coordinate planes).  The device code (rt_device.h) is what renders; this is the same
// function for drivers that spawn rays themselves.
inline Vec3 offset_ray_origin(const Vec3 &p, const Vec3 &n) {
    auto one = [](float pc, float nc) {
        if (fabsf(pc) < 1.f / 32.f) return pc + (1.f / 65536.f) * nc;
        int32_t bits, step = (int32_t)(256.f * nc);
        memcpy(&bits, &pc, 4);
        bits += pc < 0 ? -step : step;
        float r;
        memcpy(&r, &bits, 4);
        return r;
    };
    return Vec3(one(p.x, n.x), one(p.y, n.y), one(p.z, n.z));
}

// ray.cuh:4-25
struct Ray {
    Ray() {}
    Ray(const Vec3 &origin, const Vec3 &unit_d, float tmax = FLT_MAX) : origin(origin), unit_d(unit_d), tmax(tmax) {}
    Vec3 at(float t) const { return origin + t * unit_d; }
    static Ray spawn_offset_ray(const Vec3 &origin, const Vec3 &unit_n, const Vec3 &unit_d, float tmax = FLT_MAX) {
        return Ray(offset_ray_origin(origin, unit_n), unit_d, tmax);
    }
    Vec3 origin, unit_d;
    float tmax;
};

// triangle.cuh:4-37, host side: the reference's public members {p0, e1 = p0 - p1, e2 = p2 - p0, n = e1 x e2} and its
// accessors.  Note p1() = p0 - e1 and p2() = p0 + e2 are the reference's ROUNDED reconstructions, not the constructor's
// arguments; those are kept beside them (p1_, p2_) because the library derives its own e1, e2, n from the three
// vertices with pinned fp32 arithmetic (rt_scene_create), exactly as the reference's constructor does on the host.
struct Triangle {
    Triangle() {}
    Triangle(const Vec3 &p0, const Vec3 &p1, const Vec3 &p2)
        : p0(p0), e1(p0 - p1), e2(p2 - p0), n(cross(e1, e2)), p1_(p1), p2_(p2) {}
    Vec3 p1() const { return p0 - e1; }
    Vec3 p2() const { return p0 + e2; }
    Vec3 center() const { return (p0 + p1() + p2()) * (1.f / 3.f); }
    Vec3 p(float u, float v) const { return p0 - u * e1 + v * e2; }  // triangle.cuh:15
    float area() const { return 0.5f * n.length(); }                 // triangle.cuh:84-86
    BoundingBox bounding_box() const {
        const Vec3 a = p1(), b = p2();
        return BoundingBox(fminf(p0.x, fminf(a.x, b.x)), fmaxf(p0.x, fmaxf(a.x, b.x)), fminf(p0.y, fminf(a.y, b.y)),
                           fmaxf(p0.y, fmaxf(a.y, b.y)), fminf(p0.z, fminf(a.z, b.z)), fmaxf(p0.z, fmaxf(a.z, b.z)));
    }
    Vec3 p0, e1, e2, n;
    Vec3 p1_, p2_;  // the constructor's second and third vertex, as given
};

enum MaterialType { MATTE, MIRROR, GLASS };
struct Material {
    Material() : albedo(0.f), index_of_refraction(0.f), type(MATTE) {}
    static Material make_matte(const Vec3 &albedo) { Material m; m.albedo = albedo; m.type = MATTE; return m; }
    static Material make_mirror(const Vec3 &albedo) { Material m; m.albedo = albedo; m.type = MIRROR; return m; }
    static Material make_glass(float ior) { Material m; m.index_of_refraction = ior; m.type = GLASS; return m; }
    Vec3 albedo;
    float index_of_refraction;
    MaterialType type;
};

enum LightType { POINT_LIGHT, AREA_LIGHT };
struct Light {
    Light() : type(POINT_LIGHT), pos(0.f), d_triangle(nullptr), L(0.f) {}
    static Light make_point_light(const Vec3 &pos, const Vec3 &I) { Light l; l.type = POINT_LIGHT; l.pos = pos; l.L = I; return l; }
    static Light make_area_light(Triangle *d_triangle, const Vec3 &L) { Light l; l.type = AREA_LIGHT; l.d_triangle = d_triangle; l.L = L; return l; }
    LightType type;
    Vec3 pos;
    Triangle *d_triangle;
    Vec3 L;  // I for point lights
};

struct Primitive {
    Primitive() : d_triangle(nullptr), d_mat(nullptr), d_area_light(nullptr) {}
    Primitive(Triangle *d_triangle, Material *d_mat, Light *d_area_light = nullptr)
        : d_triangle(d_triangle), d_mat(d_mat), d_area_light(d_area_light) {}
    Triangle *d_triangle;
    Material *d_mat;
    Light *d_area_light;
};

namespace rtcuda_detail {
struct SceneHandle {
    rt_scene *h = nullptr;
    const Light *lights_key = nullptr;
    int num_lights_key = -1;
    ~SceneHandle() { if (h) rt_scene_destroy(h); }
};
inline void check(int rc, const char *what) {
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + rt_last_error());
}
}  // namespace rtcuda_detail

// Host-side description only; the device BVH is built by the library when render() first sees the scene.
struct Bvh {
    Bvh() : num_primitives(0) {}
    Bvh(const std::vector<Triangle> &triangles, const std::vector<Primitive> &primitives)
        : num_primitives((int)triangles.size()), triangles(triangles), primitives(primitives),
          triangle_base(triangles.empty() ? nullptr : &triangles[0]),
          handle(std::make_shared<rtcuda_detail::SceneHandle>()) {
        assert(triangles.size() == primitives.size());  // bvh.cuh:33
    }
    int num_primitives;
    std::vector<Triangle> triangles;
    std::vector<Primitive> primitives;
    const Triangle *triangle_base;  // primitives[i].d_triangle and Light::d_triangle point into [base, base + n)
    std::shared_ptr<rtcuda_detail::SceneHandle> handle;
};

struct Scene {
    Bvh bvh;
    int num_lights;
    Light *d_lights;
};

struct Camera {
    Camera() {}
    Camera(Vec3 lookfrom, Vec3 lookat, Vec3 up, float vfov, float aspect_ratio) {
        float a[3] = {lookfrom.x, lookfrom.y, lookfrom.z}, b[3] = {lookat.x, lookat.y, lookat.z}, c[3] = {up.x, up.y, up.z};
        rtcuda_detail::check(rt_camera_make(a, b, c, vfov, aspect_ratio, &pod), "Camera");
    }
    rt_camera pod;
};

namespace rtcuda_detail {
// The flat arrays of rt_scene_create from the host description: vertices, per-triangle material and light indices (materials
// numbered in the order the primitives first name them), the material table and the lights.
struct FlatScene {
    std::vector<float> verts;
    std::vector<int32_t> tri_mat, tri_light;
    std::vector<rt_material> mats;
    std::vector<rt_light> lights;
    int n = 0;
};
inline FlatScene flatten(const Scene &scene) {
    FlatScene f;
    const Bvh &bvh = scene.bvh;
    const int n = f.n = bvh.num_primitives;
    f.verts.resize((size_t)9 * (n > 0 ? n : 1));
    f.tri_mat.resize(n > 0 ? n : 1);
    f.tri_light.resize(n > 0 ? n : 1);
    std::vector<float> &verts = f.verts;
    std::vector<int32_t> &tri_mat = f.tri_mat, &tri_light = f.tri_light;
    std::vector<const Material *> mat_ptrs;
    std::vector<rt_material> &mats = f.mats;
    // primitives may come in any order: primitive i describes triangle (d_triangle - base)
    for (int i = 0; i < n; i++) {
        const Primitive &pr = bvh.primitives[i];
        long ti = pr.d_triangle - bvh.triangle_base;
        if (ti < 0 || ti >= n) throw std::runtime_error("render: Primitive::d_triangle does not point into the Bvh's triangles");
        const Triangle &t = bvh.triangles[ti];
        float *q = &verts[9 * (size_t)ti];
        q[0] = t.p0.x; q[1] = t.p0.y; q[2] = t.p0.z;
        q[3] = t.p1_.x; q[4] = t.p1_.y; q[5] = t.p1_.z;
        q[6] = t.p2_.x; q[7] = t.p2_.y; q[8] = t.p2_.z;
        int mi = -1;
        for (size_t k = 0; k < mat_ptrs.size(); k++) if (mat_ptrs[k] == pr.d_mat) { mi = (int)k; break; }
        if (mi < 0) {
            if (!pr.d_mat) throw std::runtime_error("render: Primitive without material");
            mi = (int)mat_ptrs.size();
            mat_ptrs.push_back(pr.d_mat);
            rt_material m;
            m.albedo[0] = pr.d_mat->albedo.x; m.albedo[1] = pr.d_mat->albedo.y; m.albedo[2] = pr.d_mat->albedo.z;
            m.index_of_refraction = pr.d_mat->index_of_refraction;
            m.type = (int32_t)pr.d_mat->type;
            mats.push_back(m);
        }
        tri_mat[ti] = mi;
        long li = pr.d_area_light ? pr.d_area_light - scene.d_lights : -1;
        if (pr.d_area_light && (li < 0 || li >= scene.num_lights)) throw std::runtime_error("render: Primitive::d_area_light does not point into Scene::d_lights");
        tri_light[ti] = (int32_t)li;
    }
    std::vector<rt_light> &lights = f.lights;
    lights.resize(scene.num_lights > 0 ? scene.num_lights : 1);
    for (int k = 0; k < scene.num_lights; k++) {
        const Light &l = scene.d_lights[k];
        rt_light &o = lights[k];
        o.type = (int32_t)l.type;
        o.pos[0] = l.pos.x; o.pos[1] = l.pos.y; o.pos[2] = l.pos.z;
        o.L[0] = l.L.x; o.L[1] = l.L.y; o.L[2] = l.L.z;
        o.triangle = -1;
        if (l.type == AREA_LIGHT) {
            long ti = l.d_triangle - bvh.triangle_base;
            if (ti < 0 || ti >= n) throw std::runtime_error("render: Light::d_triangle does not point into the Bvh's triangles");
            o.triangle = (int32_t)ti;
        }
    }
    return f;
}
inline rt_scene *realise(const Scene &scene) {
    SceneHandle &sh = *scene.bvh.handle;
    if (sh.h && sh.lights_key == scene.d_lights && sh.num_lights_key == scene.num_lights) return sh.h;
    if (sh.h) { rt_scene_destroy(sh.h); sh.h = nullptr; }
    FlatScene f = flatten(scene);
    check(rt_scene_create(f.verts.data(), f.n, f.tri_mat.data(), f.tri_light.data(), f.mats.data(), (int)f.mats.size(),
                          f.lights.data(), scene.num_lights, &sh.h), "rt_scene_create");
    sh.lights_key = scene.d_lights;
    sh.num_lights_key = scene.num_lights;
    return sh.h;
}
}  // namespace rtcuda_detail

// The reference builds and uploads its BVH in the Bvh constructor (bvh.cuh:30-219); here the device scene is created
// the first time a Scene is rendered.  prepare() does it ahead of time, so a driver can time the two apart.
inline void prepare(const Scene &scene) { (void)rtcuda_detail::realise(scene); }

// Moving geometry (no reference counterpart: its Bvh is built once): new positions for the Bvh's triangles, same count and
// order, materials and lights kept.  Bvh::triangles takes them; a scene already realised on the device is refit there
// (rt_scene_update), otherwise the next prepare() / render() simply builds from the new triangles.
inline void update(Scene &scene, const std::vector<Triangle> &triangles) {
    Bvh &bvh = scene.bvh;
    if ((int)triangles.size() != bvh.num_primitives)
        throw std::runtime_error("update: " + std::to_string(triangles.size()) + " triangles, the Bvh holds " + std::to_string(bvh.num_primitives));
    std::copy(triangles.begin(), triangles.end(), bvh.triangles.begin());
    rtcuda_detail::SceneHandle *sh = bvh.handle.get();
    if (!sh || !sh->h) return;
    const int n = bvh.num_primitives;
    std::vector<float> verts((size_t)9 * (n > 0 ? n : 1));
    for (int i = 0; i < n; i++) {
        const Triangle &t = bvh.triangles[(size_t)i];
        float *q = &verts[9 * (size_t)i];
        q[0] = t.p0.x; q[1] = t.p0.y; q[2] = t.p0.z;
        q[3] = t.p1_.x; q[4] = t.p1_.y; q[5] = t.p1_.z;
        q[6] = t.p2_.x; q[7] = t.p2_.y; q[8] = t.p2_.z;
    }
    rtcuda_detail::check(rt_scene_update(sh->h, verts.data(), n), "update");
}

// The same with a new tree: a scene already realised on the device gets a BVH built there by the device builder
// (rt_scene_rebuild) instead of a refit -- for when rt_scene_refit_info's sah_ratio has grown after many update()s.
inline void rebuild(Scene &scene, const std::vector<Triangle> &triangles) {
    Bvh &bvh = scene.bvh;
    if ((int)triangles.size() != bvh.num_primitives)
        throw std::runtime_error("rebuild: " + std::to_string(triangles.size()) + " triangles, the Bvh holds " + std::to_string(bvh.num_primitives));
    std::copy(triangles.begin(), triangles.end(), bvh.triangles.begin());
    rtcuda_detail::SceneHandle *sh = bvh.handle.get();
    if (!sh || !sh->h) return;
    const int n = bvh.num_primitives;
    std::vector<float> verts((size_t)9 * (n > 0 ? n : 1));
    for (int i = 0; i < n; i++) {
        const Triangle &t = bvh.triangles[(size_t)i];
        float *q = &verts[9 * (size_t)i];
        q[0] = t.p0.x; q[1] = t.p0.y; q[2] = t.p0.z;
        q[3] = t.p1_.x; q[4] = t.p1_.y; q[5] = t.p1_.z;
        q[6] = t.p2_.x; q[7] = t.p2_.y; q[8] = t.p2_.z;
    }
    rtcuda_detail::check(rt_scene_rebuild(sh->h, verts.data(), n), "rebuild");
}

// Editing a scene in place (no reference counterpart: its Scene is assembled once) -- rt_scene_set_materials,
// rt_scene_set_lights, rt_scene_set_triangles*, rt_scene_create_device, which document the contract (the bits of a scene
// created anew from the same arrays) and the errors.  The host description is the source: change it, then call the matching
// function; a scene not yet realised on the device simply takes the change when prepare() / render() first builds it.
//
// set_materials: the VALUES of the Materials the primitives point to have changed (which Material a primitive points to is
// part of the triangle set: set_triangles).  The tree is kept.
inline void set_materials(Scene &scene) {
    rtcuda_detail::SceneHandle *sh = scene.bvh.handle.get();
    if (!sh || !sh->h) return;
    rtcuda_detail::FlatScene f = rtcuda_detail::flatten(scene);
    rtcuda_detail::check(rt_scene_set_materials(sh->h, f.mats.data(), (int)f.mats.size()), "set_materials");
}
// set_lights: new lights for the scene (Scene::d_lights / num_lights take them) and the primitives' d_area_light as they
// point into them now.  The tree is kept.
inline void set_lights(Scene &scene, Light *d_lights, int num_lights) {
    scene.d_lights = d_lights;
    scene.num_lights = num_lights;
    rtcuda_detail::SceneHandle *sh = scene.bvh.handle.get();
    if (!sh || !sh->h) return;
    rtcuda_detail::FlatScene f = rtcuda_detail::flatten(scene);
    rtcuda_detail::check(rt_scene_set_lights(sh->h, f.lights.data(), num_lights, f.tri_light.data()), "set_lights");
    sh->lights_key = d_lights;
    sh->num_lights_key = num_lights;
}
// set_triangles: a new Bvh (any number of triangles >= 1) and new lights for it; the device scene, if there is one, is
// kept and takes the new set (the tree is built on the device).
inline void set_triangles(Scene &scene, const std::vector<Triangle> &triangles, const std::vector<Primitive> &primitives,
                          Light *d_lights, int num_lights) {
    std::shared_ptr<rtcuda_detail::SceneHandle> handle = scene.bvh.handle;
    Scene next{Bvh(triangles, primitives), num_lights, d_lights};
    // (the caller's primitives and lights point into the caller's triangle vector: the copy is addressed from its base)
    next.bvh.triangle_base = triangles.empty() ? nullptr : &triangles[0];
    if (handle && handle->h) {
        rtcuda_detail::FlatScene f = rtcuda_detail::flatten(next);
        rtcuda_detail::check(rt_scene_set_triangles(handle->h, f.verts.data(), f.n, f.tri_mat.data(), f.tri_light.data(), f.mats.data(),
                                                    (int)f.mats.size(), f.lights.data(), num_lights), "set_triangles");
        handle->lights_key = d_lights;
        handle->num_lights_key = num_lights;
        next.bvh.handle = handle;
    }
    scene = next;
}
// The device forms take the flat arrays of the C-ABI: the three per-triangle arrays are DEVICE buffers on the scene's device,
// ordered on `stream` (a hipStream_t; nullptr = default stream), materials and lights host arrays.  The Bvh's host triangles
// then no longer describe the device scene (only Bvh::num_primitives follows); a Scene without a Bvh fails with the library's
// message.
inline void set_triangles_device(Scene &scene, const float *d_tri_p0p1p2, int n_tris, const int32_t *d_tri_material,
                                 const int32_t *d_tri_light, const rt_material *materials, int n_materials, const rt_light *lights,
                                 int n_lights, void *stream = nullptr) {
    rt_scene *h = scene.bvh.handle ? rtcuda_detail::realise(scene) : nullptr;
    rtcuda_detail::check(rt_scene_set_triangles_device(h, d_tri_p0p1p2, n_tris, d_tri_material, d_tri_light, materials, n_materials,
                                                       lights, n_lights, stream), "set_triangles_device");
    scene.bvh.num_primitives = n_tris;
}
// A Scene that exists on the device only (rt_scene_create_device): render(), the queries and set_triangles_device take it.
inline Scene create_scene_device(const float *d_tri_p0p1p2, int n_tris, const int32_t *d_tri_material, const int32_t *d_tri_light,
                                 const rt_material *materials, int n_materials, const rt_light *lights, int n_lights,
                                 void *stream = nullptr) {
    Scene scene{};
    scene.bvh.handle = std::make_shared<rtcuda_detail::SceneHandle>();
    rtcuda_detail::check(rt_scene_create_device(d_tri_p0p1p2, n_tris, d_tri_material, d_tri_light, materials, n_materials, lights,
                                                n_lights, stream, &scene.bvh.handle->h), "create_scene_device");
    scene.bvh.num_primitives = n_tris;
    scene.num_lights = n_lights;
    scene.d_lights = nullptr;
    scene.bvh.handle->lights_key = nullptr;
    scene.bvh.handle->num_lights_key = n_lights;
    return scene;
}

// Ray queries (no reference counterpart): n rays from DEVICE buffers on the scene's device, ordered on `stream` (a hipStream_t;
// nullptr = default stream), synchronous on return -- rt_query_closest_device / rt_query_any_device, which document the
// buffers, the flags and the errors.  The scene is realised on the device like prepare() does; a Scene without a Bvh has no
// device scene and fails with the library's message.
inline void query_closest(const Scene &scene, int n, const float *d_origin, const float *d_dir, const float *d_tmax, int32_t *d_hit,
                          float *d_t, float *d_u, float *d_v, void *stream = nullptr, uint32_t flags = 0) {
    rt_scene *h = scene.bvh.handle ? rtcuda_detail::realise(scene) : nullptr;
    rtcuda_detail::check(rt_query_closest_device(h, flags, n, d_origin, d_dir, d_tmax, d_hit, d_t, d_u, d_v, stream), "query_closest");
}
inline void query_any(const Scene &scene, int n, const float *d_origin, const float *d_dir, const float *d_tmax,
                      const int32_t *d_excluded, int32_t *d_occluded, void *stream = nullptr, uint32_t flags = 0) {
    rt_scene *h = scene.bvh.handle ? rtcuda_detail::realise(scene) : nullptr;
    rtcuda_detail::check(rt_query_any_device(h, flags, n, d_origin, d_dir, d_tmax, d_excluded, d_occluded, stream), "query_any");
}

// Radiance along the caller's camera rays (no reference counterpart: its render() makes its rays from its pinhole Camera):
// n_rays rays from DEVICE buffers, raw sums ADDED into d_sum_rgb (n_pixels x 3 floats) or, render_rays_fixed, into int64 sums
// in units of 2^-30 -- rt_render_rays_device / rt_render_rays_fixed_device, which document the frame, the flags and the
// errors.  d_pixel nullptr: ray c lands on pixel c / rays_per_pixel.  Post-processing is the caller's (rt_post_process*).
inline rt_stats render_rays(const Scene &scene, int64_t n_rays, const float *d_origin, const float *d_dir, const int32_t *d_pixel,
                            int rays_per_pixel, int n_pixels, float *d_sum_rgb, int max_bounces = 10, void *stream = nullptr,
                            uint32_t flags = 0, uint64_t seed = 1) {
    rt_scene *h = scene.bvh.handle ? rtcuda_detail::realise(scene) : nullptr;
    rt_stats st{};
    rtcuda_detail::check(rt_render_rays_device(h, n_rays, d_origin, d_dir, d_pixel, rays_per_pixel, n_pixels, max_bounces, seed, flags,
                                               d_sum_rgb, stream, &st), "render_rays");
    return st;
}
inline rt_stats render_rays_fixed(const Scene &scene, int64_t n_rays, const float *d_origin, const float *d_dir, const int32_t *d_pixel,
                                  int rays_per_pixel, int n_pixels, int64_t *d_sum_fixed, int max_bounces = 10, void *stream = nullptr,
                                  uint32_t flags = 0, uint64_t seed = 1) {
    rt_scene *h = scene.bvh.handle ? rtcuda_detail::realise(scene) : nullptr;
    rt_stats st{};
    rtcuda_detail::check(rt_render_rays_fixed_device(h, n_rays, d_origin, d_dir, d_pixel, rays_per_pixel, n_pixels, max_bounces, seed,
                                                     flags, d_sum_fixed, stream, &st), "render_rays_fixed");
    return st;
}

// The same with a stream per ray (rt_render_rays_keyed_device / rt_render_rays_keyed_fixed_device, which document the keys, the
// flags and the errors): row c has the 64-bit key key_first + c * key_stride and the random numbers of camera ray `key` of an
// RT_FLAG_RNG_PER_SAMPLE frame; d_pixel nullptr: it lands on pixel key / rays_per_pixel.  With `fixed`-point sums any split of a
// table -- chunks (key_first = the chunk's first row), rank r of R (key_first = r, key_stride = R) -- adds up to exactly the
// whole frame's.
inline rt_stats render_rays_keyed(const Scene &scene, int64_t n_rays, const float *d_origin, const float *d_dir, const int32_t *d_pixel,
                                  int rays_per_pixel, int n_pixels, float *d_sum_rgb, uint64_t key_first = 0, uint32_t key_stride = 1,
                                  int max_bounces = 10, void *stream = nullptr, uint32_t flags = 0, uint64_t seed = 1) {
    rt_scene *h = scene.bvh.handle ? rtcuda_detail::realise(scene) : nullptr;
    rt_stats st{};
    rtcuda_detail::check(rt_render_rays_keyed_device(h, n_rays, d_origin, d_dir, d_pixel, rays_per_pixel, n_pixels, max_bounces, seed,
                                                     key_first, key_stride, flags, d_sum_rgb, stream, &st), "render_rays_keyed");
    return st;
}
inline rt_stats render_rays_keyed_fixed(const Scene &scene, int64_t n_rays, const float *d_origin, const float *d_dir,
                                        const int32_t *d_pixel, int rays_per_pixel, int n_pixels, int64_t *d_sum_fixed,
                                        uint64_t key_first = 0, uint32_t key_stride = 1, int max_bounces = 10, void *stream = nullptr,
                                        uint32_t flags = 0, uint64_t seed = 1) {
    rt_scene *h = scene.bvh.handle ? rtcuda_detail::realise(scene) : nullptr;
    rt_stats st{};
    rtcuda_detail::check(rt_render_rays_keyed_fixed_device(h, n_rays, d_origin, d_dir, d_pixel, rays_per_pixel, n_pixels, max_bounces,
                                                           seed, key_first, key_stride, flags, d_sum_fixed, stream, &st),
                         "render_rays_keyed_fixed");
    return st;
}

// A sample count per pixel (rt_render_counts_fixed, which documents the samples, the promises, the flags and the errors): pixel p
// renders the samples d_first[p] .. d_first[p] + d_count[p] - 1 (d_first nullptr: from 0) of the RT_FLAG_RNG_PER_SAMPLE frame with
// sample_stride samples per pixel; the int64 sums are ADDED into d_sum_fixed and the counts into d_samples (if given).  Calls whose
// ranges tile [0, sample_stride) add up to exactly the whole frame's sums.
inline rt_stats render_counts(const Scene &scene, const Camera &camera, int width, int height, int sample_stride, const int32_t *d_first,
                              const int32_t *d_count, int64_t *d_sum_fixed, int32_t *d_samples = nullptr, int max_bounces = 10,
                              uint64_t seed = 1, uint32_t flags = 0, void *stream = nullptr) {
    rt_scene *h = scene.bvh.handle ? rtcuda_detail::realise(scene) : nullptr;
    rt_stats st{};
    rtcuda_detail::check(rt_render_counts_fixed(h, &camera.pod, width, height, sample_stride, d_first, d_count, max_bounces, seed, flags,
                                                d_sum_fixed, d_samples, stream, &st), "render_counts");
    return st;
}
// What a counted frame is used with (rt_normalize_counts_fixed / rt_post_process_counts_fixed / rt_sample_allocate, which document
// the arithmetic and the errors): sums over a per-pixel divisor as int64 sums of one sample of the mean (in place allowed), the
// post-processed image with the pixel's own count, and counts from a weight map under a budget (returns the total placed).
inline void normalize_counts(const int64_t *d_sum_fixed, const int32_t *d_samples, int num_pixels, int64_t *d_out_fixed, void *stream = nullptr) {
    rtcuda_detail::check(rt_normalize_counts_fixed(d_sum_fixed, d_samples, num_pixels, d_out_fixed, stream), "normalize_counts");
}
inline void post_process_counts(const int64_t *d_sum_fixed, const int32_t *d_samples, int num_pixels, float *d_rgb_out, void *stream = nullptr) {
    rtcuda_detail::check(rt_post_process_counts_fixed(d_sum_fixed, d_samples, num_pixels, d_rgb_out, stream), "post_process_counts");
}
inline int64_t sample_allocate(const float *d_weight, int num_pixels, int min_count, int max_count, int64_t budget, int32_t *d_count_out,
                               void *stream = nullptr) {
    int64_t total = 0;
    rtcuda_detail::check(rt_sample_allocate(d_weight, num_pixels, min_count, max_count, budget, d_count_out, &total, stream), "sample_allocate");
    return total;
}

// First-hit feature buffers (no reference counterpart): albedo, normal, emission, depth and hit count per pixel as int64
// fixed-point sums ADDED into d_aov_fixed (n_pixels x RT_AOV_CHANNELS), optionally {triangle, material} of every pixel's first
// sample in d_ids (n_pixels x 2) -- rt_render_aov_fixed / rt_render_aov_rays_fixed_device / rt_aov_resolve, which document the
// frame, the channels, the flags and the errors.  render_aov: the camera's own per-sample rays, shard (shard_index,
// shard_count) of them; render_aov_rays: the caller's rays, row c with the key key_first + c * key_stride; aov_resolve: the
// sums as n_pixels x RT_AOV_CHANNELS floats (means over the samples, depth over the hits, coverage).
inline rt_stats render_aov(const Scene &scene, const Camera &camera, int width, int height, int num_samples, int64_t *d_aov_fixed,
                           int32_t *d_ids = nullptr, uint64_t seed = 1, uint32_t flags = 0, int shard_index = 0, int shard_count = 1,
                           void *stream = nullptr) {
    rt_scene *h = scene.bvh.handle ? rtcuda_detail::realise(scene) : nullptr;
    rt_stats st{};
    rtcuda_detail::check(rt_render_aov_fixed(h, &camera.pod, width, height, num_samples, seed, shard_index, shard_count, flags,
                                             d_aov_fixed, d_ids, stream, &st), "render_aov");
    return st;
}
inline rt_stats render_aov_rays(const Scene &scene, int64_t n_rays, const float *d_origin, const float *d_dir, const int32_t *d_pixel,
                                int rays_per_pixel, int n_pixels, int64_t *d_aov_fixed, int32_t *d_ids = nullptr, uint64_t key_first = 0,
                                uint32_t key_stride = 1, uint32_t flags = 0, void *stream = nullptr) {
    rt_scene *h = scene.bvh.handle ? rtcuda_detail::realise(scene) : nullptr;
    rt_stats st{};
    rtcuda_detail::check(rt_render_aov_rays_fixed_device(h, n_rays, d_origin, d_dir, d_pixel, rays_per_pixel, n_pixels, key_first,
                                                         key_stride, flags, d_aov_fixed, d_ids, stream, &st), "render_aov_rays");
    return st;
}
// The same buffers with mirror and glass followed to the first non-specular vertex, for up to max_specular (0 ..
// RT_AOV_FOLLOW_MAX) vertices -- rt_render_aov_follow_fixed / rt_render_aov_follow_rays_fixed_device, which document the followed
// path and the deposit.  max_specular = 0 is render_aov / render_aov_rays.
inline rt_stats render_aov_follow(const Scene &scene, const Camera &camera, int width, int height, int num_samples, int max_specular,
                                  int64_t *d_aov_fixed, int32_t *d_ids = nullptr, uint64_t seed = 1, uint32_t flags = 0,
                                  int shard_index = 0, int shard_count = 1, void *stream = nullptr) {
    rt_scene *h = scene.bvh.handle ? rtcuda_detail::realise(scene) : nullptr;
    rt_stats st{};
    rtcuda_detail::check(rt_render_aov_follow_fixed(h, &camera.pod, width, height, num_samples, seed, shard_index, shard_count, flags,
                                                    max_specular, d_aov_fixed, d_ids, stream, &st), "render_aov_follow");
    return st;
}
inline rt_stats render_aov_follow_rays(const Scene &scene, int64_t n_rays, const float *d_origin, const float *d_dir,
                                       const int32_t *d_pixel, int rays_per_pixel, int n_pixels, int max_specular, int64_t *d_aov_fixed,
                                       int32_t *d_ids = nullptr, uint64_t seed = 1, uint64_t key_first = 0, uint32_t key_stride = 1,
                                       uint32_t flags = 0, void *stream = nullptr) {
    rt_scene *h = scene.bvh.handle ? rtcuda_detail::realise(scene) : nullptr;
    rt_stats st{};
    rtcuda_detail::check(rt_render_aov_follow_rays_fixed_device(h, n_rays, d_origin, d_dir, d_pixel, rays_per_pixel, n_pixels, seed,
                                                                key_first, key_stride, flags, max_specular, d_aov_fixed, d_ids, stream,
                                                                &st), "render_aov_follow_rays");
    return st;
}
inline void aov_resolve(const int64_t *d_aov_fixed, float *d_out, int n_pixels, int num_samples, void *stream = nullptr) {
    rtcuda_detail::check(rt_aov_resolve(d_aov_fixed, d_out, n_pixels, num_samples, stream), "aov_resolve");
}

// The denoiser (rt_denoise_fixed, which documents the filter, the parameters and the errors): fixed-point beauty sums and AOV
// sums of one view, DEVICE buffers -> width * height * 3 floats of linear mean radiance in d_rgb_out.  d_scratch: the caller's,
// denoise_scratch_bytes(width, height) bytes, 16-byte aligned.  params = nullptr: the library's defaults.
inline int64_t denoise_scratch_bytes(int width, int height) {
    const int64_t n = rt_denoise_scratch_bytes(width, height);
    if (n < 0) throw std::runtime_error("denoise_scratch_bytes: bad frame size " + std::to_string(width) + " x " + std::to_string(height));
    return n;
}
inline void denoise(const int64_t *d_sum_fixed, int num_samples, const int64_t *d_aov_fixed, int aov_samples, int width, int height,
                    void *d_scratch, float *d_rgb_out, const rt_denoise_params *params = nullptr, void *stream = nullptr) {
    rtcuda_detail::check(rt_denoise_fixed(d_sum_fixed, num_samples, d_aov_fixed, aov_samples, width, height, params, d_scratch,
                                          d_rgb_out, stream), "denoise");
}

// The dual-buffer denoiser (rt_denoise_dual_fixed, which documents the filter): two half frames of one view -- shards (0, 2) and
// (1, 2) of render_shard_fixed with RT_FLAG_RNG_PER_SAMPLE, each into a zeroed buffer -- and the AOV sums, DEVICE buffers ->
// width * height * 3 floats of linear mean radiance.  d_scratch: denoise_dual_scratch_bytes(width, height) bytes, 16-byte aligned.
inline int64_t denoise_dual_scratch_bytes(int width, int height) {
    const int64_t n = rt_denoise_dual_scratch_bytes(width, height);
    if (n < 0) throw std::runtime_error("denoise_dual_scratch_bytes: bad frame size " + std::to_string(width) + " x " + std::to_string(height));
    return n;
}
inline void denoise_dual(const int64_t *d_sum_a, int samples_a, const int64_t *d_sum_b, int samples_b, const int64_t *d_aov_fixed,
                         int aov_samples, int width, int height, void *d_scratch, float *d_rgb_out,
                         const rt_denoise_dual_params *params = nullptr, void *stream = nullptr) {
    rtcuda_detail::check(rt_denoise_dual_fixed(d_sum_a, samples_a, d_sum_b, samples_b, d_aov_fixed, aov_samples, width, height, params,
                                               d_scratch, d_rgb_out, stream), "denoise_dual");
}

// Temporal accumulation (rt_render_motion / rt_temporal_accumulate_fixed, which document both definitions and the errors).
// render_motion: per pixel where its first hit lay in prev_camera's image one frame ago, {sx, sy, dist, bits of the triangle},
// width * height * 4 floats in d_motion (DEVICE, 16-byte aligned); d_prev_tri_p0p1p2: last frame's vertices (DEVICE, n_tris x 9,
// the caller's order) or nullptr when they did not move.  temporal_accumulate: this frame's sums blended into the reprojected
// history; the outputs are sums of ONE sample of the accumulated mean, which denoise(..., 1, ...) and denoise_dual(..., 1, ..., 1,
// ...) take as they are, and next frame's `in` buffers.  d_sum_b, d_hist_b_in and d_hist_b_out are nullptr together (one buffer);
// the three `in` pointers and d_prev_aov_fixed are nullptr on the first frame.
inline rt_stats render_motion(const Scene &scene, const Camera &camera, int width, int height, const Camera &prev_camera,
                              const float *d_prev_tri_p0p1p2, float *d_motion, uint32_t flags = 0, void *stream = nullptr) {
    rt_scene *h = scene.bvh.handle ? rtcuda_detail::realise(scene) : nullptr;
    rt_stats st{};
    rtcuda_detail::check(rt_render_motion(h, &camera.pod, width, height, &prev_camera.pod, d_prev_tri_p0p1p2, flags, d_motion, stream, &st),
                         "render_motion");
    return st;
}
inline rt_temporal_params temporal_default_params() {
    rt_temporal_params p{};
    rtcuda_detail::check(rt_temporal_default_params(&p), "temporal_default_params");
    return p;
}
inline void temporal_accumulate(const int64_t *d_sum_a, int samples_a, const int64_t *d_sum_b, int samples_b, const int64_t *d_aov_fixed,
                                int aov_samples, const float *d_motion, const int64_t *d_hist_a_in, const int64_t *d_hist_b_in,
                                const int32_t *d_len_in, const int64_t *d_prev_aov_fixed, int prev_aov_samples, int width, int height,
                                int64_t *d_hist_a_out, int64_t *d_hist_b_out, int32_t *d_len_out, const rt_temporal_params *params = nullptr,
                                void *stream = nullptr) {
    rtcuda_detail::check(rt_temporal_accumulate_fixed(d_sum_a, samples_a, d_sum_b, samples_b, d_aov_fixed, aov_samples, d_motion, d_hist_a_in,
                                                      d_hist_b_in, d_len_in, d_prev_aov_fixed, prev_aov_samples, width, height, params,
                                                      d_hist_a_out, d_hist_b_out, d_len_out, stream), "temporal_accumulate");
}

// The single-buffer loop (rt_temporal_accumulate_moments_fixed / rt_denoise_variance_fixed, which document both).
// temporal_accumulate_moments: temporal_accumulate with an emission stop, a triangle stop (d_prev_motion: last frame's motion
// buffer, or nullptr) and, with d_moments_out / d_variance_out, temporally accumulated moments (width * height * 4 floats, 16-byte
// aligned; d_moments_in: last frame's, nullptr on the first frame) and the variance of the mean (width * height floats).
// denoise_variance: denoise_dual's filter on ONE frame's sums and that variance; scratch and params are denoise_dual's.
inline rt_temporal_moments_params temporal_moments_default_params() {
    rt_temporal_moments_params p{};
    rtcuda_detail::check(rt_temporal_moments_default_params(&p), "temporal_moments_default_params");
    return p;
}
inline void temporal_accumulate_moments(const int64_t *d_sum_a, int samples_a, const int64_t *d_sum_b, int samples_b, const int64_t *d_aov_fixed,
                                        int aov_samples, const float *d_motion, const int64_t *d_hist_a_in, const int64_t *d_hist_b_in,
                                        const int32_t *d_len_in, const int64_t *d_prev_aov_fixed, int prev_aov_samples, const float *d_prev_motion,
                                        const float *d_moments_in, int width, int height, int64_t *d_hist_a_out, int64_t *d_hist_b_out,
                                        int32_t *d_len_out, float *d_moments_out, float *d_variance_out,
                                        const rt_temporal_moments_params *params = nullptr, void *stream = nullptr) {
    rtcuda_detail::check(rt_temporal_accumulate_moments_fixed(d_sum_a, samples_a, d_sum_b, samples_b, d_aov_fixed, aov_samples, d_motion,
                                                              d_hist_a_in, d_hist_b_in, d_len_in, d_prev_aov_fixed, prev_aov_samples, d_prev_motion,
                                                              d_moments_in, width, height, params, d_hist_a_out, d_hist_b_out, d_len_out,
                                                              d_moments_out, d_variance_out, stream), "temporal_accumulate_moments");
}
inline void denoise_variance(const int64_t *d_sum_fixed, int num_samples, const float *d_variance, const int64_t *d_aov_fixed, int aov_samples,
                             int width, int height, void *d_scratch, float *d_rgb_out, const rt_denoise_dual_params *params = nullptr,
                             void *stream = nullptr) {
    rtcuda_detail::check(rt_denoise_variance_fixed(d_sum_fixed, num_samples, d_variance, d_aov_fixed, aov_samples, width, height, params,
                                                   d_scratch, d_rgb_out, stream), "denoise_variance");
}

// AOV-guided upsampling (rt_upsample_fixed / rt_upsample_rgb, which document the filter): a low_width x low_height beauty frame
// -- fixed-point sums, or float linear mean radiance -- with its AOV sums, and the AOV sums of the same rt_camera at factor (2, 3
// or 4) times the width and the height, all DEVICE buffers, become the full-size frame: d_rgb_out (3 floats per pixel, linear
// mean radiance) and / or d_out_fixed (3 int64 per pixel, sums of ONE sample: what denoise(..., 1, ...), denoise_variance and the
// accumulators take).  One of the two outputs may be nullptr.  No scratch.  params = nullptr: the library's defaults.
inline rt_upsample_params upsample_default_params() {
    rt_upsample_params p{};
    rtcuda_detail::check(rt_upsample_default_params(&p), "upsample_default_params");
    return p;
}
inline void upsample(const int64_t *d_sum_lo, int num_samples, const int64_t *d_aov_lo, int aov_samples_lo, int low_width, int low_height,
                     int factor, const int64_t *d_aov_hi, int aov_samples_hi, float *d_rgb_out, int64_t *d_out_fixed,
                     const rt_upsample_params *params = nullptr, void *stream = nullptr) {
    rtcuda_detail::check(rt_upsample_fixed(d_sum_lo, num_samples, d_aov_lo, aov_samples_lo, low_width, low_height, factor, d_aov_hi,
                                           aov_samples_hi, params, d_rgb_out, d_out_fixed, stream), "upsample");
}
inline void upsample_rgb(const float *d_rgb_lo, const int64_t *d_aov_lo, int aov_samples_lo, int low_width, int low_height, int factor,
                         const int64_t *d_aov_hi, int aov_samples_hi, float *d_rgb_out, int64_t *d_out_fixed,
                         const rt_upsample_params *params = nullptr, void *stream = nullptr) {
    rtcuda_detail::check(rt_upsample_rgb(d_rgb_lo, d_aov_lo, aov_samples_lo, low_width, low_height, factor, d_aov_hi, aov_samples_hi, params,
                                         d_rgb_out, d_out_fixed, stream), "upsample_rgb");
}

// A driver that must keep the reference's exact call (main.cu:173) can still reach several GPUs: RTCUDA_DEVICES="0,1,2,3" in
// the environment sends the seven-argument render() below through the multi-device path (rt_render_multi).
inline std::vector<int> devices_from_env() {
    std::vector<int> d;
    if (const char *e = std::getenv("RTCUDA_DEVICES")) {
        // a typo must not silently change which GPUs render: anything but non-negative integers separated by
        // single commas is an error, and so is an empty list
        const std::string text(e);
        const char *q = e;
        while (true) {
            char *end = nullptr;
            const long v = std::strtol(q, &end, 10);
            if (end == q || v < 0 || v > 1 << 20 || (*end != ',' && *end != 0))
                throw std::runtime_error("RTCUDA_DEVICES=\"" + text + "\": expected a comma-separated list of device ordinals, e.g. 0,1,2,3");
            d.push_back((int)v);
            if (*end == 0) break;
            q = end + 1;
        }
    }
    return d;
}

// ... and the library's modes: RTCUDA_WATERTIGHT=1 (RT_FLAG_WATERTIGHT: the triangle-list definition of the hits instead of the
// reference's -- no accepted hit lost to a box test, ties by caller index), RTCUDA_REFERENCE_WALK=1 (RT_FLAG_REFERENCE_WALK: every
// ray through the reference's own tree; the same image as the default, several times slower: a cross-check) and
// RTCUDA_DETERMINISTIC=1 (RT_FLAG_DETERMINISTIC: order-independent fixed-point accumulation, bit-reproducible image).
inline uint32_t flags_from_env() {
    uint32_t f = 0;
    if (const char *e = std::getenv("RTCUDA_WATERTIGHT")) f |= std::atoi(e) != 0 ? RT_FLAG_WATERTIGHT : 0u;
    if (const char *e = std::getenv("RTCUDA_REFERENCE_WALK")) f |= std::atoi(e) != 0 ? RT_FLAG_REFERENCE_WALK : 0u;
    if (const char *e = std::getenv("RTCUDA_DETERMINISTIC")) f |= std::atoi(e) != 0 ? RT_FLAG_DETERMINISTIC : 0u;
    return f;
}

// render.cuh:366-367.  `seed` is the reference's hard-coded RAND_SEED = 1 (render.cuh:417).
inline void render(int width, int height, int num_samples, int max_bounces, Camera camera, Scene scene,
                   std::vector<Vec3> &framebuffer, uint64_t seed = 1, rt_stats *stats = nullptr) {
    rt_scene *h = rtcuda_detail::realise(scene);
    framebuffer.resize((size_t)width * height);
    static_assert(sizeof(Vec3) == 12, "Vec3 must be three packed floats");
    const std::vector<int> devices = devices_from_env();
    const uint32_t flags = flags_from_env();
    if (!devices.empty()) {
        rtcuda_detail::check(rt_render_multi(h, &camera.pod, width, height, num_samples, max_bounces, seed, flags, devices.data(),
                                             (int)devices.size(), reinterpret_cast<float *>(framebuffer.data()), stats), "render");
        return;
    }
    rtcuda_detail::check(rt_render(h, &camera.pod, width, height, num_samples, max_bounces, seed, flags,
                                   reinterpret_cast<float *>(framebuffer.data()), stats), "render");
}

// The same call over several GPUs of the node (rt_render_multi): slot-range shards, one host thread per device, the
// shards' sums added on devices[0].  No reference counterpart -- render.cuh:366-367 is one device.  `devices` are HIP device
// ordinals (their number must divide 1048576); `flags`: RT_FLAG_* of rtcuda_amd.h.
inline void render(int width, int height, int num_samples, int max_bounces, Camera camera, Scene scene,
                   std::vector<Vec3> &framebuffer, const std::vector<int> &devices, uint64_t seed = 1, rt_stats *stats = nullptr,
                   uint32_t flags = 0) {
    rt_scene *h = rtcuda_detail::realise(scene);
    framebuffer.resize((size_t)width * height);
    rtcuda_detail::check(rt_render_multi(h, &camera.pod, width, height, num_samples, max_bounces, seed, flags, devices.data(),
                                         (int)devices.size(), reinterpret_cast<float *>(framebuffer.data()), stats), "render");
}

#endif  // RTCUDA_HPP
