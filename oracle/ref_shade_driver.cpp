// ref_shade_driver.cpp -- the reference's OWN shading functions, called one at a time on a table of inputs.
//
// TEST INFRASTRUCTURE (oracle/): own code; nothing here is linked into, or run by, the product.
//
// The reference's device headers are included BY PATH and unmodified, after oracle/ref_shim.h built with
// -DREF_SHIM_REPLAY_RNG: a curandState here replays the uniforms a row supplies, so a row can ask for 2^-33 or 1.0.
// Outputs are written as raw 32-bit patterns.  tests/golden/make_ref_shade_fixture.py makes the input tables
// (tests/shade_scenes.py) and turns the output into tests/golden/ref_shade_fixture.npz; tests/test_ref_shade_pins.py holds
// the oracle's functions to every row.
//
//   ref_shade <in.bin> <out.bin>
//
// in.bin: sections of int32 {function id, rows, words in, words out} followed by rows x words-in 32-bit words;
// out.bin: the same headers, each followed by rows x words-out words.  Row layouts (f = float32, i = int32; a material is
// {albedo f3, ior f, type i}, a light {type i, pos f3, L f3, triangle p0 p1 p2 f9}, `draws` the uniforms consumed):
//    1 Material::sample_f       in  material, wo f3, n f3, u f2                 out f f3, wi f3, n f3, pdf f, draws i
//    2 Material::get_f          in  material, wo f3, wi f3, n f3                out ret i, f f3, pdf f   (f, pdf zero before the call)
//    3 Light::sample_Li         in  light, p f3, u f2                           out ret i, wi f3, Li f3, t f, pdf f, draws i
//    4 Light::pdf_Li            in  light, p f3, wi f3                          out pdf f
//    5 Triangle::sample_p       in  p0 p1 p2 f9, u f2                           out p f3, pdf f, draws i
//    6 Triangle::intersect      in  p0 p1 p2 f9, o f3, d f3, tmax f             out ret i, t f, u f, v f (zero before the call)
//    7 offset_ray_origin        in  p f3, n f3                                  out f3
//    8 power_heuristic          in  f_pdf f, g_pdf f (converted at the call as render.cuh:201,229 convert it)   out f
//    9 same_hemisphere          in  wo f3, wi f3, n f3                          out i
//   10 reflect                  in  v f3, n f3                                  out f3
//   11 refract (4 arguments)    in  v f3, n f3, eta f, cos_theta f              out f3
//   12 uniform_sample_sphere    in  u f2                                        out f3, draws i
//   13 Camera::get_ray          in  camera f12, x f, y f                        out origin f3, unit_d f3
#define REF_SHIM_REPLAY_RNG
#include "ref_shim.h"

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
#include "camera.cuh"

namespace {

union Word {
    float f;
    int32_t i;
    uint32_t u;
};
static_assert(sizeof(Word) == 4, "32-bit words");

Vec3 vec(const Word *w) { return Vec3(w[0].f, w[1].f, w[2].f); }
void put_vec(Word *w, const Vec3 &v) {
    w[0].f = v.x;
    w[1].f = v.y;
    w[2].f = v.z;
}
Material material(const Word *w) {
    switch (w[4].i) {
        case 0: return Material::make_matte(vec(w));
        case 1: return Material::make_mirror(vec(w));
        case 2: return Material::make_glass(w[3].f);
    }
    throw std::runtime_error("material type");
}
Light light(const Word *w, Triangle *tri) {  // 16 words
    *tri = Triangle(vec(w + 7), vec(w + 10), vec(w + 13));
    if (w[0].i == 0) return Light::make_point_light(vec(w + 1), vec(w + 4));
    if (w[0].i == 1) return Light::make_area_light(tri, vec(w + 4));
    throw std::runtime_error("light type");
}
curandState replay(const Word *u, int n) {
    curandState s;
    s.u = &u->f;
    s.pos = 0;
    s.n = n;
    return s;
}

const int kWordsIn[14] = {0, 13, 14, 21, 22, 11, 16, 6, 2, 9, 6, 8, 2, 14};
const int kWordsOut[14] = {0, 11, 5, 10, 1, 5, 4, 3, 1, 1, 3, 3, 4, 6};

void row(int func, const Word *in, Word *out) {
    switch (func) {
        case 1: {
            Material m = material(in);
            Vec3 n = vec(in + 8), wi(0.f);
            float pdf = 0.f;
            curandState rs = replay(in + 11, 2);
            Vec3 f = m.sample_f(vec(in + 5), rs, n, wi, pdf);
            put_vec(out, f);
            put_vec(out + 3, wi);
            put_vec(out + 6, n);
            out[9].f = pdf;
            out[10].i = rs.pos;
            break;
        }
        case 2: {
            Material m = material(in);
            Vec3 f(0.f);
            float pdf = 0.f;
            out[0].i = m.get_f(vec(in + 5), vec(in + 8), vec(in + 11), f, pdf) ? 1 : 0;
            put_vec(out + 1, f);
            out[4].f = pdf;
            break;
        }
        case 3: {
            Triangle tri;
            Light l = light(in, &tri);
            Vec3 wi(0.f), Li(0.f);
            float t = 0.f, pdf = 0.f;
            curandState rs = replay(in + 19, 2);
            out[0].i = l.sample_Li(vec(in + 16), rs, wi, Li, t, pdf) ? 1 : 0;
            put_vec(out + 1, wi);
            put_vec(out + 4, Li);
            out[7].f = t;
            out[8].f = pdf;
            out[9].i = rs.pos;
            break;
        }
        case 4: {
            Triangle tri;
            Light l = light(in, &tri);
            out[0].f = l.pdf_Li(vec(in + 16), vec(in + 19));
            break;
        }
        case 5: {
            Triangle tri(vec(in), vec(in + 3), vec(in + 6));
            float pdf = 0.f;
            curandState rs = replay(in + 9, 2);
            put_vec(out, tri.sample_p(rs, pdf));
            out[3].f = pdf;
            out[4].i = rs.pos;
            break;
        }
        case 6: {
            Triangle tri(vec(in), vec(in + 3), vec(in + 6));
            Ray ray(vec(in + 9), vec(in + 12), in[15].f);
            Intersection is;
            is.t = is.u = is.v = 0.f;
            out[0].i = tri.intersect(ray, is) ? 1 : 0;
            out[1].f = is.t;
            out[2].f = is.u;
            out[3].f = is.v;
            break;
        }
        case 7: put_vec(out, offset_ray_origin(vec(in), vec(in + 3))); break;
        case 8: out[0].f = power_heuristic(in[0].f, in[1].f); break;
        case 9: out[0].i = same_hemisphere(vec(in), vec(in + 3), vec(in + 6)) ? 1 : 0; break;
        case 10: put_vec(out, reflect(vec(in), vec(in + 3))); break;
        case 11: put_vec(out, refract(vec(in), vec(in + 3), in[6].f, in[7].f)); break;
        case 12: {
            curandState rs = replay(in, 2);
            put_vec(out, uniform_sample_sphere(rs));
            out[3].i = rs.pos;
            break;
        }
        case 13: {
            Camera c;
            c.lookfrom = vec(in);
            c.upper_left = vec(in + 3);
            c.horizontal = vec(in + 6);
            c.vertical = vec(in + 9);
            Ray r = c.get_ray(in[12].f, in[13].f);
            put_vec(out, r.origin);
            put_vec(out + 3, r.unit_d);
            break;
        }
        default: throw std::runtime_error("function id");
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <in.bin> <out.bin>\n", argv[0]);
        return 2;
    }
    try {
        FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
        if (!f || !o) throw std::runtime_error("cannot open the files");
        int32_t hd[4];
        while (fread(hd, 4, 4, f) == 4) {
            const int func = hd[0], rows = hd[1];
            if (func < 1 || func > 13 || hd[2] != kWordsIn[func] || hd[3] != kWordsOut[func] || rows < 0)
                throw std::runtime_error("bad section header");
            std::vector<Word> in((size_t)rows * hd[2]), out((size_t)rows * hd[3]);
            if (fread(in.data(), 4, in.size(), f) != in.size()) throw std::runtime_error("short read");
            memset(out.data(), 0, out.size() * 4);
            for (int r = 0; r < rows; r++) row(func, &in[(size_t)r * hd[2]], &out[(size_t)r * hd[3]]);
            if (fwrite(hd, 4, 4, o) != 4 || fwrite(out.data(), 4, out.size(), o) != out.size()) throw std::runtime_error("short write");
        }
        fclose(f);
        fclose(o);
    } catch (const std::exception &e) {
        fprintf(stderr, "ref_shade: %s\n", e.what());
        return 1;
    }
    return 0;
}
