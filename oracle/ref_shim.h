// ref_shim.h -- just enough of the CUDA runtime, cuRAND and CUB interfaces, on the CPU, for the reference's device
// headers to compile with g++ and run serially.  TEST INFRASTRUCTURE (oracle/): own code, written from the public
// interfaces; nothing here is linked into, or run by, the product.
//
// A driver includes this header, then the reference's headers BY PATH and unmodified (oracle/Makefile, targets _ref_render
// and _ref_shade; the one exception, the <<< >>> launches of render.cuh, is described there).  What the shim substitutes,
// and therefore what "the reference" means in the fixtures made with it:
//   * cuRAND XORWOW: an own restatement of the published generator (Marsaglia xorwow + Weyl 362437, curand_init's seed
//     scramble, subsequence stride 2^67 as a GF(2) linear map, uniform = x * 2^-32 + 2^-33).  The scramble constants are
//     those of curand_kernel.h as recalled and cannot be verified without a CUDA toolkit.
//   * cub::DeviceSelect::Flagged: a serial stable select.
//   * kernel launches: a serial loop over blocks and threads, in thread-id order; atomicAdd is a plain add.  The order of
//     the float adds into a pixel is therefore queue order, where a GPU's is unspecified.
//   * sincosf and powf(x, 5), in the pinned flavour (the default): rt_sincosf / rt_pow5f of rt_pinned_math.h, this
//     project's stated definition of those two library calls.  -DREF_SHIM_LIBM keeps glibc's.
//   * rounding is g++'s at -O2 -ffp-contract=off (one rounding per operation), not an nvcc binary's contracted FMAs.
// Two hooks serve the drivers and change nothing the reference computes: ref_shim::seed_override (render.cuh:417 fixes the
// seed at 1; a fixture wants two seeds) and ref_shim::before_launch (called with the kernel's name before each launch).
// -DREF_SHIM_REPLAY_RNG (the shade driver): curandState replays a caller-supplied list of uniforms instead.
#ifndef REF_SHIM_H
#define REF_SHIM_H

#include <algorithm>
#include <array>
#include <cassert>
#include <cfloat>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <numeric>
#include <stack>
#include <string>
#include <unordered_map>
#include <vector>

#include "../rtcuda_amd/csrc/rt_pinned_math.h"

#define __host__
#define __device__
#define __global__
#define __constant__

using std::max;
using std::min;

// ---------------------------------------------------------------------------------------------- runtime
typedef int cudaError_t;
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };
struct int3 {
    int x, y, z;
};

namespace ref_shim {
struct Idx {
    unsigned x = 0, y = 0, z = 0;
};
inline uint64_t &seed_override() {  // 0: the caller's seed
    static uint64_t s = 0;
    return s;
}
typedef void (*launch_hook_t)(const char *kernel);
inline launch_hook_t &before_launch() {
    static launch_hook_t h = nullptr;
    return h;
}
inline const char *&current_kernel() {
    static const char *k = "";
    return k;
}
// float atomicAdd calls per kernel name (a Vec3 deposit is three of them)
inline std::unordered_map<std::string, long long> &atomic_adds() {
    static std::unordered_map<std::string, long long> m;
    return m;
}
// number selected by each DeviceSelect::Flagged call that selects, in call order
inline std::vector<int> &select_counts() {
    static std::vector<int> v;
    return v;
}
}  // namespace ref_shim

static ref_shim::Idx blockIdx, blockDim, threadIdx;

template <typename T>
inline cudaError_t cudaMalloc(T **p, size_t n) {
    *p = (T *)calloc(1, n ? n : 1);
    return *p ? 0 : 2;
}
inline cudaError_t cudaFree(void *p) {
    free(p);
    return 0;
}
inline cudaError_t cudaMemcpy(void *dst, const void *src, size_t n, cudaMemcpyKind) {
    memcpy(dst, src, n);
    return 0;
}
inline const char *cudaGetErrorName(cudaError_t e) { return e ? "shim error" : "cudaSuccess"; }
#define cudaMemcpyToSymbol(symbol, src, n) (memcpy((void *)&(symbol), (src), (n)), 0)
#define cudaGetSymbolAddress(pp, symbol) (*(pp) = (void *)&(symbol), 0)

inline float __int_as_float(int i) {
    float f;
    memcpy(&f, &i, 4);
    return f;
}
inline int __float_as_int(float f) {
    int i;
    memcpy(&i, &f, 4);
    return i;
}
inline float atomicAdd(float *address, float val) {
    float old = *address;
    *address = old + val;
    ref_shim::atomic_adds()[ref_shim::current_kernel()]++;
    return old;
}

// kernel<<<G, B>>>(args) -> LAUNCH(kernel, G, B, args): blocks and threads one after the other, in thread-id order
#define LAUNCH(kernel, G, B, ...)                                          \
    do {                                                                   \
        ref_shim::current_kernel() = #kernel;                              \
        if (ref_shim::before_launch()) ref_shim::before_launch()(#kernel); \
        const unsigned g_ = (unsigned)(G), b_ = (unsigned)(B);             \
        blockDim.x = b_;                                                   \
        for (unsigned bi_ = 0; bi_ < g_; bi_++) {                          \
            blockIdx.x = bi_;                                              \
            for (unsigned ti_ = 0; ti_ < b_; ti_++) {                      \
                threadIdx.x = ti_;                                         \
                kernel(__VA_ARGS__);                                       \
            }                                                              \
        }                                                                  \
        ref_shim::current_kernel() = "";                                   \
    } while (0)

// ---------------------------------------------------------------------------------------------- CUB
namespace cub {
struct DeviceSelect {
    // d_temp_storage == NULL: size query.  Otherwise a stable select of the flagged items.
    template <typename In, typename Flag, typename Out, typename Num>
    static cudaError_t Flagged(void *d_temp_storage, size_t &temp_storage_bytes, In d_in, Flag d_flags, Out d_out,
                               Num d_num_selected_out, int num_items) {
        if (!d_temp_storage) {
            temp_storage_bytes = 1;
            return 0;
        }
        int k = 0;
        for (int i = 0; i < num_items; i++)
            if (d_flags[i]) d_out[k++] = d_in[i];
        *d_num_selected_out = k;
        ref_shim::select_counts().push_back(k);
        return 0;
    }
};
}  // namespace cub

// ---------------------------------------------------------------------------------------------- cuRAND
#ifdef REF_SHIM_REPLAY_RNG
struct curandState {  // replays `n` supplied uniforms; `pos` counts the draws made (a draw past the end returns NaN)
    const float *u;
    int pos, n;
};
inline float curand_uniform(curandState *s) {
    float r = s->pos < s->n ? s->u[s->pos] : NAN;
    s->pos++;
    return r;
}
#else
struct curandState {  // the layout of curandStateXORWOW_t: 48 bytes
    unsigned int d, v[5];
    int boxmuller_flag;
    int boxmuller_flag_double;
    float boxmuller_extra;
    double boxmuller_extra_double;
};
static_assert(sizeof(curandState) == 48, "curandStateXORWOW_t is 48 bytes");

namespace ref_shim {
inline void xorwow_linear_step(uint32_t v[5]) {
    uint32_t t = v[0] ^ (v[0] >> 2);
    v[0] = v[1];
    v[1] = v[2];
    v[2] = v[3];
    v[3] = v[4];
    v[4] = (v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1));
}
// the 160 x 160 GF(2) matrix of 2^67 steps (row b = image of basis bit b), as a byte-indexed table
struct Jump {
    uint32_t lut[20][256][5];
    Jump() {
        static uint32_t a[160][5], b[160][5];
        for (int i = 0; i < 160; i++) {
            uint32_t v[5] = {0, 0, 0, 0, 0};
            v[i / 32] = 1u << (i % 32);
            xorwow_linear_step(v);
            memcpy(a[i], v, 20);
        }
        for (int s = 0; s < 67; s++) {  // square 67 times
            for (int i = 0; i < 160; i++) {
                uint32_t r[5] = {0, 0, 0, 0, 0};
                for (int j = 0; j < 160; j++)
                    if (a[i][j / 32] & (1u << (j % 32)))
                        for (int k = 0; k < 5; k++) r[k] ^= a[j][k];
                memcpy(b[i], r, 20);
            }
            memcpy(a, b, sizeof(a));
        }
        for (int byte = 0; byte < 20; byte++)
            for (int val = 0; val < 256; val++) {
                uint32_t r[5] = {0, 0, 0, 0, 0};
                for (int bit = 0; bit < 8; bit++)
                    if (val & (1 << bit))
                        for (int k = 0; k < 5; k++) r[k] ^= a[byte * 8 + bit][k];
                memcpy(lut[byte][val], r, 20);
            }
    }
    void apply(uint32_t v[5]) const {
        uint32_t r[5] = {0, 0, 0, 0, 0};
        for (int w = 0; w < 5; w++)
            for (int by = 0; by < 4; by++) {
                const uint32_t *e = lut[w * 4 + by][(v[w] >> (8 * by)) & 0xff];
                for (int k = 0; k < 5; k++) r[k] ^= e[k];
            }
        memcpy(v, r, 20);
    }
};
// the linear part of the state of (seed, subsequence), memoised per seed: subsequence s is one jump after s - 1
inline const std::array<uint32_t, 5> &initial_v(uint64_t seed, uint64_t subsequence, uint32_t &d) {
    static const Jump *jump = new Jump;
    struct PerSeed {
        uint32_t d;
        std::vector<std::array<uint32_t, 5>> v;
    };
    static std::unordered_map<uint64_t, PerSeed> memo;
    auto it = memo.find(seed);
    if (it == memo.end()) {
        uint32_t s0 = ((uint32_t)seed) ^ 0xaad26b49u;
        uint32_t s1 = ((uint32_t)(seed >> 32)) ^ 0xf7dcefddu;
        uint32_t t0 = 1099087573u * s0;
        uint32_t t1 = 2591861531u * s1;
        PerSeed p;
        p.d = 6615241u + t1 + t0;  // (unchanged by a subsequence jump: 362437 * 2^67 = 0 mod 2^32)
        p.v.push_back({123456789u + t0, 362436069u ^ t0, 521288629u + t1, 88675123u ^ t1, 5783321u + t0});
        it = memo.emplace(seed, std::move(p)).first;
    }
    PerSeed &p = it->second;
    while (p.v.size() <= subsequence) {
        std::array<uint32_t, 5> v = p.v.back();
        jump->apply(v.data());
        p.v.push_back(v);
    }
    d = p.d;
    return p.v[subsequence];
}
}  // namespace ref_shim

inline void curand_init(unsigned long long seed, unsigned long long subsequence, unsigned long long offset, curandState *s) {
    assert(offset == 0);
    if (ref_shim::seed_override()) seed = ref_shim::seed_override();
    memset(s, 0, sizeof(*s));
    uint32_t d;
    const std::array<uint32_t, 5> &v = ref_shim::initial_v(seed, subsequence, d);
    s->d = d;
    memcpy(s->v, v.data(), 20);
}
inline unsigned int curand(curandState *s) {
    uint32_t t = s->v[0] ^ (s->v[0] >> 2);
    s->v[0] = s->v[1];
    s->v[1] = s->v[2];
    s->v[2] = s->v[3];
    s->v[3] = s->v[4];
    s->v[4] = (s->v[4] ^ (s->v[4] << 4)) ^ (t ^ (t << 1));
    s->d += 362437u;
    return s->v[4] + s->d;
}
inline float curand_uniform(curandState *s) { return curand(s) * 2.3283064e-10f + (2.3283064e-10f / 2.0f); }
#endif  // REF_SHIM_REPLAY_RNG

// ---------------------------------------------------------------------------------------------- pinned library calls
#ifndef REF_SHIM_LIBM
namespace ref_shim {
inline float pow_pinned(float x, int n) {
    if (n != 5) {
        fprintf(stderr, "ref_shim: powf(x, %d) has no pinned definition\n", n);
        abort();
    }
    return rt_pow5f(x);
}
}  // namespace ref_shim
#define sincosf(x, s, c) rt_sincosf((x), (s), (c))
#define powf(x, n) ref_shim::pow_pinned((x), (n))
#endif

#endif  // REF_SHIM_H
