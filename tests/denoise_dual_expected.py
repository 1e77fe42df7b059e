"""rt_denoise_dual_fixed in numpy float32, restated from the text of include/rtcuda_amd.h: every intermediate
is a float32 array, so every operation is rounded on its own, in the order the header writes it.  Nothing here reads
rtcuda_amd/csrc/rt_denoise.h.  What the header says "is rt_denoise_fixed's" is imported from tests/denoise_expected.py.
tests/test_denoise_dual_host.py holds the CPU twin (hc_denoise_dual) to this file, tests/test_gpu_denoise_dual.py the kernels."""
import numpy as np

import aov_expected as ae
from denoise_expected import ALBEDO_FLOOR, KERNEL, bits, expnegf, prepare  # noqa: F401  (bits: for the tests)

F32 = np.float32
K3 = (F32(0.25), F32(0.5), F32(0.25))  # k3[dx + 1]
VAR_EPS = F32(2.0 ** -26)


def default_params():
    """What rt_denoise_dual_default_params writes (profiles/denoise_dual_quality.json is where they come from)."""
    return dict(passes=3, sigma_variance=F32(4.0), sigma_depth=F32(0.03125), normal_power_log2=5)


def wrapped_sum(a, b):
    """S = A + B as the two's-complement wrapping add of step 1."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return (a.view(np.uint64) + b.view(np.uint64)).view(np.int64)


def pass_constants(sigma_variance, sigma_depth, spp_a, spp_b):
    """(ks, kz, kv) as the host makes them."""
    with np.errstate(all="ignore"):
        ks = F32(F32(sigma_variance) * F32(sigma_variance))
        kz = F32(F32(1.0) / F32(F32(sigma_depth) * F32(sigma_depth)))
    n = spp_a + spp_b
    kv = F32(float(spp_a) * float(spp_b) / (float(n) * float(n)))
    return ks, kz, kv


def half_u(half, spp, d, e):
    """u_a of step 1: formed like u, from one half's sums and sample count, with the frame's d and e."""
    s = (np.asarray(half, np.int64).reshape(-1, 3).astype(np.float64) * (1.0 / 1073741824.0)).astype(F32)
    c = (s * F32(F32(1.0) / F32(spp))).astype(F32)
    t = (c - e).astype(F32)
    return (np.where(t > 0, t, F32(0)).astype(F32) / d).astype(F32)


def prepare_dual(a, spp_a, b, spp_b, aov, aov_spp, kv):
    """Steps 1 and 2: (u, v, z, normal, d, e)."""
    a, b = np.ascontiguousarray(a, np.int64).reshape(-1, 3), np.ascontiguousarray(b, np.int64).reshape(-1, 3)
    u, z, n, d, e = prepare(wrapped_sum(a, b), spp_a + spp_b, aov, aov_spp)
    df = (half_u(a, spp_a, d, e) - half_u(b, spp_b, d, e)).astype(F32)
    sq = (df * df).astype(F32)
    v = (((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32) * kv).astype(F32)
    return u, v, z, n, d, e


def variance_blur(v, w, h):
    """Step 3a: g, the 3 x 3 prefilter at stride 1."""
    V = v.reshape(h, w)
    sg, sk = np.zeros((h, w), F32), np.zeros((h, w), F32)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            k = F32(K3[dx + 1] * K3[dy + 1])
            sg[P] = (sg[P] + (k * V[Q]).astype(F32)).astype(F32)
            sk[P] = (sk[P] + k).astype(F32)
    return (sg / sk).astype(F32)


def atrous_var_pass(u, v, z, n, w, h, stride, ks, kz, normal_power_log2):
    """Step 3 for one pass: (u (h * w, 3), v (h * w,)) -> the filtered pair, the taps in the header's order."""
    U, V, Z, N = u.reshape(h, w, 3), v.reshape(h, w), z.reshape(h, w), n.reshape(h, w, 3)
    with np.errstate(all="ignore"):
        g = variance_blur(v, w, h)
        r = (F32(1.0) / ((ks * g).astype(F32) + VAR_EPS).astype(F32)).astype(F32)
        sw = np.zeros((h, w), F32)
        sv = np.zeros((h, w), F32)
        su = np.zeros((h, w, 3), F32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = stride * dy, stride * dx
                y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                hk = F32(KERNEL[dx + 2] * KERNEL[dy + 2])
                uq = U[Q]
                if dx == 0 and dy == 0:
                    wt = np.full(uq.shape[:2], hk, F32)
                else:
                    du = (uq - U[P]).astype(F32)
                    sq = (du * du).astype(F32)
                    xv = (((sq[..., 0] + sq[..., 1]).astype(F32) + sq[..., 2]).astype(F32) * r[P]).astype(F32)
                    dz = (Z[Q] - Z[P]).astype(F32)
                    xz = ((dz * dz).astype(F32) * kz).astype(F32)
                    ex = expnegf(-((xv + xz).astype(F32)))
                    pr = (N[P] * N[Q]).astype(F32)
                    dot = ((pr[..., 0] + pr[..., 1]).astype(F32) + pr[..., 2]).astype(F32)
                    wn = np.where(dot > 0, np.where(dot < 1, dot, F32(1)), F32(0)).astype(F32)
                    for _ in range(normal_power_log2):
                        wn = (wn * wn).astype(F32)
                    wt = ((hk * ex).astype(F32) * wn).astype(F32)
                sw[P] = (sw[P] + wt).astype(F32)
                su[P] = (su[P] + (wt[..., None] * uq).astype(F32)).astype(F32)
                sv[P] = (sv[P] + ((wt * wt).astype(F32) * V[Q]).astype(F32)).astype(F32)
        return (su / sw[..., None]).astype(F32).reshape(-1, 3), (sv / (sw * sw).astype(F32)).astype(F32).reshape(-1)


def denoise_dual(a, spp_a, b, spp_b, aov, aov_spp, w, h, passes=None, sigma_variance=None, sigma_depth=None, normal_power_log2=None,
                 with_variance=False):
    """rt_denoise_dual_fixed: (h * w, 3) float32 linear mean radiance (and the final v with ``with_variance``)."""
    dp = default_params()
    passes = dp["passes"] if passes is None else passes
    sigma_variance = dp["sigma_variance"] if sigma_variance is None else sigma_variance
    sigma_depth = dp["sigma_depth"] if sigma_depth is None else sigma_depth
    npow = dp["normal_power_log2"] if normal_power_log2 is None else normal_power_log2
    ks, kz, kv = pass_constants(sigma_variance, sigma_depth, spp_a, spp_b)
    u, v, z, n, d, e = prepare_dual(a, spp_a, b, spp_b, aov, aov_spp, kv)
    assert u.shape[0] == w * h
    for i in range(passes):
        u, v = atrous_var_pass(u, v, z, n, w, h, 1 << i, ks, kz, npow)
    with np.errstate(all="ignore"):
        out = ((u * d).astype(F32) + e).astype(F32)
    return (out, v) if with_variance else out


# ---- inputs the host and the GPU tests share
def split_frame(frame, spp_a, spp_b, seed=5):
    """(a, spp_a, b, spp_b, aov, aov_spp) from a denoise_expected frame: its beauty sums dealt to two halves at random (A gets
    a random share of every sum, B the rest, so A + B is the frame's sum; the frame's fireflies land unevenly in the halves)."""
    beauty, _, aov, aov_spp = frame
    rng = np.random.default_rng(seed + beauty.shape[0])
    share = rng.random(beauty.shape)
    a = np.floor(beauty.astype(np.float64) * share).astype(np.int64)
    b = beauty - a
    return a, spp_a, b, spp_b, aov, aov_spp


def extreme_halves(w, h):
    """Both halves at the edges of the number formats: A is denoise_expected.extreme_frame's beauty (aov_expected.synthetic_sums,
    values over +-2^62), B the same generator at another seed and, on every third pixel, A itself; pixel 0 holds sums of one
    sign beyond 2^62 in both halves, so the add wraps; AOV sums as extreme_frame's.  Unequal sample counts."""
    aov = ae.synthetic_sums(w * h)
    a = ae.synthetic_sums(w * h, seed=29)[:, :3].copy()
    b = ae.synthetic_sums(w * h, seed=31)[:, :3].copy()
    b[::3] = a[::3]
    a[0] = ((1 << 62) + 5, -(1 << 62) - 9, (1 << 62) + (1 << 40))  # (pixel 0: sums of one sign beyond 2^62 in both halves -- the
    b[0] = ((1 << 62) + 77, -(1 << 62) - 3, 1 << 62)               #  add wraps at every frame size)
    return a, 3, b, 1, aov, 7


def flat_aov(n, spp=1):
    """Albedo 1, the normal +z, depth 1, full coverage."""
    one = 1 << 30
    aov = np.zeros((n, ae.CHANNELS), np.int64)
    aov[:, 0:3] = one * spp
    aov[:, 5] = one * spp
    aov[:, 9] = one * spp
    aov[:, 10] = spp
    return aov


def denormal_case(w=9, h=7):
    """(halves, params) whose w * w and v fall in the fp32 denormal range.  One normal, one depth, albedo 2^32 (an albedo sum of
    2^62 at one AOV sample), so u = c * 2^-32: in y half A holds k = 0 .. 3 units of the fixed-point sums and half B none, u_a - u_b =
    k * 2^-62 and v = k^2 * 2^-126, at the bottom of the normal range; a pass multiplies it by (sum of w^2) / (sum of w)^2 < 1:
    denormal from the first pass on, as are the products (w * w) * v_q.  ks * g vanishes against 2^-26, so r = 2^26; u.x
    alternates by 860 * 2^-20 between the pixels of a checkerboard, x_v = (860 * 2^-20)^2 * 2^26 = 45.1: those taps have
    w = h * e^-45.1, about 1e-21, and w * w about 1e-42, a denormal that is not zero."""
    n, one = w * h, 1 << 30
    aov = flat_aov(n)
    aov[:, 0:3] = 1 << 62
    x = np.arange(n) % w
    y = np.arange(n) // w
    a = np.zeros((n, 3), np.int64)
    a[:, 0] = (1 << 58) + ((x + y) % 2) * (860 << 42)
    a[:, 2] = 1 << 60
    b = a.copy()
    a[:, 1] = (x * 5 + y * 3) % 4
    b[:, 1] = 0
    params = dict(passes=2, sigma_variance=F32(1.0), sigma_depth=F32(1.0), normal_power_log2=1)
    return (a, 1, b, 1, aov, 1), params


def firefly_case(w=33, h=17, at=(16, 8)):
    """A flat frame at radiance 2 in both halves (1 sample each), one interior pixel whose A sum is multiplied by 64."""
    n, one = w * h, 1 << 30
    a = np.full((n, 3), 2 * one, np.int64)
    b = a.copy()
    p = at[1] * w + at[0]
    a[p] *= 64
    params = dict(passes=3, sigma_variance=F32(4.0), sigma_depth=F32(0.5), normal_power_log2=1)
    return (a, 1, b, 1, flat_aov(n), 1), params, p
