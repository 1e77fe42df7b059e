"""rt_denoise_fixed in numpy float32, restated from the text of include/rtcuda_amd.h: every intermediate
is a float32 array, so every operation is rounded on its own, in the order the header writes it.  Nothing here reads
rtcuda_amd/csrc/rt_denoise.h.  tests/test_denoise_host.py holds the CPU twin (hc_denoise) to this file, tests/test_gpu_denoise.py
the kernels."""
import numpy as np

import aov_expected as ae

F32 = np.float32
KERNEL = (F32(0.0625), F32(0.25), F32(0.375), F32(0.25), F32(0.0625))  # k[dx + 2]
EXP_CUTOFF = F32(-87.0)
ALBEDO_FLOOR = F32(2.0 ** -10)
MAX_PASSES = 8
MAX_NORMAL_POWER_LOG2 = 8


def expnegf(x):
    """rt_expnegf: 0 for x <= -87 and NaN; else k = floor(x * log2e + 0.5), r = (x - k * C1) - k * C2, the degree-5 polynomial
    in Horner form, ((p * r^2) + r) + 1, times 2^k from its bits."""
    x = np.asarray(x, np.float32)
    live = x > EXP_CUTOFF
    xs = np.where(live, x, F32(0))
    kf = np.floor((xs * F32(1.44269504)).astype(F32) + F32(0.5)).astype(F32)
    r = (xs - (kf * F32(0.693359375)).astype(F32)).astype(F32)
    r = (r - (kf * F32(-2.12194440e-4)).astype(F32)).astype(F32)
    r2 = (r * r).astype(F32)
    p = np.full(x.shape, F32(1.9875691500e-4), F32)
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = ((p * r).astype(F32) + F32(c)).astype(F32)
    y = (((p * r2).astype(F32) + r).astype(F32) + F32(1)).astype(F32)
    scale = ((kf.astype(np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(F32)
    return np.where(live, (y * scale).astype(F32), F32(0)).astype(F32)


def default_params():
    """What rt_denoise_default_params writes (profiles/denoise_quality.json is where they come from)."""
    return dict(passes=2, sigma_color=F32(0.125), sigma_depth=F32(0.5), normal_power_log2=1)


def pass_constants(passes, sigma_color, sigma_depth):
    """(kc_i for i < passes, kz) as the host makes them, in float32."""
    sc2 = F32(F32(sigma_color) * F32(sigma_color))
    sd2 = F32(F32(sigma_depth) * F32(sigma_depth))
    with np.errstate(all="ignore"):
        kc = [F32(F32(4.0 ** i) / sc2) for i in range(passes)]
        kz = F32(F32(1.0) / sd2)
    return kc, kz


def prepare(beauty, spp, aov, aov_spp):
    """Steps 1 and 2: (u (n, 3), z (n,), normal (n, 3), d (n, 3), e (n, 3)) of the int64 sums."""
    beauty = np.asarray(beauty, np.int64).reshape(-1, 3)
    s = (beauty.astype(np.float64) * (1.0 / 1073741824.0)).astype(F32)
    c = (s * F32(F32(1.0) / F32(spp))).astype(F32)
    f = ae.resolve(np.asarray(aov, np.int64).reshape(-1, ae.CHANNELS), aov_spp)
    a, n, e, z = f[:, ae.ALBEDO:ae.ALBEDO + 3], f[:, ae.NORMAL:ae.NORMAL + 3], f[:, ae.EMISSION:ae.EMISSION + 3], f[:, ae.DEPTH]
    d = np.where(a > ALBEDO_FLOOR, a, ALBEDO_FLOOR).astype(F32)
    t = (c - e).astype(F32)
    u = (np.where(t > 0, t, F32(0)).astype(F32) / d).astype(F32)
    return u, z.astype(F32).copy(), n.astype(F32).copy(), d, e.astype(F32).copy()


def atrous_pass(u, z, n, w, h, stride, kc, kz, normal_power_log2):
    """Step 3 for one pass: u (h * w, 3) -> the filtered u, all pixels at once, the taps in the header's order."""
    U, Z, N = u.reshape(h, w, 3), z.reshape(h, w), n.reshape(h, w, 3)
    sw = np.zeros((h, w), F32)
    su = np.zeros((h, w, 3), F32)
    with np.errstate(all="ignore"):
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
                    xc = (((sq[..., 0] + sq[..., 1]).astype(F32) + sq[..., 2]).astype(F32) * kc).astype(F32)
                    dz = (Z[Q] - Z[P]).astype(F32)
                    xz = ((dz * dz).astype(F32) * kz).astype(F32)
                    ex = expnegf(-((xc + xz).astype(F32)))
                    pr = (N[P] * N[Q]).astype(F32)
                    dot = ((pr[..., 0] + pr[..., 1]).astype(F32) + pr[..., 2]).astype(F32)
                    wn = np.where(dot > 0, np.where(dot < 1, dot, F32(1)), F32(0)).astype(F32)
                    for _ in range(normal_power_log2):
                        wn = (wn * wn).astype(F32)
                    wt = ((hk * ex).astype(F32) * wn).astype(F32)
                sw[P] = (sw[P] + wt).astype(F32)
                su[P] = (su[P] + (wt[..., None] * uq).astype(F32)).astype(F32)
        return (su / sw[..., None]).astype(F32).reshape(-1, 3)


def denoise(beauty, spp, aov, aov_spp, w, h, passes=None, sigma_color=None, sigma_depth=None, normal_power_log2=None):
    """rt_denoise_fixed: (h * w, 3) float32 linear mean radiance."""
    dp = default_params()
    passes = dp["passes"] if passes is None else passes
    sigma_color = dp["sigma_color"] if sigma_color is None else sigma_color
    sigma_depth = dp["sigma_depth"] if sigma_depth is None else sigma_depth
    npow = dp["normal_power_log2"] if normal_power_log2 is None else normal_power_log2
    u, z, n, d, e = prepare(beauty, spp, aov, aov_spp)
    assert u.shape[0] == w * h
    kc, kz = pass_constants(passes, sigma_color, sigma_depth)
    for i in range(passes):
        u = atrous_pass(u, z, n, w, h, 1 << i, kc[i], kz, npow)
    with np.errstate(all="ignore"):
        return ((u * d).astype(F32) + e).astype(F32)


def noisy_mean(beauty, spp):
    """The undenoised linear mean of fixed-point beauty sums, as step 1 forms it."""
    s = (np.asarray(beauty, np.int64).reshape(-1, 3).astype(np.float64) * (1.0 / 1073741824.0)).astype(F32)
    return (s * F32(F32(1.0) / F32(spp))).astype(F32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- inputs the host and the GPU tests share
def synthetic_frame(w, h, seed=3):
    """Bounded random sums with structure: (beauty (n, 3), spp, aov (n, 11), aov_spp).  Albedo in (0, 1], unit-ish normals of a
    few directions, depths in steps, a band of misses, a band of partial coverage, some emission."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    n, spp = w * h, 4
    one = 1 << 30
    aov = np.zeros((n, ae.CHANNELS), np.int64)
    hits = np.full(n, spp, np.int64)
    hits[rng.random(n) < 0.15] = 0
    part = rng.random(n) < 0.15
    hits[part] = rng.integers(1, spp, part.sum())
    alb = rng.integers(0, one + 1, (n, 3))
    alb[rng.random(n) < 0.1] = 0  # (black albedo: the 2^-10 floor)
    dirs = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0, 0.8], [0, -0.6, 0.8]], np.float64)
    nn = dirs[rng.integers(0, len(dirs), n)] * np.where(rng.random(n) < 0.2, -1.0, 1.0)[:, None]
    depth = rng.integers(1, 6, n) * (one // 4) + rng.integers(0, one // 64, n)
    em = np.where(rng.random(n) < 0.1, 1, 0)[:, None] * rng.integers(0, 4 * one, (n, 3))
    aov[:, 0:3] = alb * hits[:, None]
    aov[:, 3:6] = np.rint(nn * one).astype(np.int64) * hits[:, None]
    aov[:, 6:9] = em * hits[:, None]
    aov[:, 9] = depth * hits
    aov[:, 10] = hits
    beauty = rng.integers(0, 3 * one, (n, 3)) * spp
    beauty[rng.random(n) < 0.02] *= 64  # fireflies
    return beauty.astype(np.int64), spp, aov, spp


def extreme_frame(w, h):
    """Sums at the edges of the number formats, after aov_expected.synthetic_sums: values over +-2^62, hits of every kind
    (0, more than the samples, negative), beauty likewise."""
    aov = ae.synthetic_sums(w * h)
    beauty = ae.synthetic_sums(w * h, seed=29)[:, :3].copy()
    return beauty, 3, aov, 7


def denormal_case(w=9, h=7):
    """(frame, params) whose tap weights fall in the fp32 denormal range: constant albedo 1, one normal, one depth, and u in
    steps of 9.3 such that x_c = (delta u)^2 * kc is about 86.5 for the four direct neighbours: exp gives about 2.7e-38, the
    kernel weight 3/32 takes it below FLT_MIN = 1.18e-38 (DENORMAL_TAP is that tap, for the tests to check the claim)."""
    n, one = w * h, 1 << 30
    aov = np.zeros((n, ae.CHANNELS), np.int64)
    aov[:, 0:3] = one
    aov[:, 5] = one
    aov[:, 9] = one
    aov[:, 10] = 1
    x = np.arange(n) % w
    y = np.arange(n) // w
    beauty = np.zeros((n, 3), np.int64)
    beauty[:, 0] = (x + y) * int(9.3 * one)   # neighbours differ by 9.3 or 18.6 in u.x
    beauty[:, 1] = ((x * 3 + y) % 2) * (one // 2)
    beauty[:, 2] = one
    params = dict(passes=2, sigma_color=F32(1.0), sigma_depth=F32(1.0), normal_power_log2=1)
    return (beauty, 1, aov, 1), params


# ---- real frames, from the oracle alone (one per session and argument tuple)
_frame_cache = {}
REFERENCE_SPP, REFERENCE_SEED = 1024, 2
REAL_FRAME = (64, 48, 4)


def oracle_beauty(oracle, osc, cam12, w, h, spp, seed=1):
    """(h * w, 3) int64: the fixed-point sums of the per-sample frame (what rt_render_shard_fixed leaves with
    RT_FLAG_RNG_PER_SAMPLE)."""
    from oracle.oracle import usable_cpus
    key = ("beauty", oracle.flavour, id(osc), tuple(np.asarray(cam12).tolist()), w, h, spp, seed)
    if key not in _frame_cache:
        fixed = np.zeros((h, w, 3), np.int64)
        osc.render(cam12, w, h, spp, seed=seed, threads=usable_cpus(), fixed_out=fixed, rng_mode="per_sample")
        _frame_cache[key] = fixed.reshape(-1, 3)
    return _frame_cache[key]


def real_frame(oracle, osc, cam12, w, h, spp):
    """(beauty, spp, aov, spp) of the view, both from the CPU: the oracle's per-sample frame and aov_expected.frame_expected."""
    key = ("aov", oracle.flavour, id(osc), tuple(np.asarray(cam12).tolist()), w, h, spp)
    if key not in _frame_cache:
        _frame_cache[key] = ae.frame_expected(oracle, osc, cam12, w, h, spp)[0]
    return oracle_beauty(oracle, osc, cam12, w, h, spp), spp, _frame_cache[key], spp


def reference_mean(oracle, osc, cam12, w, h):
    """(h * w, 3) float64: the linear mean radiance of the view at 1024 spp (another seed than the noisy frames')."""
    return oracle_beauty(oracle, osc, cam12, w, h, REFERENCE_SPP, REFERENCE_SEED).astype(np.float64) * (2.0 ** -30 / REFERENCE_SPP)


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def noise_free_frame(aov, aov_spp):
    """A frame without noise on the features of a real one: beauty = 2 * albedo (2 * 2^-10 in the channels whose mean albedo
    is not above the floor), the emission channels of the AOV copy zeroed.  Then u is exactly 2 in every channel of every
    pixel.  Returns (beauty, aov_spp, aov copy, aov_spp)."""
    aov = np.array(aov, np.int64, copy=True)
    aov[:, ae.EMISSION:ae.EMISSION + 3] = 0
    a = ae.resolve(aov, aov_spp)[:, ae.ALBEDO:ae.ALBEDO + 3]
    floor_sum = (1 << 20) * aov_spp  # 2^-10 per sample, in units of 2^-30
    beauty = 2 * np.where(a > ALBEDO_FLOOR, aov[:, ae.ALBEDO:ae.ALBEDO + 3], floor_sum)
    return beauty.astype(np.int64), aov_spp, aov, aov_spp
