"""What an AOV frame must hold (rt_render_aov_fixed / rt_render_aov_rays_fixed_device), from numpy and
the oracle alone.  Rays: raytable_keyed.keyed_pinhole_table (held to the oracle by tests/test_render_rays_keyed_host.py) or any
table.  Hits: OracleScene.trace_closest -- the literal walk for flags 0 and RT_FLAG_REFERENCE_WALK, after set_watertight() for
RT_FLAG_WATERTIGHT.  Normals: Oracle.triangle(p9) and a float32 restatement of unit (1 / sqrt, then three products).  to_fixed
and the resolve are restated in numpy.  tests/test_aov_host.py holds this file to the oracle's own per-sample frame before any
GPU test leans on it."""
import numpy as np

import raytable_keyed as rk

CHANNELS = 11
ALBEDO, NORMAL, EMISSION, DEPTH, HITS = 0, 3, 6, 9, 10
FLT_MAX = np.float32(3.4028234663852886e38)
F32 = np.float32


def to_fixed(x):
    """to_fixed of the kernels: non-finite or |x| > 2^31 is clamped (NaN: 0), then the float32 product x * 2^30 rounded to the
    nearest integer, ties to even."""
    x = np.array(x, np.float32, copy=True)
    big = ~(np.abs(x) <= F32(2147483648.0))
    x[big] = np.where(np.isnan(x[big]), F32(0), np.copysign(F32(2147483648.0), x[big]))
    return np.rint((x * F32(1073741824.0)).astype(np.float32).astype(np.float64)).astype(np.int64)


_normal_cache = {}


def shading_normals(oracle, arrays, tri_ids):
    """-unit(tri.n) of the triangles `tri_ids` ((k,) caller's order) -> (k, 3) float32: n from Oracle.triangle, unit as
    vec3.cuh:131-134 (inv_len = 1 / sqrt((x * x + y * y) + z * z), three products), the sign flipped."""
    cache = _normal_cache.setdefault(id(arrays), {})
    tris = np.asarray(arrays.tris, np.float32).reshape(-1, 9)
    out = np.zeros((len(tri_ids), 3), np.float32)
    for k, t in enumerate(np.asarray(tri_ids).tolist()):
        if t not in cache:
            n = oracle.triangle(tris[t])[0][9:12].astype(np.float32)
            inv_len = F32(1.0) / np.sqrt(F32(F32(n[0] * n[0]) + F32(n[1] * n[1])) + F32(n[2] * n[2]))
            cache[t] = -(n * F32(inv_len)).astype(np.float32)
        out[k] = cache[t]
    return out


def sample_features(oracle, osc, o, d):
    """Per ray: (tri (n,) int32 in the caller's order or -1, material (n,) int32 or -1, values (n, 10) float32: albedo, faced
    normal, emission, depth; zero rows on a miss).  `osc`: the OracleScene in the hit mode wanted."""
    arrays = osc.arrays
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    n = o.shape[0]
    tri, t, _, _ = osc.trace_closest(o, d, np.full(n, FLT_MAX, np.float32))
    hit = tri >= 0
    vals = np.zeros((n, 10), np.float32)
    mat = np.full(n, -1, np.int32)
    k = tri[hit]
    mat[hit] = np.asarray(arrays.tri_material, np.int32)[k]
    vals[hit, ALBEDO:ALBEDO + 3] = arrays.materials["albedo"][mat[hit]]
    nn = shading_normals(oracle, arrays, k)
    dd = d[hit]
    dot = ((nn[:, 0] * dd[:, 0]).astype(np.float32) + (nn[:, 1] * dd[:, 1]).astype(np.float32)).astype(np.float32)
    dot = (dot + (nn[:, 2] * dd[:, 2]).astype(np.float32)).astype(np.float32)
    vals[hit, NORMAL:NORMAL + 3] = np.where((dot > 0)[:, None], -nn, nn)
    li = np.asarray(arrays.tri_light, np.int32)[k]
    em = np.zeros((len(k), 3), np.float32)
    if len(arrays.lights):
        em[li >= 0] = arrays.lights["L"][li[li >= 0]]
    vals[hit, EMISSION:EMISSION + 3] = em
    vals[hit, DEPTH] = t[hit]
    return tri.astype(np.int32), mat, vals


def deposit(tri, vals, pixel, n_pixels):
    """The int64 sums (n_pixels, 11) of samples that land on `pixel`."""
    sums = np.zeros((n_pixels, CHANNELS), np.int64)
    hit = tri >= 0
    fx = to_fixed(vals[hit])
    p = np.asarray(pixel, np.int64)[hit]
    for c in range(10):
        np.add.at(sums[:, c], p, fx[:, c])
    np.add.at(sums[:, HITS], p, 1)
    return sums


def table_expected(oracle, osc, o, d, pixel, n_pixels, first=None):
    """(sums (n_pixels, 11) int64, ids (n_pixels, 2) int32) of a table whose row c lands on pixel[c]; `first`: boolean mask of the
    rows that write their pixel's ids (ids of pixels no such row lands on stay -7, the tests' poison)."""
    tri, mat, vals = sample_features(oracle, osc, o, d)
    sums = deposit(tri, vals, pixel, n_pixels)
    ids = np.full((n_pixels, 2), -7, np.int32)
    if first is not None:
        f = np.asarray(first, bool)
        ids[np.asarray(pixel)[f], 0] = tri[f]
        ids[np.asarray(pixel)[f], 1] = mat[f]
    return sums, ids


def frame_expected(oracle, osc, cam12, w, h, spp, seed=1, shard=(0, 1)):
    """(sums, ids, (tri, mat, vals, pixel, keys)) of shard (r, R) of the camera's AOV frame: the samples G with G % R == r."""
    r, R = shard
    keys = np.arange(r, w * h * spp, R, dtype=np.int64)
    o, d, pixel = rk.keyed_pinhole_table(oracle, cam12, w, h, spp, seed, keys.tolist())
    tri, mat, vals = sample_features(oracle, osc, o, d)
    sums = deposit(tri, vals, pixel, w * h)
    ids = np.full((w * h, 2), -7, np.int32)
    f = keys % spp == 0
    ids[pixel[f], 0] = tri[f]
    ids[pixel[f], 1] = mat[f]
    return sums, ids, (tri, mat, vals, pixel, keys)


def resolve(sums, spp):
    """rt_aov_resolve in numpy: s = float32(float64(sum) * 2^-30), inv = 1.f / spp; albedo, normal, emission s * inv; depth
    s / float32(hits) where hits > 0, else 0; channel 10 float32(hits) * inv."""
    sums = np.asarray(sums, np.int64)
    s = (sums.astype(np.float64) * (1.0 / 1073741824.0)).astype(np.float32)
    inv = F32(1.0) / F32(spp)
    out = (s * inv).astype(np.float32)
    hits = sums[:, HITS]
    hf = hits.astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[:, DEPTH] = np.where(hits > 0, (s[:, DEPTH] / hf).astype(np.float32), F32(0))
    out[:, HITS] = (hf * inv).astype(np.float32)
    return out


# The wide-angle view of the frame tests: off the box's axis, vfov 80 -- most of the frame looks past the box, the rest holds
# the light, the glass bunny and the mirror wall (tests/test_aov_host.py checks those shares on the CPU).
WIDE_VIEW = dict(lookfrom=(0.3, 0.6, 1.2), lookat=(0.5, 0.5, 0.0), up=(0.0, 1.0, 0.0), vfov=80.0)
WIDE_FRAME = (32, 24, 2)


def wide_camera(make_camera, aspect):
    """make_camera: Oracle.camera or api.make_camera (the same 12 floats)."""
    v = WIDE_VIEW
    return make_camera(v["lookfrom"], v["lookat"], v["up"], v["vfov"], aspect)


def assert_wide_content(arrays, tri, mat, sums):
    """What makes the wide frame worth rendering: at least 5 % misses, at least 5 % hits, emission, hits on a non-matte."""
    miss = float(np.mean(tri < 0))
    assert miss >= 0.05 and 1.0 - miss >= 0.05, miss
    assert int(sums[:, EMISSION:EMISSION + 3].sum()) > 0
    assert int(np.sum(arrays.materials["type"][mat[mat >= 0]] != 0)) > 0


# ---- what tests/test_aov_deposit_host.py and tests/test_gpu_aov_deposit.py share: pixel arrays with known runs for the in-wave
# sums of aov_deposit, the exact-integer bound on a frame's sums, values at the edges of to_fixed, sums at the edges of the resolve
FIBONACCI_RUNS = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144)


def run_lengths(pixel):
    """The lengths of the maximal runs of equal neighbours of `pixel`, in order."""
    p = np.asarray(pixel)
    if p.size == 0:
        return np.zeros(0, np.int64)
    cut = np.flatnonzero(p[1:] != p[:-1]) + 1
    return np.diff(np.concatenate([[0], cut, [p.size]])).astype(np.int64)


def run_histogram(pixel):
    """{run length: number of such runs} of `pixel`."""
    length, count = np.unique(run_lengths(pixel), return_counts=True)
    return dict(zip(length.tolist(), count.tolist()))


def drawn_runs(n, seed=5, lengths=FIBONACCI_RUNS, n_pixels=16):
    """(pixel (n,) int32, the run lengths drawn): runs of lengths drawn from `lengths`, each run's pixel drawn from 0 ..
    n_pixels - 1 with repetition -- but never its predecessor's, so that a drawn run is a run; the last run is cut at n."""
    rng = np.random.default_rng(seed)
    pixel = np.zeros(n, np.int32)
    drawn = []
    at, last = 0, -1
    while at < n:
        k = min(int(rng.choice(lengths)), n - at)
        p = int(rng.integers(0, n_pixels)) if last < 0 else int(rng.integers(0, n_pixels - 1))
        p += 0 <= last <= p
        pixel[at:at + k] = p
        drawn.append(k)
        at, last = at + k, p
    return pixel, drawn


def exact_sums(tri, vals, pixel, n_pixels):
    """deposit() in Python integers: asserts that every sum fits int64 (what lies beyond is outside the contract of the
    entry points, and numpy's int64 adds would wrap in silence) and that deposit() gives the same."""
    hit = np.asarray(tri) >= 0
    fx = to_fixed(vals[hit]).astype(object)
    p = np.asarray(pixel, np.int64)[hit]
    sums = np.zeros((n_pixels, CHANNELS), object)
    for c in range(10):
        np.add.at(sums[:, c], p, fx[:, c])
    np.add.at(sums[:, HITS], p, 1)
    top = max(abs(int(v)) for v in sums.ravel())
    assert top < 1 << 63, ("a sum leaves int64", top)
    out = sums.astype(np.int64)
    assert np.array_equal(out, deposit(tri, vals, pixel, n_pixels))
    return out


def table_cases(tri):
    """The pixel arrays of the crafted tables, from the hit triangles `tri` (n,) of the base table: a list of (name, rows (k,)
    into the base table, pixel (k,) int32, n_pixels, the run-length histogram claimed).  H: the rows that hit, M: those
    that miss, B: all."""
    tri = np.asarray(tri)
    n = tri.size
    H, M, B = np.flatnonzero(tri >= 0), np.flatnonzero(tri < 0), np.arange(n)
    cases = []

    def whole_runs(k, length, first=None):  # runs of `length` over k rows, the first one `first` long, the last one the rest
        first = length if first is None else first
        h = {}
        for r in [first] + [length] * ((k - first) // length) + [(k - first) % length]:
            if r:
                h[r] = h.get(r, 0) + 1
        return h

    def add(name, rows, pixel, n_pixels, claim):
        pixel = np.ascontiguousarray(pixel, np.int32)
        assert pixel.shape == rows.shape and pixel.min() >= 0 and pixel.max() < n_pixels
        cases.append((name, rows, pixel, int(n_pixels), claim))

    c = np.arange(H.size)
    add("H-full-waves", H, c // 64, (H.size + 63) // 64, whole_runs(H.size, 64))
    add("H-split-across-chunks", H, (c + 32) // 64, (H.size + 32 + 63) // 64, whole_runs(H.size, 64, 32))
    add("H-one-address", H, np.ones(H.size), 3, {H.size: 1})
    add("H-alternating", H, c % 2, 2, {1: H.size})
    runs, drawn = drawn_runs(n)
    h = {}
    for r in drawn:
        h[r] = h.get(r, 0) + 1
    add("B-drawn-runs", B, runs, 16, h)
    nb = (n + 6) // 7
    add("B-descending-sevens", B, nb - 1 - B // 7, nb, whole_runs(n, 7))
    add("M-nothing-deposits", M, np.arange(M.size) // 64, (M.size + 63) // 64, whole_runs(M.size, 64))
    # even rows from H's first half, odd rows from its second: every pixel occurs 64 times, never in two neighbouring rows
    half = H.size // 2
    order = np.empty(2 * half, np.int64)
    order[0::2], order[1::2] = np.arange(half), half + np.arange(half)
    assert half >= 64  # (rows j and half + j lie at least a pixel apart)
    add("H-interleaved-halves", H[order], order // 64, (2 * half + 63) // 64, {1: 2 * half})
    return cases


EXTREME_VALUES = (3e9, -3e9, np.inf, -np.inf, np.nan, -0.5, 1e-10, 1.5 * 2.0 ** -31, 1.0)
EXTREME_LIGHT = (3e9, -np.inf, np.nan)
EXTREME_FRAME = (64, 48, 2)


def extreme_arrays(arrays, seed=11):
    """A copy of `arrays` whose albedos are drawn from EXTREME_VALUES (two seeded permutations of the nine one after the other:
    the first three materials hold every value) and whose lights all have L = EXTREME_LIGHT."""
    import dataclasses
    rng = np.random.default_rng(seed)
    mats = arrays.materials.copy()
    k = mats["albedo"].size
    draw = np.concatenate([rng.permutation(len(EXTREME_VALUES)) for _ in range((k + 8) // 9)])[:k]
    with np.errstate(over="ignore"):
        mats["albedo"] = np.array(EXTREME_VALUES, np.float32)[draw].reshape(mats["albedo"].shape)
        lights = arrays.lights.copy()
        lights["L"] = np.array(EXTREME_LIGHT, np.float32)
    return dataclasses.replace(arrays, materials=mats, lights=lights)


RESOLVE_LITERALS = (0, 1, (1 << 30) - 1, 1 << 53, (1 << 53) + 1, 1 << 61)
RESOLVE_HITS = (0, 1, 2, 3, 1 << 24, (1 << 24) + 1, 1 << 31, 1 << 40, -1)
RESOLVE_PIXELS = (1, 23, 24, 1000, 100003)
RESOLVE_SAMPLES = (1, 3, 7, 16, 1000003, (1 << 31) - 1)


def synthetic_sums(n_pixels, seed=17):
    """(n_pixels, 11) int64 for the resolve: values uniform over +-2^62, every third one replaced by one of +-RESOLVE_LITERALS in
    turn; hits from RESOLVE_HITS in turn (so one pixel already holds all of a kind that a small n_pixels can)."""
    rng = np.random.default_rng(seed + n_pixels)
    sums = rng.integers(-(1 << 62), (1 << 62) + 1, size=(n_pixels, CHANNELS), dtype=np.int64)
    lit = np.array([s * v for v in RESOLVE_LITERALS for s in (1, -1)], np.int64)
    flat = sums.reshape(-1)
    at = np.arange(0, flat.size, 3)
    flat[at] = lit[(np.arange(at.size) + n_pixels) % lit.size]
    sums[:, HITS] = np.array(RESOLVE_HITS, np.int64)[(np.arange(n_pixels) + n_pixels) % len(RESOLVE_HITS)]
    return sums


# (w, h, spp, wide view): runs of 16 (scan distances 1 to 8), runs that straddle every chunk boundary at another lane, a chunk
# that is one pixel (all six distances, one deposit per wave), a run start that shifts by a lane per pixel, a pixel of several
# chunks and waves, every wave on one address, long runs broken up by misses
DEPOSIT_FRAMES = ((8, 6, 16, False), (5, 3, 33, False), (4, 3, 64, False), (3, 2, 65, False), (2, 2, 200, False), (1, 1, 1000, False),
                  (5, 4, 64, True))
DEPOSIT_SHARD_FRAME = (4, 3, 64)
DEPOSIT_BASE_TABLE = (64, 48, 4)
KEYS_RPP, KEYS_FIRST, KEYS_ROWS = 64, (1 << 32) - 100, 1000         # pixel = K // 64 around K = 2^32
WIDE_KEYS_RPP, WIDE_KEYS_STRIDE, WIDE_KEYS_ROWS = 3 << 28, 1 << 25, 288  # row c: t = c * 2^25 passes 2^32 inside the run of pixel 5


def frame_census(sums, spp):
    """(full, partial, empty): the pixels with hits == spp, 0 < hits < spp, hits == 0."""
    hits = sums[:, HITS]
    return int((hits == spp).sum()), int(((hits > 0) & (hits < spp)).sum()), int((hits == 0).sum())
