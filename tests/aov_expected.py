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
