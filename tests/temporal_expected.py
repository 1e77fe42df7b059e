"""What rt_render_motion and rt_temporal_accumulate_fixed must give (include/rtcuda_amd.h, "temporal accumulation"; DESIGN.md
section 2.9), restated from the header's text in numpy float32: every operation below is one rounded float32 operation in the
header's order.  Reads neither rtcuda_amd/csrc/rt_temporal.h nor the CPU twins.  Hits come from OracleScene.trace_closest (the
literal walk for flags 0 and RT_FLAG_REFERENCE_WALK, after set_watertight() for RT_FLAG_WATERTIGHT), pixel-centre rays from
Oracle.camera_get_ray.  The synthetic cases of the accumulator's tests (CPU twin and kernel) live here too."""
import numpy as np

import aov_expected as ae

F32 = np.float32
FLT_MAX = ae.FLT_MAX
SCALE = 1.0 / 1073741824.0


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def f32(x):
    return np.asarray(x, np.float32)


def dot3(a, b):
    """(a.x * b.x + a.y * b.y) + a.z * b.z, each operation rounded; a, b (..., 3) float32."""
    a, b = f32(a), f32(b)
    return ((a[..., 0] * b[..., 0]).astype(F32) + (a[..., 1] * b[..., 1]).astype(F32)).astype(F32) + (a[..., 2] * b[..., 2]).astype(F32)


def cross3(a, b):
    """rt_device.h's cross: (a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x)."""
    a, b = f32(a), f32(b)
    return np.array([F32(F32(a[1] * b[2]) - F32(a[2] * b[1])), F32(F32(a[2] * b[0]) - F32(a[0] * b[2])),
                     F32(F32(a[0] * b[1]) - F32(a[1] * b[0]))], np.float32)


# ----------------------------------------------------------------------------- rt_render_motion
def centre_rays(oracle, cam12, w, h):
    """(origins, dirs) (w * h, 3) of the rays through the pixel centres: camera.get_ray((px + 0.5f) / w, (py + 0.5f) / h)."""
    o = np.zeros((w * h, 3), np.float32)
    d = np.zeros((w * h, 3), np.float32)
    for p in range(w * h):
        py, px = divmod(p, w)
        x = F32(F32(F32(px) + F32(0.5)) / F32(w))
        y = F32(F32(F32(py) + F32(0.5)) / F32(h))
        r = oracle.camera_get_ray(cam12, float(x), float(y))
        o[p], d[p] = r[:3], r[3:]
    return o, d


def previous_points(tri, u, v, prev_tris):
    """Step 4: e1 = q0 - q1, e2 = q2 - q0, P = (q0 - e1 * u) + e2 * v on row tri of prev_tris (n_tris, 9); rows of misses are 0."""
    tri = np.asarray(tri)
    q = f32(prev_tris).reshape(-1, 9)[np.where(tri >= 0, tri, 0)]
    q0, q1, q2 = q[:, 0:3], q[:, 3:6], q[:, 6:9]
    e1 = (q0 - q1).astype(F32)
    e2 = (q2 - q0).astype(F32)
    u, v = f32(u)[:, None], f32(v)[:, None]
    P = ((q0 - (e1 * u).astype(F32)).astype(F32) + (e2 * v).astype(F32)).astype(F32)
    P[tri < 0] = 0
    return P


def project(P, prev_cam12, w, h):
    """Steps 5 and 6 for points P (n, 3) -> (n, 3) float32 {sx, sy, dist}, sx = sy = -1 where lam is not positive and finite."""
    c = f32(prev_cam12)
    lf, ul, hz, vt = c[0:3], c[3:6], c[6:9], c[9:12]
    with np.errstate(all="ignore"):
        a = (f32(P) - lf).astype(F32)
        A = (ul - lf).astype(F32)
        m = cross3(hz, vt)
        lam = (dot3(A, m) / dot3(a, m)).astype(F32)
        r = ((a * lam[:, None]).astype(F32) - A).astype(F32)
        sx = ((dot3(r, hz) / dot3(hz, hz)).astype(F32) * F32(w)).astype(F32)
        sy = ((dot3(r, vt) / dot3(vt, vt)).astype(F32) * F32(h)).astype(F32)
        dist = np.sqrt(dot3(a, a)).astype(F32)
        ok = (lam > 0) & np.isfinite(lam)
    return np.stack([np.where(ok, sx, F32(-1)), np.where(ok, sy, F32(-1)), dist], axis=1).astype(F32)


def motion_records(tri, u, v, prev_tris, prev_cam12, w, h):
    """(n, 4) float32 records from given hits: {sx, sy, dist, bits of tri}; {0, 0, 0, bits of -1} on a miss."""
    tri = np.asarray(tri, np.int32)
    rec = np.zeros((tri.size, 4), np.float32)
    rec[:, :3] = project(previous_points(tri, u, v, prev_tris), prev_cam12, w, h)
    rec[tri < 0, :3] = 0
    rec[:, 3] = np.where(tri >= 0, tri, -1).astype(np.int32).view(np.float32)
    return rec


def motion_expected(oracle, osc, cam12, w, h, prev_cam12, prev_tris=None):
    """The motion buffer of a frame: `osc` is the OracleScene of the CURRENT vertices in the hit mode wanted; prev_tris None:
    the vertices did not move.  -> (records (w * h, 4), tri (w * h,))."""
    o, d = centre_rays(oracle, cam12, w, h)
    tri, _, u, v = osc.trace_closest(o, d, np.full(w * h, FLT_MAX, np.float32))
    prev = osc.arrays.tris if prev_tris is None else prev_tris
    return motion_records(tri, u, v, prev, prev_cam12, w, h), tri


def tri_ids(records):
    return np.ascontiguousarray(f32(records)[:, 3]).view(np.int32)


# ----------------------------------------------------------------------------- rt_temporal_accumulate_fixed
def fixed_to_float(s):
    return (np.asarray(s, np.int64).astype(np.float64) * SCALE).astype(F32)


def features(aov, spp):
    """(normal (n, 3), depth (n,), hits (n,)) as rt_aov_resolve forms them."""
    aov = np.asarray(aov, np.int64)
    inv = F32(1.0) / F32(spp)
    n = (fixed_to_float(aov[:, ae.NORMAL:ae.NORMAL + 3]) * inv).astype(F32)
    hits = aov[:, ae.HITS]
    with np.errstate(all="ignore"):
        z = np.where(hits > 0, (fixed_to_float(aov[:, ae.DEPTH]) / hits.astype(F32)).astype(F32), F32(0))
    return n, z, hits


def accumulate(sum_a, spp_a, sum_b, spp_b, aov, aov_spp, motion, history, w, h, max_history, alpha_min, depth_tolerance, normal_cos_min):
    """-> (hist_a (n, 3) int64, hist_b or None, length (n,) int32).  history: None or (hist_a, hist_b or None, length, prev_aov,
    prev_aov_spp).  Vectorised over the pixels; the four taps in the header's order."""
    n = w * h
    bufs = [(np.asarray(sum_a, np.int64), spp_a)] + ([(np.asarray(sum_b, np.int64), spp_b)] if sum_b is not None else [])
    c = [(fixed_to_float(s) * (F32(1.0) / F32(k))).astype(F32) for s, k in bufs]
    motion = f32(motion).reshape(n, 4)
    tri = tri_ids(motion)
    sw = np.zeros(n, np.float32)
    sh = [np.zeros((n, 3), np.float32) for _ in bufs]
    n_prev = np.full(n, np.iinfo(np.int64).max, np.int64)
    if history is not None:
        hist_in = [history[0]] + ([history[1]] if sum_b is not None else [])
        hist_in = [fixed_to_float(x) for x in hist_in]
        len_in = np.asarray(history[2], np.int32)
        n_p, _, _ = features(aov, aov_spp)
        n_q_all, z_q_all, hits_q_all = features(history[3], history[4])
        alpha_min, depth_tolerance, normal_cos_min = F32(alpha_min), F32(depth_tolerance), F32(normal_cos_min)
        with np.errstate(all="ignore"):
            fx = (motion[:, 0] - F32(0.5)).astype(F32)
            fy = (motion[:, 1] - F32(0.5)).astype(F32)
            dist = motion[:, 2]
            ok = (tri >= 0) & (fx >= F32(-1)) & (fx < F32(w)) & (fy >= F32(-1)) & (fy < F32(h))
            fx, fy = np.where(ok, fx, F32(0)), np.where(ok, fy, F32(0))
            flx, fly = np.floor(fx).astype(F32), np.floor(fy).astype(F32)
            x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
            ax, ay = (fx - flx).astype(F32), (fy - fly).astype(F32)
            tol = (depth_tolerance * dist).astype(F32)
            for j in (0, 1):
                for i in (0, 1):
                    xx, yy = x0 + i, y0 + j
                    inside = ok & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                    q = np.where(inside, yy * w + xx, 0)
                    dz = (z_q_all[q] - dist).astype(F32)
                    adz = np.where(dz < 0, -dz, dz)
                    acc = inside & (len_in[q] >= 1) & (hits_q_all[q] > 0) & (adz <= tol) & (dot3(n_p, n_q_all[q]) >= normal_cos_min)
                    b = ((ax if i else (F32(1) - ax).astype(F32)) * (ay if j else (F32(1) - ay).astype(F32))).astype(F32)
                    sw = np.where(acc, (sw + b).astype(F32), sw)
                    for k in range(len(bufs)):
                        sh[k] = np.where(acc[:, None], (sh[k] + (b[:, None] * hist_in[k][q]).astype(F32)).astype(F32), sh[k])
                    n_prev = np.where(acc, np.minimum(n_prev, len_in[q].astype(np.int64)), n_prev)
    blend = sw > 0
    N = np.where(blend, np.minimum(n_prev + (n_prev < np.iinfo(np.int64).max), max_history), 1).astype(np.int32)
    with np.errstate(all="ignore"):
        alpha = (F32(1.0) / N.astype(F32)).astype(F32)
        alpha = np.where(alpha > F32(alpha_min), alpha, F32(alpha_min)).astype(F32)
        outs = []
        for k in range(len(bufs)):
            hbar = (sh[k] / sw[:, None]).astype(F32)
            o = (((c[k] - hbar).astype(F32) * alpha[:, None]).astype(F32) + hbar).astype(F32)
            outs.append(ae.to_fixed(np.where(blend[:, None], o, c[k]).astype(F32)))
    return outs[0], (outs[1] if sum_b is not None else None), N


# ---- the synthetic cases both accumulator tests run (tests/test_temporal_host.py on the twin, tests/test_gpu_temporal.py on the kernel)
SIZES = ((1, 1), (1, 65), (33, 9), (97, 19))
PARAMS = dict(max_history=8, alpha_min=F32(0.125), depth_tolerance=F32(0.25), normal_cos_min=F32(0.5))


def random_sums(rng, n, ch=3, extreme=True):
    s = rng.integers(-(1 << 34), 1 << 34, size=(n, ch), dtype=np.int64)
    if extreme:
        flat = s.reshape(-1)
        flat[::7] = np.array([1 << 62, -(1 << 62)], np.int64)[np.arange(flat[::7].size) % 2]
    return s


def unit_aov(rng, n, spp, depth):
    """AOV sums of `spp` hits per pixel: a unit normal drawn from four directions, the given mean depth; every tenth pixel has no hit."""
    dirs = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8], [0, 0, -1]], np.float32)
    aov = np.zeros((n, ae.CHANNELS), np.int64)
    pick = rng.integers(0, 4, n)
    aov[:, ae.NORMAL:ae.NORMAL + 3] = ae.to_fixed(dirs[pick]) * spp
    aov[:, ae.DEPTH] = ae.to_fixed(f32(depth)) * spp
    aov[:, ae.HITS] = spp
    aov[::10] = 0
    return aov


def crafted_motion(w, h, rng):
    """(n, 4) records that walk through the cases of the tap step, one per pixel in turn; the rest of the frame has random
    positions near the pixel.  dist is set by the caller."""
    n = w * h
    px, py = (np.arange(n) % w).astype(np.float32), (np.arange(n) // w).astype(np.float32)
    rec = np.zeros((n, 4), np.float32)
    rec[:, 0] = px + F32(0.5) + rng.uniform(-1.5, 1.5, n).astype(np.float32)
    rec[:, 1] = py + F32(0.5) + rng.uniform(-1.5, 1.5, n).astype(np.float32)
    rec[:, 3] = np.arange(n, dtype=np.int32).view(np.float32)
    nan, inf = np.nan, np.inf
    below = np.nextafter(F32(-0.5), F32(-1))  # fx just below -1
    specials = [
        ("centre", lambda x, y: (x + 0.5, y + 0.5)), ("ax0", lambda x, y: (x + 0.5, y + 0.75)), ("ay0", lambda x, y: (x + 0.25, y + 0.5)),
        ("left-edge", lambda x, y: (-0.5, y + 0.5)), ("left-out", lambda x, y: (below, y + 0.5)), ("left-in", lambda x, y: (0.0, y + 0.3)),
        ("right-edge", lambda x, y: (w - 0.5, y + 0.5)), ("right-out", lambda x, y: (w + 0.5, y + 0.5)),
        ("right-just-in", lambda x, y: (np.nextafter(F32(w + 0.5), F32(0)), y + 0.5)),
        ("top-edge", lambda x, y: (x + 0.5, -0.5)), ("top-out", lambda x, y: (x + 0.5, below)),
        ("bottom-edge", lambda x, y: (x + 0.5, h - 0.5)), ("bottom-out", lambda x, y: (x + 0.5, h + 0.5)),
        ("corner", lambda x, y: (-0.5, -0.5)), ("far-corner", lambda x, y: (w + 0.25, h + 0.25)),
        ("minus-one", lambda x, y: (-1.0, -1.0)), ("nan-x", lambda x, y: (nan, y + 0.5)), ("nan-y", lambda x, y: (x + 0.5, nan)),
        ("inf", lambda x, y: (inf, y + 0.5)), ("minus-inf", lambda x, y: (x + 0.5, -inf)), ("huge", lambda x, y: (3e9, -3e9)),
        ("miss", None),
    ]
    for k, (name, f) in enumerate(specials):
        for p in range(k, n, max(len(specials) + 3, 1)):  # (a frame of one pixel gets the first case; the sizes walk through all)
            if f is None:
                rec[p] = (0, 0, 0, np.array(-1, np.int32).view(np.float32))
            else:
                with np.errstate(all="ignore"):
                    rec[p, 0], rec[p, 1] = (F32(t) for t in f(float(px[p]), float(py[p])))
    return rec


def synthetic_case(w, h, seed=0, two=True, spp=(2, 2), aov_spp=4, prev_spp=3):
    """One frame's inputs with history: dict(sum_a, sum_b, aov, motion, history=(hist_a, hist_b, len, prev_aov, prev_spp)).  Depths of
    the previous frame and the records' dist are drawn so that the depth stop falls on either side of equality (see
    equality_stops for the exact ones); normals from four directions against normal_cos_min = 0.5 (dots 1, 0.8, 0.6, 0, -1)."""
    rng = np.random.default_rng(1000 * w + h + seed)
    n = w * h
    case = dict(sum_a=random_sums(rng, n), sum_b=random_sums(rng, n) if two else None, spp=spp, aov_spp=aov_spp)
    case["aov"] = unit_aov(rng, n, aov_spp, np.full(n, 2.0))
    prev_depth = rng.choice(np.array([1.0, 1.5, 2.0, 2.5, 2.75, 4.0], np.float32), n)
    prev_aov = unit_aov(rng, n, prev_spp, prev_depth)
    motion = crafted_motion(w, h, rng)
    motion[:, 2] = np.where(tri_ids(motion) >= 0, F32(2.0), F32(0))
    motion[5::31, 2] = np.nan
    motion[7::37, 2] = np.inf
    length = rng.integers(0, 12, n).astype(np.int32)
    length[3::13] = -1
    length[4::17] = np.iinfo(np.int32).max
    case["motion"] = motion
    case["history"] = (random_sums(rng, n), random_sums(rng, n) if two else None, length, prev_aov, prev_spp)
    return case


def equality_stops():
    """A 4 x 1 frame, identity motion, whose stops sit exactly on and one ulp beside equality.  dist = 2, depth_tolerance = 0.25:
    the stop is |z_q - 2| <= 0.5 -- z_q = 2.5 passes, nextafter(2.5, 3) fails, 1.5 passes.  Normals: n_p = (0, 0, 1) exactly
    (to_fixed(1) * spp resolved with spp), n_q = (0, 0, c): the dot is c; normal_cos_min = c passes, nextafter(c, 1) fails.
    -> (case, parameter sets with the lengths each must give)."""
    w, h, n = 4, 1, 4
    one = ae.to_fixed(F32(1.0))
    aov = np.zeros((n, ae.CHANNELS), np.int64)
    aov[:, ae.NORMAL + 2] = one
    aov[:, ae.DEPTH] = ae.to_fixed(F32(2.0))
    aov[:, ae.HITS] = 1
    prev = aov.copy()
    z = np.array([2.5, np.nextafter(F32(2.5), F32(3)), 1.5, np.nextafter(F32(1.5), F32(1))], np.float32)
    prev[:, ae.DEPTH] = ae.to_fixed(z)
    assert (fixed_to_float(prev[:, ae.DEPTH]) == z).all()
    c = F32(0.625)
    prev[:, ae.NORMAL + 2] = ae.to_fixed(c)
    motion = np.zeros((n, 4), np.float32)
    motion[:, 0] = np.arange(n) + F32(0.5)
    motion[:, 1] = F32(0.5)
    motion[:, 2] = F32(2.0)
    motion[:, 3] = np.zeros(n, np.int32).view(np.float32)
    rng = np.random.default_rng(3)
    case = dict(sum_a=random_sums(rng, n, extreme=False), sum_b=random_sums(rng, n, extreme=False), spp=(1, 1), aov_spp=1, aov=aov,
                motion=motion, history=(random_sums(rng, n, extreme=False), random_sums(rng, n, extreme=False), np.full(n, 3, np.int32), prev, 1))
    base = dict(max_history=8, alpha_min=F32(0.125), depth_tolerance=F32(0.25))
    return case, [(dict(base, normal_cos_min=c), [4, 1, 4, 1]), (dict(base, normal_cos_min=np.nextafter(c, F32(1))), [1, 1, 1, 1])]


def run_case(fn, case, w, h, prm, history="given"):
    """fn(sum_a, spp_a, sum_b, spp_b, aov, aov_spp, motion, history, w, h, **prm) on a case dict."""
    hist = case["history"] if history == "given" else history
    return fn(case["sum_a"], case["spp"][0], case["sum_b"], case["spp"][1], case["aov"], case["aov_spp"], case["motion"], hist, w, h, **prm)


def identity_motion(w, h):
    n = w * h
    rec = np.zeros((n, 4), np.float32)
    rec[:, 0] = (np.arange(n) % w).astype(np.float32) + F32(0.5)
    rec[:, 1] = (np.arange(n) // w).astype(np.float32) + F32(0.5)
    rec[:, 2] = F32(2.0)
    rec[:, 3] = np.zeros(n, np.int32).view(np.float32)
    return rec


# ---- moving geometry for the motion tests: the glass bunny of full_bsdf (material 4) translated
def moved_arrays(arrays, delta):
    import dataclasses
    tris = np.array(arrays.tris, np.float32, copy=True).reshape(-1, 9)
    bunny = np.asarray(arrays.tri_material) == 4
    assert bunny.any()
    tris[bunny] = (tris[bunny] + np.tile(np.asarray(delta, np.float32), 3)).astype(np.float32)
    return dataclasses.replace(arrays, tris=tris)
