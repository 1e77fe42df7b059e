"""What rt_temporal_accumulate_moments_fixed and rt_denoise_variance_fixed must give (include/rtcuda_amd.h, "temporal moments and
two more stops"), restated from the header's text in numpy float32: every operation below is one rounded
float32 operation in the header's order.  Reads neither rtcuda_amd/csrc/rt_temporal.h nor the CPU twins.  What the header says
"is rt_temporal_accumulate_fixed's" / "rt_denoise_fixed's" / "rt_denoise_dual_fixed's" is imported from the restatements of
those.  The synthetic cases of the tests (CPU twins and kernels) live here too."""
import numpy as np

import aov_expected as ae
import denoise_dual_expected as dd
import denoise_expected as de
import temporal_expected as te

F32 = np.float32
INF = F32(np.inf)
VAR_MAX = F32(2.0 ** 87)
bits = te.bits


def emission(aov, spp):
    """e[k] = float(double(aov[EMISSION + k]) * 2^-30) * (1.f / spp)."""
    return (te.fixed_to_float(np.asarray(aov, np.int64)[:, ae.EMISSION:ae.EMISSION + 3]) * (F32(1.0) / F32(spp))).astype(F32)


def frame_moments(sum_a, spp_a, sum_b, spp_b, aov, aov_spp):
    """f (n, 4) = {u.x, u.y, u.z, dot(u, u)} with u the demodulated radiance of S = sum_a (+ sum_b, wrapping), n = spp_a (+ spp_b)."""
    if sum_b is None:
        s, n = np.asarray(sum_a, np.int64), spp_a
    else:
        s, n = dd.wrapped_sum(sum_a, sum_b), spp_a + spp_b
    u = de.prepare(s, n, aov, aov_spp)[0]
    with np.errstate(all="ignore"):
        return np.concatenate([u, te.dot3(u, u)[:, None]], axis=1).astype(F32)


def variance_of(m, N):
    """t = m[3] - dot(m1, m1); v = (t > 0 ? t : 0) / float(N)."""
    with np.errstate(all="ignore"):
        t = (m[..., 3] - te.dot3(m[..., :3], m[..., :3])).astype(F32)
        return (np.where(t > 0, t, F32(0)).astype(F32) / np.asarray(N).astype(F32)).astype(F32)


def spatial_variance(f, aov, aov_spp, N, w, h, depth_tolerance, normal_cos_min):
    """The spatial estimate at every pixel: the 5 x 5 window, dy outer and dx inner, the stops against the centre."""
    nrm, z, hits = te.features(aov, aov_spp)
    F, Z, NR, H = f.reshape(h, w, 4), z.reshape(h, w), nrm.reshape(h, w, 3), hits.reshape(h, w)
    cnt = np.zeros((h, w), F32)
    s = np.zeros((h, w, 4), F32)
    with np.errstate(all="ignore"):
        tol = (F32(depth_tolerance) * Z).astype(F32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                if dx == 0 and dy == 0:
                    counts = np.ones(cnt[P].shape, bool)
                else:
                    dz = (Z[Q] - Z[P]).astype(F32)
                    adz = np.where(dz < 0, -dz, dz)
                    counts = (H[Q] > 0) & (adz <= tol[P]) & (te.dot3(NR[P], NR[Q]) >= F32(normal_cos_min))
                cnt[P] = np.where(counts, (cnt[P] + F32(1)).astype(F32), cnt[P])
                s[P] = np.where(counts[..., None], (s[P] + F[Q]).astype(F32), s[P])
        M = (s / cnt[..., None]).astype(F32)
    return variance_of(M.reshape(-1, 4), N)


def accumulate_moments(sum_a, spp_a, sum_b, spp_b, aov, aov_spp, motion, history, w, h, max_history, alpha_min, depth_tolerance, normal_cos_min,
                       emission_tolerance, variance_min_history, moments=True):
    """-> (hist_a (n, 3) int64, hist_b or None, length (n,) int32, moments (n, 4) float32 or None, variance (n,) float32 or None).
    history: None or (hist_a, hist_b or None, length, prev_aov, prev_aov_spp, prev_motion or None, prev_moments or None).
    Vectorised over the pixels; the four taps in the header's order."""
    n = w * h
    bufs = [(np.asarray(sum_a, np.int64), spp_a)] + ([(np.asarray(sum_b, np.int64), spp_b)] if sum_b is not None else [])
    c = [(te.fixed_to_float(s) * (F32(1.0) / F32(k))).astype(F32) for s, k in bufs]
    motion = te.f32(motion).reshape(n, 4)
    tri = te.tri_ids(motion)
    sw = np.zeros(n, np.float32)
    sh = [np.zeros((n, 3), np.float32) for _ in bufs]
    sm = np.zeros((n, 4), np.float32)
    n_prev = np.full(n, np.iinfo(np.int64).max, np.int64)
    f = frame_moments(sum_a, spp_a, sum_b, spp_b, aov, aov_spp) if moments else None
    m_in = None
    if history is not None:
        hist_in = [history[0]] + ([history[1]] if sum_b is not None else [])
        hist_in = [te.fixed_to_float(x) for x in hist_in]
        len_in = np.asarray(history[2], np.int32)
        prev_ids = None if history[5] is None else te.tri_ids(te.f32(history[5]).reshape(n, 4))
        m_in = None if history[6] is None or not moments else te.f32(history[6]).reshape(n, 4)
        n_p, _, _ = te.features(aov, aov_spp)
        n_q_all, z_q_all, hits_q_all = te.features(history[3], history[4])
        e_p, e_q_all = emission(aov, aov_spp), emission(history[3], history[4])
        depth_tolerance, normal_cos_min, emission_tolerance = F32(depth_tolerance), F32(normal_cos_min), F32(emission_tolerance)
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
                    acc = inside & (len_in[q] >= 1) & (hits_q_all[q] > 0) & (adz <= tol) & (te.dot3(n_p, n_q_all[q]) >= normal_cos_min)
                    d = (e_p - e_q_all[q]).astype(F32)
                    ad = np.where(d < 0, -d, d)
                    dmax = ad[:, 0]
                    for k in (1, 2):
                        dmax = np.where(ad[:, k] > dmax, ad[:, k], dmax)
                    acc = acc & (dmax <= emission_tolerance)
                    if prev_ids is not None:
                        acc = acc & (prev_ids[q] == tri)
                    b = ((ax if i else (F32(1) - ax).astype(F32)) * (ay if j else (F32(1) - ay).astype(F32))).astype(F32)
                    sw = np.where(acc, (sw + b).astype(F32), sw)
                    for k in range(len(bufs)):
                        sh[k] = np.where(acc[:, None], (sh[k] + (b[:, None] * hist_in[k][q]).astype(F32)).astype(F32), sh[k])
                    if m_in is not None:
                        sm = np.where(acc[:, None], (sm + (b[:, None] * m_in[q]).astype(F32)).astype(F32), sm)
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
        m_out = var = None
        if moments:
            m_out = f
            if m_in is not None:
                mbar = (sm / sw[:, None]).astype(F32)
                o = (((f - mbar).astype(F32) * alpha[:, None]).astype(F32) + mbar).astype(F32)
                m_out = np.where(blend[:, None], o, f).astype(F32)
            temporal = variance_of(m_out, N)
            spatial = spatial_variance(f, aov, aov_spp, N, w, h, depth_tolerance, normal_cos_min)
            var = np.where(N >= variance_min_history, temporal, spatial).astype(F32)
    return outs[0], (outs[1] if sum_b is not None else None), N, m_out, var


def sanitise(x):
    """Step 2 of rt_denoise_variance_fixed: v = x > 0 ? (x < 2^87 ? x : 2^87) : 0."""
    x = te.f32(x)
    with np.errstate(all="ignore"):
        return np.where(x > 0, np.where(x < VAR_MAX, x, VAR_MAX), F32(0)).astype(F32)


def denoise_variance(beauty, spp, variance, aov, aov_spp, w, h, passes=None, sigma_variance=None, sigma_depth=None, normal_power_log2=None,
                     with_variance=False):
    """rt_denoise_variance_fixed: (h * w, 3) float32 linear mean radiance (and the final v with ``with_variance``)."""
    dp = dd.default_params()
    passes = dp["passes"] if passes is None else passes
    sigma_variance = dp["sigma_variance"] if sigma_variance is None else sigma_variance
    sigma_depth = dp["sigma_depth"] if sigma_depth is None else sigma_depth
    npow = dp["normal_power_log2"] if normal_power_log2 is None else normal_power_log2
    ks, kz, _ = dd.pass_constants(sigma_variance, sigma_depth, 1, 1)
    u, z, n, d, e = de.prepare(beauty, spp, aov, aov_spp)
    v = sanitise(variance).reshape(-1)
    assert u.shape[0] == w * h and v.shape[0] == w * h
    for i in range(passes):
        u, v = dd.atrous_var_pass(u, v, z, n, w, h, 1 << i, ks, kz, npow)
    with np.errstate(all="ignore"):
        out = ((u * d).astype(F32) + e).astype(F32)
    return (out, v) if with_variance else out


# ---- the synthetic cases both test files run (tests/test_temporal_moments_host.py on the twin, tests/test_gpu_temporal_moments.py
# on the kernel)
SIZES = te.SIZES + ((4, 1),)  # (1 x 1, 1 x 65, 33 x 9 -- the 5 x 5 window and the bilinear taps cross a 32 x 8 tile edge and the image edge --, 97 x 19)
assert {(1, 1), (4, 1), (33, 9), (97, 19)} <= set(SIZES)
EMISSION_TOLERANCE = F32(0.25)
PARAMS = dict(te.PARAMS, emission_tolerance=EMISSION_TOLERANCE, variance_min_history=2)


def param_sets():
    """variance_min_history 1 (temporal wherever a length exists), 2 (mixed), max_history + 1 (spatial everywhere); the emission
    stop at its tolerance, open and shut; stops that accept everything."""
    mh = PARAMS["max_history"]
    return (dict(PARAMS, variance_min_history=1), PARAMS, dict(PARAMS, variance_min_history=mh + 1), dict(PARAMS, emission_tolerance=INF),
            dict(PARAMS, emission_tolerance=F32(0.0), max_history=3),
            dict(PARAMS, normal_cos_min=F32(-1.0), depth_tolerance=F32(1e30), emission_tolerance=F32(1e30), variance_min_history=3))


def history_variants(hist):
    """(history, moments): no triangle stop; no moments history; neither; no moments at all, with and without the triangle stop."""
    return tuple((hist[:5] + (h5, h6), moments) for h5, h6, moments in
                 ((None, hist[6], True), (hist[5], None, True), (None, None, True), (hist[5], None, False), (None, None, False)))


def synthetic_case(w, h, seed=0, two=True, **kw):
    """temporal_expected.synthetic_case with what the new entry point reads besides: triangle ids from a handful of values in both
    motion buffers (so the triangle stop passes some taps and fails others, -1 among the previous ids), first-hit emission in both
    AOV frames from values whose differences are 0, exactly EMISSION_TOLERANCE, one ulp more, and larger (in one channel each), an
    albedo on half of the pixels, and a moments history.  history grows to (hist_a, hist_b, len, prev_aov, prev_spp, prev_motion,
    prev_moments)."""
    case = te.synthetic_case(w, h, seed=seed, two=two, **kw)
    rng = np.random.default_rng(77 * w + h + seed)
    n = w * h
    motion = case["motion"]
    ids = te.tri_ids(motion).copy()
    ids[ids >= 0] = rng.integers(0, 3, int((ids >= 0).sum()))
    motion[:, 3] = ids.view(np.float32)
    prev_motion = np.zeros((n, 4), np.float32)
    prev_motion[:, :3] = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    prev_motion[:, 3] = rng.choice(np.array([-1, 0, 0, 1, 2], np.int32), n).view(np.float32)
    levels = np.array([0.0, 0.5, 0.75, np.nextafter(F32(0.75), F32(1)), 4.0], np.float32)  # |0.5 - 0.75| = tol; one ulp beyond; far
    aov_spp, prev_spp = case["aov_spp"], case["history"][4]
    prev_aov = case["history"][3]
    for aov, spp, pick in ((case["aov"], aov_spp, np.array([0, 1, 1, 1])), (prev_aov, prev_spp, np.array([0, 1, 2, 3, 4]))):
        lit = aov[:, ae.HITS] > 0
        ch = rng.integers(0, 3, n)
        val = levels[rng.choice(pick, n)]
        for k in range(3):
            aov[:, ae.EMISSION + k] = np.where(lit & (ch == k), ae.to_fixed(val) * spp, ae.to_fixed(F32(0.5)) * spp * lit)
        aov[:, ae.ALBEDO:ae.ALBEDO + 3] = np.where((lit & (rng.random(n) < 0.5))[:, None], ae.to_fixed(F32(0.625)) * spp, 0)
    m_prev = rng.uniform(0, 8, (n, 4)).astype(np.float32)
    m_prev[:, 3] = (te.dot3(m_prev[:, :3], m_prev[:, :3]) + rng.uniform(0, 4, n).astype(np.float32)).astype(np.float32)
    m_prev[::11] = (F32(2.0 ** 43), F32(0), F32(2.0 ** 40), F32(2.0 ** 88))
    case["history"] = case["history"] + (prev_motion, m_prev)
    return case


def run_case(fn, case, w, h, prm, history="given", **kw):
    hist = case["history"] if history == "given" else history
    return fn(case["sum_a"], case["spp"][0], case["sum_b"], case["spp"][1], case["aov"], case["aov_spp"], case["motion"], hist, w, h, **prm, **kw)


def emission_equality_case():
    """A 4 x 1 frame, identity motion, stops that pass, whose emission differences sit on and one float above the tolerance 0.25:
    pixel 0: e_p.x = 0.25 against 0 (accepted), pixel 1: nextafter(0.25, 1) against 0 (rejected), pixels 2 and 3 the same with the
    sign turned and in channel z.  -> (case, [(parameters, the lengths they must give)])."""
    case, _ = te.equality_stops()
    n = 4
    above = np.nextafter(F32(0.25), F32(1))
    aov, prev = case["aov"], case["history"][3].copy()
    prev[:, ae.DEPTH] = aov[:, ae.DEPTH]
    prev[:, ae.NORMAL + 2] = aov[:, ae.NORMAL + 2]
    aov[:, ae.EMISSION] = ae.to_fixed(np.array([0.25, above, 0, 0], np.float32))
    prev[:, ae.EMISSION + 2] = ae.to_fixed(np.array([0, 0, 0.25, above], np.float32))
    assert (emission(aov, 1)[:2, 0] == np.array([0.25, above], np.float32)).all()
    ids = np.array([5, 5, 6, -1], np.int32)
    prev_motion = np.zeros((n, 4), np.float32)
    prev_motion[:, 3] = ids.view(np.float32)
    case["motion"][:, 3] = np.array([5, 5, 5, 5], np.int32).view(np.float32)
    h0 = case["history"]
    case["history"] = (h0[0], h0[1], h0[2], prev, 1, None, None)
    with_ids = dict(case, history=(h0[0], h0[1], h0[2], prev, 1, prev_motion, None))
    base = dict(max_history=8, alpha_min=F32(0.125), depth_tolerance=F32(0.25), normal_cos_min=F32(0.5), variance_min_history=1)
    return [(case, dict(base, emission_tolerance=F32(0.25)), [4, 1, 4, 1]), (case, dict(base, emission_tolerance=above), [4, 4, 4, 4]),
            (case, dict(base, emission_tolerance=F32(0.0)), [1, 1, 1, 1]), (case, dict(base, emission_tolerance=INF), [4, 4, 4, 4]),
            (with_ids, dict(base, emission_tolerance=INF), [4, 4, 1, 1])]


def lonely_centre_case():
    """A 5 x 5 first frame whose centre pixel faces +z and all others -z: at the centre only the centre counts, M = f and
    v = f[3] - dot(u, u) = 0 exactly, whatever its radiance.  -> (case, the centre's index)."""
    w = h = 5
    n = w * h
    rng = np.random.default_rng(8)
    aov = np.zeros((n, ae.CHANNELS), np.int64)
    aov[:, ae.NORMAL + 2] = -ae.to_fixed(F32(1.0))
    aov[12, ae.NORMAL + 2] = ae.to_fixed(F32(1.0))
    aov[:, ae.DEPTH] = ae.to_fixed(F32(2.0))
    aov[:, ae.HITS] = 1
    case = dict(sum_a=te.random_sums(rng, n, extreme=False), sum_b=None, spp=(1, 0), aov=aov, aov_spp=1, motion=te.identity_motion(w, h), history=None)
    case["sum_a"] = np.abs(case["sum_a"])
    return case, 12
