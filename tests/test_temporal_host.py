"""CPU tests of temporal accumulation (rt_render_motion, rt_temporal_accumulate_fixed, rt_temporal_default_params): the CPU twins
(hc_motion_records and hc_temporal_accumulate of librt_hostcheck.so: serial loops over rtcuda_amd/csrc/rt_temporal.h, the kernels'
arithmetic) are held to the numpy restatement of the header's text (tests/temporal_expected.py) bit for bit; the accumulator's
properties and the projection's accuracy are shown; the entry points are declared / exported / bound / refuse bad arguments.
Everything that runs a kernel is in tests/test_gpu_motion.py and tests/test_gpu_temporal.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, default_camera, oracle_scene
import aov_expected as ae
import temporal_expected as te
import temporal_moments_expected as tm

NEW = ("rt_render_motion", "rt_temporal_default_params", "rt_temporal_accumulate_fixed")
F32 = np.float32


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


@pytest.fixture(scope="module")
def hc(api):
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.hc_motion_records.argtypes = [ci, vp, vp, vp, vp, ci, vp, ci, ci, vp]
    L.hc_temporal_accumulate.argtypes = [vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, cf, cf, cf, vp, vp, vp]
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data


def twin_accumulate(hc, sum_a, spp_a, sum_b, spp_b, aov, aov_spp, motion, history, w, h, max_history, alpha_min, depth_tolerance,
                    normal_cos_min, expect_rc=0):
    n = w * h
    c64 = lambda a: None if a is None else np.ascontiguousarray(a, np.int64)  # noqa: E731
    sum_a, sum_b, aov = c64(sum_a), c64(sum_b), c64(aov)
    motion = np.ascontiguousarray(motion, np.float32)
    ha = hb = ln = pa = None
    ps = 1
    if history is not None:
        ha, hb, ln, pa, ps = c64(history[0]), c64(history[1]), np.ascontiguousarray(history[2], np.int32), c64(history[3]), history[4]
    out_a = np.full((n, 3), -7, np.int64)
    out_b = None if sum_b is None else np.full((n, 3), -7, np.int64)
    out_len = np.full(n, -7, np.int32)
    rc = hc.hc_temporal_accumulate(_ptr(sum_a), spp_a, _ptr(sum_b), spp_b, _ptr(aov), aov_spp, _ptr(motion), _ptr(ha), _ptr(hb), _ptr(ln),
                                   _ptr(pa), ps, w, h, int(max_history), float(alpha_min), float(depth_tolerance), float(normal_cos_min),
                                   _ptr(out_a), _ptr(out_b), _ptr(out_len))
    assert rc == expect_rc
    return out_a, out_b, out_len


def twin_case(hc, case, w, h, prm, history="given"):
    return te.run_case(lambda *a, **k: twin_accumulate(hc, *a, **k), case, w, h, prm, history)


def twin_motion(hc, tri, u, v, prev_tris, cam12, w, h):
    tri, u, v = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
    prev_tris, cam12 = np.ascontiguousarray(prev_tris, np.float32).reshape(-1, 9), np.ascontiguousarray(cam12, np.float32)
    out = np.full((tri.size, 4), -7, np.float32)
    assert hc.hc_motion_records(tri.size, _ptr(tri), _ptr(u), _ptr(v), _ptr(prev_tris), prev_tris.shape[0], _ptr(cam12), w, h, _ptr(out)) == 0
    return out


def assert_same(got, want):
    for g, x in zip(got, want):
        if x is None:
            assert g is None
            continue
        g, x = te.bits(g), te.bits(x)
        assert g.shape == x.shape and g.dtype == x.dtype
        bad = np.flatnonzero((g != x).reshape(-1))
        assert bad.size == 0, (bad.size, bad[:5], g.reshape(-1)[bad[:5]], x.reshape(-1)[bad[:5]])


# ----------------------------------------------------------------------------- the accumulator's twin against the restatement
@pytest.mark.parametrize("w,h", te.SIZES)
@pytest.mark.parametrize("two", [True, False])
def test_accumulate_twin_equals_the_restatement(hc, w, h, two):
    case = te.synthetic_case(w, h, two=two)
    n = w * h
    if n >= 600:  # the claims of the case: every branch of the tap step is taken somewhere
        want = te.run_case(te.accumulate, case, w, h, te.PARAMS)
        ln = want[2]
        assert (ln == 1).any() and (ln == te.PARAMS["max_history"]).any() and ((ln > 1) & (ln < te.PARAMS["max_history"])).any()
        assert (np.abs(case["sum_a"]) >= 1 << 62).any() and (case["history"][2] == 0).any()
    for prm in (te.PARAMS, dict(te.PARAMS, max_history=1), dict(te.PARAMS, alpha_min=F32(1.0)), dict(te.PARAMS, normal_cos_min=F32(-1.0), depth_tolerance=F32(1e30)),
                dict(max_history=0x7fffffff, alpha_min=F32(1e-30), depth_tolerance=F32(0.5), normal_cos_min=F32(1.0))):
        assert_same(twin_case(hc, case, w, h, prm), te.run_case(te.accumulate, case, w, h, prm))
    # the first frame
    assert_same(twin_case(hc, case, w, h, te.PARAMS, history=None), te.run_case(te.accumulate, case, w, h, te.PARAMS, history=None))


def test_stops_on_either_side_of_equality(hc):
    case, sets = te.equality_stops()
    for prm, lengths in sets:
        want = te.run_case(te.accumulate, case, 4, 1, prm)
        assert want[2].tolist() == lengths
        got = twin_accumulate(hc, case["sum_a"], 1, case["sum_b"], 1, case["aov"], 1, case["motion"], case["history"], 4, 1, **prm)
        assert_same(got, want)


def test_special_outcomes(hc):
    """max_history = 1: N = 1 and alpha = 1, so the output is c wherever history was found -- (c - hbar) * 1 + hbar is c up to the
    rounding of the two operations, so compare with the restatement; alpha_min = 1 the same; a len_in of 0 or less is no history."""
    w, h = 33, 9
    case = te.synthetic_case(w, h)
    got = twin_accumulate(hc, case["sum_a"], 2, case["sum_b"], 2, case["aov"], 4, case["motion"], case["history"], w, h, **dict(te.PARAMS, max_history=1))
    assert (got[2] == 1).all()
    hist = list(case["history"])
    hist[2] = np.zeros(w * h, np.int32)
    got = twin_accumulate(hc, case["sum_a"], 2, case["sum_b"], 2, case["aov"], 4, case["motion"], tuple(hist), w, h, **te.PARAMS)
    first = twin_accumulate(hc, case["sum_a"], 2, case["sum_b"], 2, case["aov"], 4, case["motion"], None, w, h, **te.PARAMS)
    assert_same(got, first)


def test_first_frame_is_to_fixed_of_the_mean(hc):
    w, h = 33, 9
    case = te.synthetic_case(w, h)
    a, b, ln = twin_accumulate(hc, case["sum_a"], 2, case["sum_b"], 3, case["aov"], 4, case["motion"], None, w, h, **te.PARAMS)
    assert (ln == 1).all()
    for out, s, spp in ((a, case["sum_a"], 2), (b, case["sum_b"], 3)):
        c = (te.fixed_to_float(s) * (F32(1) / F32(spp))).astype(F32)
        assert np.array_equal(out, ae.to_fixed(c))
    assert (np.abs(a) == 1 << 61).any()  # (sums of 2^62 resolve to 2^31 and beyond: the clamp of to_fixed is exercised)


def test_one_buffer_equals_the_two_buffer_a(hc):
    for w, h in ((33, 9), (97, 19)):
        case = te.synthetic_case(w, h)
        two = twin_accumulate(hc, case["sum_a"], 2, case["sum_b"], 2, case["aov"], 4, case["motion"], case["history"], w, h, **te.PARAMS)
        hist = (case["history"][0], None) + tuple(case["history"][2:])
        one = twin_accumulate(hc, case["sum_a"], 2, None, 0, case["aov"], 4, case["motion"], hist, w, h, **te.PARAMS)
        assert one[1] is None and np.array_equal(one[0], two[0]) and np.array_equal(one[2], two[2])


def test_forwarded_twin_has_the_emission_stop_off(hc):
    """hc_temporal_accumulate is hc_temporal_accumulate_moments with emission_tolerance = +inf.  temporal_expected.synthetic_case
    cannot see a forward that left the stop on: unit_aov writes no emission, so both frames' emission is 0 everywhere and the stop
    passes every tap at any tolerance >= 0.  temporal_moments_expected.synthetic_case gives both AOV frames first-hit emission that
    differs by far more than any tolerance in use; on it the twin (which never reads a previous motion buffer or moments) must still equal
    temporal_expected.accumulate, which knows no emission."""
    for w, h in ((33, 9), (97, 19)):
        for two in (True, False):
            case = tm.synthetic_case(w, h, two=two)
            case = dict(case, history=case["history"][:5])
            assert (tm.emission(case["aov"], case["aov_spp"]) != 0).any() and (tm.emission(case["history"][3], case["history"][4]) > 1).any()
            want = te.run_case(te.accumulate, case, w, h, te.PARAMS)
            shut = dict(te.PARAMS, emission_tolerance=tm.EMISSION_TOLERANCE, variance_min_history=1)
            stopped = tm.run_case(tm.accumulate_moments, case, w, h, shut, history=case["history"] + (None, None), moments=False)
            assert (stopped[2] != want[2]).any()  # (the case tells the two apart: a stop left on loses taps)
            assert_same(twin_case(hc, case, w, h, te.PARAMS), want)


def test_identity_motion_grows_the_history_to_its_cap(hc):
    """Identity motion, stops that accept (same AOV every frame): frame i (from 1) has len = min(i, max_history) everywhere."""
    w, h, cap = 33, 9, 5
    rng = np.random.default_rng(2)
    aov = te.unit_aov(rng, w * h, 2, np.full(w * h, 2.0))
    aov[::10] = aov[1]  # (every pixel has hits)
    motion = te.identity_motion(w, h)
    prm = dict(max_history=cap, alpha_min=F32(0.01), depth_tolerance=F32(0.1), normal_cos_min=F32(0.9))
    hist = None
    for i in range(1, 9):
        sa, sb = te.random_sums(rng, w * h, extreme=False), te.random_sums(rng, w * h, extreme=False)
        a, b, ln = twin_accumulate(hc, sa, 2, sb, 2, aov, 2, motion, hist, w, h, **prm)
        assert (ln == min(i, cap)).all(), (i, np.unique(ln))
        assert_same((a, b, ln), te.accumulate(sa, 2, sb, 2, aov, 2, motion, hist, w, h, **prm))
        hist = (a, b, ln, aov, 2)


# ----------------------------------------------------------------------------- the motion twin
def _cameras(oracle, aspect):
    cur = default_camera(oracle, aspect)
    moved = oracle.camera((0.56, 0.52, 1.46), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8, aspect)
    return cur, moved


def test_motion_twin_equals_the_restatement_on_real_hits(hc, oracle):
    w, h = 64, 48
    osc = oracle_scene(oracle, "full_bsdf", True)
    cur, moved = _cameras(oracle, w / h)
    o, d = te.centre_rays(oracle, cur, w, h)
    tri, _, u, v = osc.trace_closest(o, d, np.full(w * h, te.FLT_MAX, np.float32))
    prev_moved = te.moved_arrays(osc.arrays, (0.03, 0.0, -0.02)).tris
    for prev_cam, prev_tris in ((cur, osc.arrays.tris), (moved, osc.arrays.tris), (moved, prev_moved)):
        want = te.motion_records(tri, u, v, prev_tris, prev_cam, w, h)
        assert_same((twin_motion(hc, tri, u, v, prev_tris, prev_cam, w, h),), (want,))
    # the same camera and the same vertices: every hit projects onto its own pixel centre, to within the bound of the next test
    same = te.motion_records(tri, u, v, osc.arrays.tris, cur, w, h)
    hit = tri >= 0
    px, py = np.arange(w * h) % w + 0.5, np.arange(w * h) // w + 0.5
    assert np.abs(same[hit, 0] - px[hit]).max() < 0.01 and np.abs(same[hit, 1] - py[hit]).max() < 0.01
    assert (te.tri_ids(same) == np.where(hit, tri, -1)).all() and (same[~hit, :3] == 0).all()


def projection_bound(cam12, tau, w):
    """The first-order bound on |sx - s * w| for the point X = fl(lookfrom + tau * d), d = camera.get_ray(s, t)'s direction
    (eps = 2^-24, the unit roundoff; R = |A| + |h| + |v| bounds every point of the image rectangle seen from the pinhole;
    kappa = R |m| / |A . m| >= 1, how obliquely a ray may meet the image plane; rho = (|lookfrom| + tau) / tau):
      (i)   d carries at most 8 eps (four vector operations and a normalisation of three); X = lookfrom + tau d is rounded to
            float32 (eps |X| <= eps rho |a|) and a = fl(X - lookfrom) once more (eps |a|): |da| / |a| <= (9 + 2 rho) eps.
      (ii)  m = cross(h, v): two roundings per component against |m| = |h| |v| (h is perpendicular to v): at most 4 eps |m|.  A: eps.
            fl(A . m): three roundings on sums of at most |A| |m|, so relative to A . m at most (1 + 4 + 3) kappa eps; fl(a . m):
            ((9 + 2 rho) + 4 + 3) kappa eps.  With the division, lam carries at most (25 + 2 rho) kappa eps.
      (iii) a * lam has length at most R and carries (9 + 2 rho) + (25 + 2 rho) kappa + 1; the subtraction of A (itself eps |A|)
            one more eps R: |dr| <= (37 + 4 rho) kappa R eps.
      (iv)  fl(r . h) adds 3 eps |r| |h| <= 3 eps R |h|; h . h, the division and the product by w add 5 eps to a quotient of at most 1.
    Together |sx - s w| <= w eps ((40 + 4 rho) kappa R / |h| + 5), and the same for sy with v and h exchanged.  Second-order terms
    are below 10^-5 of it."""
    c = np.asarray(cam12, np.float64)
    lf, A, hz, vt = c[0:3], c[3:6] - c[0:3], c[6:9], c[9:12]
    m = np.cross(hz, vt)
    R = np.linalg.norm(A) + np.linalg.norm(hz) + np.linalg.norm(vt)
    kappa = R * np.linalg.norm(m) / abs(A @ m)
    rho = (np.linalg.norm(lf) + tau) / tau
    eps = 2.0 ** -24
    return w * eps * ((40 + 4 * rho) * kappa * R / min(np.linalg.norm(hz), np.linalg.norm(vt)) + 5) * 1.00001


def test_projection_returns_the_image_point_of_a_camera_ray(hc, oracle):
    w, h = 192, 144
    rng = np.random.default_rng(9)
    worst = 0.0
    for cam in (default_camera(oracle, w / h), ae.wide_camera(oracle.camera, w / h), oracle.camera((3.0, -2.0, 0.5), (0.1, 0.4, -0.3), (0.2, 1.0, 0.1), 20.0, 1.0)):
        for tau in (0.05, 1.7, 40.0):
            st = rng.uniform(0, 1, (200, 2)).astype(np.float32)
            st[:4] = ((0, 0), (1, 1), (0.5, 0.5), (1, 0))
            X = np.zeros((200, 3), np.float32)
            for k, (s, t) in enumerate(st):
                r = oracle.camera_get_ray(cam, float(s), float(t)).astype(np.float64)
                X[k] = (r[:3] + tau * r[3:]).astype(np.float32)
            # a triangle per point with the point as its first vertex: (u, v) = (0, 0) gives P = (q0 - e1 * 0) + e2 * 0 = q0 exactly
            tris = np.concatenate([X, X + F32(1), X - F32(1)], axis=1).astype(np.float32)
            rec = twin_motion(hc, np.arange(200), np.zeros(200), np.zeros(200), tris, cam, w, h)
            bound = projection_bound(cam, tau, max(w, h))
            err = max(np.abs(rec[:, 0].astype(np.float64) - st[:, 0].astype(np.float64) * w).max(),
                      np.abs(rec[:, 1].astype(np.float64) - st[:, 1].astype(np.float64) * h).max())
            worst = max(worst, err / bound)
            assert err <= bound, (tau, err, bound)
            assert np.abs(rec[:, 2] - tau).max() <= 16 * 2.0 ** -24 * (tau + np.linalg.norm(cam[:3]))
            assert_same((rec,), (te.motion_records(np.arange(200), np.zeros(200), np.zeros(200), tris, cam, w, h),))
    print("largest error / bound:", worst)


def test_a_point_behind_the_previous_camera_gives_minus_one(hc, oracle):
    cam = default_camera(oracle, 1.0)  # at z = 1.5, looking down -z
    X = np.array([[0.5, 0.5, 2.5], [0.5, 0.5, 1.5], [0.4, 0.6, 1.0], [9.0, 0.5, 1.5]], np.float32)  # behind, at the pinhole, in front, beside
    tris = np.concatenate([X, X + F32(1), X - F32(1)], axis=1)
    rec = twin_motion(hc, np.arange(4), np.zeros(4), np.zeros(4), tris, cam, 8, 8)
    assert rec[0, :2].tolist() == [-1, -1] and rec[0, 2] == 1.0
    assert rec[1, :2].tolist() == [-1, -1] and rec[1, 2] == 0.0  # lam = A.m / 0 = inf, or NaN: not positive and finite
    assert (rec[2, :2] != -1).all() and 0 < rec[2, 0] < 8
    assert rec[3, :2].tolist() == [-1, -1]  # in the pinhole's plane: a . m = 0
    assert_same((rec,), (te.motion_records(np.arange(4), np.zeros(4), np.zeros(4), tris, cam, 8, 8),))
    miss = twin_motion(hc, [-1, -5], np.zeros(2), np.zeros(2), tris, cam, 8, 8)
    assert (miss[:, :3] == 0).all() and (te.tri_ids(miss) == -1).all()


# ----------------------------------------------------------------------------- the surface
def test_new_entry_points_are_declared_exported_bound_and_built(api):
    header = open(os.path.join(ROOT, "include", "rtcuda_amd.h")).read()
    for name in NEW:
        assert name in api.EXPORTS
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert getattr(api.lib(), name).argtypes is not None
    assert "typedef struct rt_temporal_params {" in header
    assert ctypes.sizeof(api.RtTemporalParams) == 20
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bT {name}$", syms, re.M), name
    all_syms = subprocess.run(["nm", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for kernel in ("k_motionIL", "k_temporal_accumulate"):
        assert re.search(rf" _Z\d+{kernel}", all_syms), kernel
    assert callable(api.Scene.render_motion) and callable(api.temporal_accumulate)
    d = api.temporal_default_params()
    assert d["max_history"] >= 1 and 0 < d["alpha_min"] <= 1 and d["depth_tolerance"] > 0 and -1 <= d["normal_cos_min"] <= 1
    hpp = open(os.path.join(ROOT, "include", "rtcuda", "rtcuda.hpp")).read()
    assert "render_motion(" in hpp and "inline void temporal_accumulate(" in hpp and "temporal_default_params()" in hpp


def test_accumulate_errors_name_the_entry_point_and_write_nothing(api, hc):
    """Every refusal comes before a device is needed: host arrays stand in for the device buffers and stay as they were."""
    L = api.lib()
    n = 4
    i64 = lambda ch: np.full(ch * n + 2, 7, np.int64)  # noqa: E731
    sa, sb, aov, ha, hb, pa, oa, ob = i64(3), i64(3), i64(11), i64(3), i64(3), i64(11), i64(3), i64(3)
    ln, ol = np.full(n + 4, 7, np.int32), np.full(n + 4, 7, np.int32)
    mo_store = np.full(4 * n + 8, 7, np.float32)
    mo = (mo_store.ctypes.data + 15) // 16 * 16
    good = dict(max_history=4, alpha_min=0.5, depth_tolerance=0.1, normal_cos_min=0.5, flags=0)
    P = lambda a: a.ctypes.data  # noqa: E731

    def call(a=P(sa), na=1, b=P(sb), nb=1, v=P(aov), nv=1, m=mo, hia=P(ha), hib=P(hb), li=P(ln), pv=P(pa), npv=1, w=2, h=2, o_a=P(oa), o_b=P(ob),
             o_l=P(ol), prm=True, **over):
        p = api.RtTemporalParams(**dict(good, **over))
        rc = L.rt_temporal_accumulate_fixed(a, na, b, nb, v, nv, m, hia, hib, li, pv, npv, w, h, ctypes.byref(p) if prm else None, o_a, o_b, o_l, None)
        return rc, L.rt_last_error().decode()

    inf, nan = float("inf"), float("nan")
    cases = [
        (dict(a=None), "null d_sum_a"), (dict(v=None), "null d_aov_fixed"), (dict(m=None), "null d_motion"), (dict(o_a=None), "null d_hist_a_out"),
        (dict(o_l=None), "null d_len_out"), (dict(w=0), "width and height"), (dict(h=-1), "width and height"),
        (dict(w=1 << 20, h=1 << 10), "more than 715827882 pixels"), (dict(na=0), "must be at least 1"), (dict(nb=0), "must be at least 1"),
        (dict(nv=-2), "must be at least 1"), (dict(npv=0), "prev_aov_samples must be at least 1"),
        (dict(b=None), "d_sum_b and d_hist_b_out must be null together"), (dict(o_b=None), "d_sum_b and d_hist_b_out must be null together"),
        (dict(hib=None), "d_sum_b and d_hist_b_in must be null together"), (dict(b=None, o_b=None), "d_sum_b and d_hist_b_in must be null together"),
        (dict(hia=None), "must be all null or all set"), (dict(li=None), "must be all null or all set"), (dict(pv=None), "must be all null or all set"),
        (dict(hia=None, hib=None, li=None), "must be all null or all set"),
        (dict(m=mo + 4), "d_motion must be 16-byte aligned"), (dict(flags=2), "flags must be 0"),
        (dict(max_history=0), "max_history must be at least 1"), (dict(max_history=-3), "max_history must be at least 1"),
        (dict(alpha_min=0.0), "alpha_min must be in (0, 1]"), (dict(alpha_min=1.5), "alpha_min must be in (0, 1]"), (dict(alpha_min=nan), "alpha_min must be"),
        (dict(depth_tolerance=0.0), "depth_tolerance must be finite and positive"), (dict(depth_tolerance=inf), "depth_tolerance must be finite"),
        (dict(depth_tolerance=nan), "depth_tolerance must be finite"), (dict(normal_cos_min=1.5), "normal_cos_min must be in [-1, 1]"),
        (dict(normal_cos_min=-1.5), "normal_cos_min must be in"), (dict(normal_cos_min=nan), "normal_cos_min must be in"),
        (dict(o_a=P(ha)), "d_hist_a_out overlaps d_hist_a_in"), (dict(o_a=P(sa) + 8), "d_hist_a_out overlaps d_sum_a"),
        (dict(o_b=P(hb)), "d_hist_b_out overlaps d_hist_b_in"), (dict(o_l=P(ln)), "d_len_out overlaps d_len_in"),
        (dict(o_l=P(aov) + 80), "d_len_out overlaps d_aov_fixed"), (dict(o_a=P(pa)), "d_hist_a_out overlaps d_prev_aov_fixed"),
        (dict(o_b=mo), "d_hist_b_out overlaps d_motion"), (dict(o_b=P(oa) + 16), "d_hist_a_out overlaps d_hist_b_out"),
        (dict(o_l=P(oa) + 4 * 3 * 8 - 4), "d_hist_a_out overlaps d_len_out"),
        (dict(w=1, h=715827882), "needs more than 16777215 workgroups"),
    ]
    for over, text in cases:
        rc, msg = call(**over)
        assert rc != 0 and msg.startswith("rt_temporal_accumulate_fixed: ") and text in msg, (over, msg)
    assert L.rt_temporal_default_params(None) != 0
    assert L.rt_last_error().decode() == "rt_temporal_default_params: null out"
    for a in (sa, sb, aov, ha, hb, pa, oa, ob, ln, ol, mo_store):
        assert (a == 7).all()
    # the twin refuses the same parameters
    case = te.synthetic_case(3, 2)
    for kw in (dict(max_history=0), dict(alpha_min=0.0), dict(alpha_min=2.0), dict(depth_tolerance=nan), dict(normal_cos_min=-2.0)):
        out = twin_accumulate(hc, case["sum_a"], 2, case["sum_b"], 2, case["aov"], 4, case["motion"], case["history"], 3, 2, expect_rc=1, **dict(te.PARAMS, **kw))
        assert (out[0] == -7).all() and (out[1] == -7).all() and (out[2] == -7).all()


def test_motion_errors_name_the_entry_point_and_write_nothing(api):
    """The refusals that need no scene and no device: host arrays stand in for the device buffer."""
    L = api.lib()
    cam = api.make_camera()
    out = np.full(64, 7, np.float32)
    op = (out.ctypes.data + 15) // 16 * 16
    fake_scene = ctypes.c_void_p(0)
    rc = L.rt_render_motion(fake_scene, cam.ctypes.data, 2, 2, cam.ctypes.data, None, 0, op, None, None)
    assert rc != 0 and L.rt_last_error().decode() == "rt_render_motion: null scene"
    assert (out == 7).all()


def test_wrapper_rejects_bad_arguments_before_reaching_the_library(api):
    torch = pytest.importorskip("torch")

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    def gpu(x):
        return x.as_subclass(OnGpu)

    a, b, v = (gpu(torch.zeros(8, 3, dtype=torch.int64)), gpu(torch.zeros(8, 3, dtype=torch.int64)), gpu(torch.zeros(8, 11, dtype=torch.int64)))
    m = gpu(torch.zeros(8, 4))
    f = api.temporal_accumulate
    cases = [
        ("temporal_accumulate: beauty_a must be a torch tensor on a GPU", lambda: f(torch.zeros(8, 3, dtype=torch.int64), 1, b, 1, v, 1, m, None, 4, 2)),
        (r"temporal_accumulate: aov_sums must be a contiguous \(8, 11\) torch.int64", lambda: f(a, 1, b, 1, gpu(torch.zeros(8, 10, dtype=torch.int64)), 1, m, None, 4, 2)),
        ("temporal_accumulate: spp_a must be a positive int", lambda: f(a, 0, b, 1, v, 1, m, None, 4, 2)),
        ("temporal_accumulate: spp_b must be a positive int", lambda: f(a, 1, b, 0, v, 1, m, None, 4, 2)),
        ("temporal_accumulate: motion must be a contiguous", lambda: f(a, 1, b, 1, v, 1, gpu(torch.zeros(8, 3)), None, 4, 2)),
        ("temporal_accumulate: history must be None or", lambda: f(a, 1, b, 1, v, 1, m, (a, b), 4, 2)),
        ("temporal_accumulate: history's hist_b and beauty_b must be None together", lambda: f(a, 1, None, 1, v, 1, m, (a, b, None, v, 1), 4, 2)),
        ("temporal_accumulate: max_history must be an int in 1", lambda: f(a, 1, b, 1, v, 1, m, None, 4, 2, max_history=0)),
        ("temporal_accumulate: alpha_min must be a finite number", lambda: f(a, 1, b, 1, v, 1, m, None, 4, 2, alpha_min=float("nan"))),
        ("temporal_accumulate: out must be", lambda: f(a, 1, b, 1, v, 1, m, None, 4, 2, out=(a, None, None))),
    ]
    for pattern, call in cases:
        with pytest.raises(api.RtError, match=pattern):
            call()


def test_defaults_are_the_sweeps_and_the_librarys(api):
    import json
    q = json.load(open(os.path.join(ROOT, "profiles", "temporal_quality.json")))
    assert api.temporal_default_params() == {k: (int(v) if k == "max_history" else float(v)) for k, v in q["defaults"].items()}
    assert [(s["name"], s["width"], s["height"]) for s in q["sequences"]] == [("orbit", 64, 48), ("bunny", 64, 48), ("orbit", 192, 144), ("bunny", 192, 144)]
    assert q["frames_per_sequence"] == 8 and q["spp_per_frame"] == 4 and q["reference_spp"] == 1024
    assert q["default_score"] <= q["table"][0]["score"] * 1.0001 and all(q["default_sequences"][k]["both_rms"] < 1 for k in (0, 1))
    assert all(0 < s["kept"] < 1 for s in q["default_sequences"])
