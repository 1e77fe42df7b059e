"""CPU tests of rt_temporal_accumulate_moments_fixed: the CPU twin (hc_temporal_accumulate_moments of librt_hostcheck.so: a serial
loop over rtcuda_amd/csrc/rt_temporal.h, the kernel's arithmetic) is held to the numpy restatement of the header's text
(tests/temporal_moments_expected.py) bit for bit; the stops' equalities, the window where only the centre counts and the reduction
to rt_temporal_accumulate_fixed are shown; the entry point is declared / exported / bound / refuses bad arguments.  Everything
that runs a kernel is in tests/test_gpu_temporal_moments.py."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import temporal_expected as te
import temporal_moments_expected as tm

F32 = np.float32
NEW = ("rt_temporal_moments_default_params", "rt_temporal_accumulate_moments_fixed")
POISON = -7


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


@pytest.fixture(scope="module")
def hc(api):
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.hc_temporal_accumulate_moments.argtypes = [vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, ci, ci, ci, cf, cf, cf, cf, ci, vp, vp, vp, vp, vp]
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data


def twin(hc, sum_a, spp_a, sum_b, spp_b, aov, aov_spp, motion, history, w, h, max_history, alpha_min, depth_tolerance, normal_cos_min,
         emission_tolerance, variance_min_history, moments=True, expect_rc=0):
    n = w * h
    c64 = lambda a: None if a is None else np.ascontiguousarray(a, np.int64)  # noqa: E731
    c32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
    sum_a, sum_b, aov, motion = c64(sum_a), c64(sum_b), c64(aov), c32(motion)
    ha = hb = ln = pa = pm = mi = None
    ps = 1
    if history is not None:
        ha, hb, ln, pa, ps = c64(history[0]), c64(history[1]), np.ascontiguousarray(history[2], np.int32), c64(history[3]), history[4]
        pm, mi = c32(history[5]), c32(history[6]) if moments else None
    out_a = np.full((n, 3), POISON, np.int64)
    out_b = None if sum_b is None else np.full((n, 3), POISON, np.int64)
    out_len = np.full(n, POISON, np.int32)
    out_m = np.full((n, 4), POISON, np.float32) if moments else None
    out_v = np.full(n, POISON, np.float32) if moments else None
    rc = hc.hc_temporal_accumulate_moments(_ptr(sum_a), spp_a, _ptr(sum_b), spp_b, _ptr(aov), aov_spp, _ptr(motion), _ptr(ha), _ptr(hb), _ptr(ln),
                                           _ptr(pa), ps, _ptr(pm), _ptr(mi), w, h, int(max_history), float(alpha_min), float(depth_tolerance),
                                           float(normal_cos_min), float(emission_tolerance), int(variance_min_history), _ptr(out_a), _ptr(out_b),
                                           _ptr(out_len), _ptr(out_m), _ptr(out_v))
    assert rc == expect_rc
    return out_a, out_b, out_len, out_m, out_v


def twin_case(hc, case, w, h, prm, history="given", **kw):
    return tm.run_case(lambda *a, **k: twin(hc, *a, **k), case, w, h, prm, history, **kw)


def assert_same(got, want):
    assert len(got) == len(want)
    for g, x in zip(got, want):
        if x is None:
            assert g is None
            continue
        g, x = te.bits(g), te.bits(x)
        assert g.shape == x.shape and g.dtype == x.dtype
        bad = np.flatnonzero((g != x).reshape(-1))
        assert bad.size == 0, (bad.size, bad[:5], g.reshape(-1)[bad[:5]], x.reshape(-1)[bad[:5]])


param_sets = tm.param_sets


@pytest.mark.parametrize("w,h", tm.SIZES)
@pytest.mark.parametrize("two", [True, False])
def test_twin_equals_the_restatement(hc, w, h, two):
    case = tm.synthetic_case(w, h, two=two)
    if w * h >= 600:  # the claims of the case: every new branch is taken somewhere
        open_, shut, ids_off = (tm.run_case(tm.accumulate_moments, dict(case, history=case["history"][:5] + k), w, h, dict(tm.PARAMS, emission_tolerance=t))
                                for k, t in ((case["history"][5:], tm.INF), (case["history"][5:], tm.EMISSION_TOLERANCE), ((None, case["history"][6]), tm.INF)))
        assert (open_[2] > 1).sum() > (shut[2] > 1).sum() > 0 and (ids_off[2] > 1).sum() > (open_[2] > 1).sum()
        assert ((shut[2] >= 2) & (shut[4] > 0)).any() and ((shut[2] < 2) & (shut[4] > 0)).any()
    for prm in param_sets():
        assert_same(twin_case(hc, case, w, h, prm), tm.run_case(tm.accumulate_moments, case, w, h, prm))
    # the first frame after the history variants
    for alt, moments in tm.history_variants(case["history"]):
        assert_same(twin_case(hc, case, w, h, tm.PARAMS, history=alt, moments=moments),
                    tm.run_case(tm.accumulate_moments, case, w, h, tm.PARAMS, history=alt, moments=moments))
    for vmh in (1, 2):
        prm = dict(tm.PARAMS, variance_min_history=vmh)
        assert_same(twin_case(hc, case, w, h, prm, history=None), tm.run_case(tm.accumulate_moments, case, w, h, prm, history=None))


def test_emission_and_triangle_stops_on_either_side_of_equality(hc):
    for case, prm, lengths in tm.emission_equality_case():
        want = tm.run_case(tm.accumulate_moments, case, 4, 1, prm)
        assert want[2].tolist() == lengths, (prm, want[2])
        assert_same(twin_case(hc, case, 4, 1, prm), want)


def test_a_window_where_only_the_centre_counts_has_no_variance(hc):
    case, centre = tm.lonely_centre_case()
    prm = dict(tm.PARAMS, variance_min_history=2)
    want = tm.run_case(tm.accumulate_moments, case, 5, 5, prm)
    got = twin_case(hc, case, 5, 5, prm)
    assert_same(got, want)
    assert got[4][centre] == 0 and got[3][centre, 3] > 0 and (got[4] > 0).sum() >= 20 and (got[2] == 1).all()


def test_variance_is_finite_not_negative_and_shrinks_with_the_length(hc):
    w, h = 33, 9
    case = tm.synthetic_case(w, h)
    for prm in param_sets():
        got = twin_case(hc, case, w, h, prm)
        assert np.isfinite(got[4]).all() and (got[4] >= 0).all() and np.isfinite(got[3]).all()
    # the spatial estimate divides by the length: the same frame with a longer history has the smaller variance
    spatial = dict(tm.PARAMS, variance_min_history=tm.PARAMS["max_history"] + 1)
    a = twin_case(hc, case, w, h, spatial)
    first = twin_case(hc, case, w, h, spatial, history=None)
    longer = a[2] > 1
    assert longer.any() and np.array_equal(a[4][longer], (first[4][longer] / a[2][longer].astype(F32)).astype(F32))


@pytest.mark.parametrize("two", [True, False])
def test_with_the_new_features_off_it_is_the_old_accumulator(hc, two):
    """emission_tolerance = +inf, no previous motion, no moments: hist_a, hist_b and len are temporal_expected.accumulate's."""
    for w, h in tm.SIZES:
        case = te.synthetic_case(w, h, two=two)
        for prm in (te.PARAMS, dict(te.PARAMS, max_history=1), dict(te.PARAMS, normal_cos_min=F32(-1.0), depth_tolerance=F32(1e30))):
            want = te.run_case(te.accumulate, case, w, h, prm)
            off = dict(prm, emission_tolerance=tm.INF, variance_min_history=1)
            got = twin_case(hc, case, w, h, off, history=case["history"] + (None, None), moments=False)
            assert got[3] is None and got[4] is None
            assert_same(got[:3], want)
            assert_same(tm.run_case(tm.accumulate_moments, case, w, h, off, history=case["history"] + (None, None), moments=False)[:3], want)
        assert_same(twin_case(hc, case, w, h, dict(te.PARAMS, emission_tolerance=tm.INF, variance_min_history=1), history=None, moments=False)[:3],
                    te.run_case(te.accumulate, case, w, h, te.PARAMS, history=None))


def test_moments_do_not_change_the_colours(hc):
    w, h = 33, 9
    case = tm.synthetic_case(w, h)
    assert_same(twin_case(hc, case, w, h, tm.PARAMS, moments=False)[:3], twin_case(hc, case, w, h, tm.PARAMS)[:3])


# ----------------------------------------------------------------------------- the surface
def test_new_entry_points_are_declared_exported_bound_and_built(api):
    header = open(os.path.join(ROOT, "include", "rtcuda_amd.h")).read()
    for name in NEW:
        assert name in api.EXPORTS
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert getattr(api.lib(), name).argtypes is not None
    assert "typedef struct rt_temporal_moments_params {" in header
    assert ctypes.sizeof(api.RtTemporalMomentsParams) == 28
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bT {name}$", syms, re.M), name
    all_syms = subprocess.run(["nm", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" _Z\d+k_temporal_accumulate_moments", all_syms)
    assert callable(api.temporal_accumulate_moments)
    hpp = open(os.path.join(ROOT, "include", "rtcuda", "rtcuda.hpp")).read()
    assert "inline void temporal_accumulate_moments(" in hpp and "temporal_moments_default_params()" in hpp


def test_defaults_are_the_sweeps_and_the_librarys(api):
    d = api.temporal_moments_default_params()
    assert d["max_history"] >= 1 and 0 < d["alpha_min"] <= 1 and d["depth_tolerance"] > 0 and -1 <= d["normal_cos_min"] <= 1
    assert d["emission_tolerance"] >= 0 and d["variance_min_history"] >= 1
    q = json.load(open(os.path.join(ROOT, "profiles", "temporal_moments_quality.json")))
    assert {k: float(v) for k, v in d.items()} == {k: float(v) for k, v in q["defaults"].items()}


def test_errors_name_the_entry_point_and_write_nothing(api, hc):
    """Every refusal comes before a device is needed: host arrays stand in for the device buffers and stay as they were."""
    L = api.lib()
    n = 4
    i64 = lambda ch: np.full(ch * n + 2, 7, np.int64)  # noqa: E731
    sa, sb, aov, ha, hb, pa, oa, ob = i64(3), i64(3), i64(11), i64(3), i64(3), i64(11), i64(3), i64(3)
    ln, ol, ov = np.full(n + 4, 7, np.int32), np.full(n + 4, 7, np.int32), np.full(n + 4, 7, np.float32)
    stores = [np.full(4 * n + 8, 7, np.float32) for _ in range(4)]
    mo, pm, mi, om = ((s.ctypes.data + 15) // 16 * 16 for s in stores)
    good = dict(max_history=4, alpha_min=0.5, depth_tolerance=0.1, normal_cos_min=0.5, emission_tolerance=0.25, variance_min_history=2, flags=0)
    P = lambda a: a.ctypes.data  # noqa: E731

    def call(a=P(sa), na=1, b=P(sb), nb=1, v=P(aov), nv=1, m=mo, hia=P(ha), hib=P(hb), li=P(ln), pv=P(pa), npv=1, pmo=pm, min_=mi, w=2, h=2,
             o_a=P(oa), o_b=P(ob), o_l=P(ol), o_m=om, o_v=P(ov), **over):
        p = api.RtTemporalMomentsParams(**dict(good, **over))
        rc = L.rt_temporal_accumulate_moments_fixed(a, na, b, nb, v, nv, m, hia, hib, li, pv, npv, pmo, min_, w, h, ctypes.byref(p), o_a, o_b, o_l,
                                                    o_m, o_v, None)
        return rc, L.rt_last_error().decode()

    inf, nan = float("inf"), float("nan")
    first = dict(hia=None, hib=None, li=None, pv=None)
    cases = [
        (dict(a=None), "null d_sum_a"), (dict(o_l=None), "null d_len_out"), (dict(w=0), "width and height"), (dict(na=0), "must be at least 1"),
        (dict(b=None), "d_sum_b and d_hist_b_out must be null together"), (dict(li=None), "must be all null or all set"),
        (dict(first, pmo=None), "d_moments_in and d_prev_motion may be set only when history is given"),
        (dict(first, min_=None), "d_moments_in and d_prev_motion may be set only when history is given"),
        (dict(o_v=None), "d_moments_out and d_variance_out must be null together"), (dict(o_m=None), "d_moments_out and d_variance_out must be null together"),
        (dict(o_m=None, o_v=None), "d_moments_in needs d_moments_out"), (dict(na=0x7fffffff, nb=1), "samples_a + samples_b must fit an int32"),
        (dict(m=mo + 4), "d_motion must be 16-byte aligned"), (dict(pmo=pm + 8), "d_prev_motion must be 16-byte aligned"),
        (dict(min_=mi + 4), "d_moments_in must be 16-byte aligned"), (dict(o_m=om + 12), "d_moments_out must be 16-byte aligned"),
        (dict(flags=1), "flags must be 0"), (dict(max_history=0), "max_history must be at least 1"), (dict(alpha_min=nan), "alpha_min must be"),
        (dict(depth_tolerance=inf), "depth_tolerance must be finite"), (dict(normal_cos_min=2.0), "normal_cos_min must be in"),
        (dict(emission_tolerance=nan), "emission_tolerance must be at least 0"), (dict(emission_tolerance=-0.5), "emission_tolerance must be at least 0"),
        (dict(variance_min_history=0), "variance_min_history must be at least 1, it is 0"), (dict(variance_min_history=-4), "variance_min_history must be at least 1"),
        (dict(o_v=P(ln)), "d_variance_out overlaps d_len_in"), (dict(o_v=mi + 32), "d_variance_out overlaps d_moments_in"),
        (dict(o_m=pm), "d_moments_out overlaps d_prev_motion"), (dict(o_m=mo), "d_moments_out overlaps d_motion"),
        (dict(o_a=mi), "d_hist_a_out overlaps d_moments_in"), (dict(o_v=om + 16), "d_moments_out overlaps d_variance_out"),
        (dict(o_l=P(ov)), "d_len_out overlaps d_variance_out"), (dict(o_a=P(ha)), "d_hist_a_out overlaps d_hist_a_in"),
        (dict(w=1, h=715827882), "needs more than 16777215 workgroups"),
    ]
    for over, text in cases:
        rc, msg = call(**over)
        assert rc != 0 and msg.startswith("rt_temporal_accumulate_moments_fixed: ") and text in msg, (over, msg)
    assert L.rt_temporal_moments_default_params(None) != 0
    assert L.rt_last_error().decode() == "rt_temporal_moments_default_params: null out"
    for a in [sa, sb, aov, ha, hb, pa, oa, ob, ln, ol, ov] + stores:
        assert (a == 7).all()
    # the twin refuses the same parameters
    case = tm.synthetic_case(3, 2)
    for kw in (dict(max_history=0), dict(emission_tolerance=nan), dict(emission_tolerance=-1.0), dict(variance_min_history=0)):
        out = twin_case(hc, case, 3, 2, dict(tm.PARAMS, **kw), expect_rc=1)
        assert all((o == POISON).all() for o in out)


def test_wrapper_rejects_bad_arguments_before_reaching_the_library(api):
    torch = pytest.importorskip("torch")

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    def gpu(x):
        return x.as_subclass(OnGpu)

    a, v = gpu(torch.zeros(8, 3, dtype=torch.int64)), gpu(torch.zeros(8, 11, dtype=torch.int64))
    m, ln = gpu(torch.zeros(8, 4)), gpu(torch.zeros(8, dtype=torch.int32))
    f = api.temporal_accumulate_moments
    cases = [
        ("temporal_accumulate_moments: beauty_a must be a torch tensor on a GPU", lambda: f(torch.zeros(8, 3, dtype=torch.int64), 1, None, 0, v, 1, m, None, 4, 2)),
        ("temporal_accumulate_moments: history must be None or", lambda: f(a, 1, None, 0, v, 1, m, (a, None, ln, v, 1), 4, 2)),
        ("temporal_accumulate_moments: history's prev_moments needs moments=True", lambda: f(a, 1, None, 0, v, 1, m, (a, None, ln, v, 1, None, m), 4, 2, moments=False)),
        ("temporal_accumulate_moments: history prev_motion must be a contiguous", lambda: f(a, 1, None, 0, v, 1, m, (a, None, ln, v, 1, gpu(torch.zeros(8, 3)), None), 4, 2)),
        ("temporal_accumulate_moments: variance_min_history must be an int in 1", lambda: f(a, 1, None, 0, v, 1, m, None, 4, 2, variance_min_history=0)),
        ("temporal_accumulate_moments: emission_tolerance must be a number", lambda: f(a, 1, None, 0, v, 1, m, None, 4, 2, emission_tolerance="x")),
        ("temporal_accumulate_moments: out must be", lambda: f(a, 1, None, 0, v, 1, m, None, 4, 2, out=(a, None, ln))),
    ]
    for pattern, call in cases:
        with pytest.raises(api.RtError, match=pattern):
            call()
