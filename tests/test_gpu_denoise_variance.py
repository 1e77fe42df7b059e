"""GPU tests of rt_denoise_variance_fixed (through api.denoise_variance).  Run with -m gpu.

What the call must return comes from tests/temporal_moments_expected.py, the numpy restatement of the header's text that
tests/test_denoise_variance_host.py holds the CPU twin to.  Every comparison of an image is EQUALITY of all output floats as bit
patterns.  The passes are rt_denoise_dual_fixed's own kernels; new here is k_dn_prepare_var in front of them and k_dn_finish
behind them.  With the defaults (3 passes) strides 1 and 2 run the LDS form and stride 4 the direct form; the knob RT_DENOISE_FORM
forces each form at every stride."""
import ctypes

import numpy as np
import pytest

import denoise_expected as de
import denoise_dual_expected as dd
import temporal_moments_expected as tm

pytestmark = pytest.mark.gpu

F32 = np.float32
OTHER = dict(sigma_variance=F32(1.5), sigma_depth=F32(0.3), normal_power_log2=3)
SIZES = [(1, 1), (5, 5), (33, 17), (97, 19)]
POISON = -7.0


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()  # raises if the HIP library is missing: there is no fallback
    return _api


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    return _torch


_expected = {}


def _frame(w, h):
    """(beauty, spp, wild variance, aov, aov_spp), made once per session and never modified."""
    k = ("frame", w, h)
    if k not in _expected:
        beauty, spp, aov, aov_spp = de.synthetic_frame(w, h)
        n = w * h
        v = np.exp2(np.random.default_rng(4 + n).uniform(-140, 100, n)).astype(np.float32)
        special = np.array([np.nan, -1.0, np.inf, 2.0 ** 100, 0.0, -0.0, -np.inf, 2.0 ** 87], np.float32)
        v[:min(n, special.size)] = special[:n]
        _expected[k] = (beauty, spp, v, aov, aov_spp)
        for t in _expected[k]:
            if isinstance(t, np.ndarray):
                t.setflags(write=False)
    return _expected[k]


def _want(w, h, **prm):
    k = (w, h, tuple(sorted((n, float(v)) for n, v in prm.items())))
    if k not in _expected:
        _expected[k] = tm.denoise_variance(*_frame(w, h), w, h, **prm)
        _expected[k].setflags(write=False)
    return _expected[k]


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()  # (the session's frames are read-only)


def _prm(kw):
    return {k: (float(v) if k.startswith("sigma") else v) for k, v in kw.items()}


def _run(api, torch, frame, w, h, **kw):
    beauty, spp, v, aov, aov_spp = frame
    out = torch.full((w * h, 3), POISON, dtype=torch.float32, device="cuda")
    got = api.denoise_variance(_dev(torch, beauty), int(spp), _dev(torch, v), _dev(torch, aov), int(aov_spp), w, h, out=out, **_prm(kw))
    assert got is out
    return got


def _assert_same_bits(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    g, w = dd.bits(got), dd.bits(want)
    assert g.shape == w.shape
    bad = g != w
    print(what, "floats that differ:", int(bad.sum()), "of", bad.size)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[bad][:6].tolist(), np.asarray(want)[bad][:6].tolist())


@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_sizes_and_pass_counts_equal_the_restatement(api, torch, w, h):
    """Variances over the whole range of the format, a NaN, negatives, infinities and 2^100 among them."""
    _assert_same_bits(_run(api, torch, _frame(w, h), w, h), _want(w, h), ("defaults", w, h))
    for passes in (0, 1, 3, 8):
        prm = dict(OTHER, passes=passes)
        _assert_same_bits(_run(api, torch, _frame(w, h), w, h, **prm), _want(w, h, **prm), (passes, w, h))


@pytest.mark.parametrize("form", [1, 2], ids=["direct", "lds"])
def test_each_pass_form_forced(api, torch, monkeypatch, form):
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "1")
    monkeypatch.setenv("RT_DENOISE_FORM", str(form))
    prm = dict(OTHER, passes=3)
    for w, h in ((33, 17), (97, 19)):
        _assert_same_bits(_run(api, torch, _frame(w, h), w, h, **prm), _want(w, h, **prm), (form, w, h))


@pytest.mark.parametrize("passes", [0, 1, 3])
def test_with_the_dual_filters_own_variance_it_is_rt_denoise_dual_fixed(api, torch, passes):
    """Two GPU calls compared with each other: denoise_dual on two halves against denoise_variance on their wrapped sum and the
    step-2 variance of the dual restatement."""
    for w, h in ((33, 17), (97, 19)):
        for halves in (dd.split_frame(de.synthetic_frame(w, h), 3, 1), dd.extreme_halves(w, h)):
            a, spp_a, b, spp_b, aov, aov_spp = halves
            kv = dd.pass_constants(OTHER["sigma_variance"], OTHER["sigma_depth"], spp_a, spp_b)[2]
            v = dd.prepare_dual(a, spp_a, b, spp_b, aov, aov_spp, kv)[1]
            prm = _prm(dict(OTHER, passes=passes))
            dual = api.denoise_dual(_dev(torch, a), spp_a, _dev(torch, b), spp_b, _dev(torch, aov), aov_spp, w, h, **prm)
            one = api.denoise_variance(_dev(torch, dd.wrapped_sum(a, b)), spp_a + spp_b, _dev(torch, v), _dev(torch, aov), aov_spp, w, h, **prm)
            _assert_same_bits(one, dual.cpu().numpy(), ("identity", passes, w, h))


def test_inputs_are_only_read_scratch_reuse_and_side_stream(api, torch):
    w, h = 97, 19
    beauty, spp, v, aov, aov_spp = _frame(w, h)
    db, dv, da = _dev(torch, beauty), _dev(torch, v), _dev(torch, aov)
    scratch = torch.full((api.denoise_dual_scratch_bytes(w, h),), 0xA5, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(2):
        out = torch.full((w * h, 3), POISON, dtype=torch.float32, device="cuda")
        got = api.denoise_variance(db, spp, dv, da, aov_spp, w, h, scratch=scratch, out=out, stream=side)
        _assert_same_bits(got, _want(w, h), "side stream, reused scratch")
    assert np.array_equal(db.cpu().numpy(), beauty) and np.array_equal(da.cpu().numpy(), aov)
    assert np.array_equal(dd.bits(dv.cpu().numpy()), dd.bits(v))


def test_bad_arguments_with_device_buffers_write_nothing(api, torch):
    w, h = 5, 5
    beauty, spp, v, aov, aov_spp = _frame(w, h)
    db, dv, da = _dev(torch, beauty), _dev(torch, v), _dev(torch, aov)
    out = torch.full((w * h, 3), POISON, dtype=torch.float32, device="cuda")
    scratch = torch.full((api.denoise_dual_scratch_bytes(w, h) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(api.RtError, match="rt_denoise_variance_fixed: sigma_variance gives a variance constant"):
        api.denoise_variance(db, spp, dv, da, aov_spp, w, h, out=out, scratch=scratch, sigma_variance=1e30)
    L, c = api.lib(), ctypes.c_void_p
    rc = L.rt_denoise_variance_fixed(c(db.data_ptr()), spp, None, c(da.data_ptr()), aov_spp, w, h, None, c(scratch.data_ptr()), c(out.data_ptr()), None)
    assert rc != 0 and L.rt_last_error().decode() == "rt_denoise_variance_fixed: null d_variance"
    rc = L.rt_denoise_variance_fixed(c(db.data_ptr()), spp, c(dv.data_ptr()), c(da.data_ptr()), aov_spp, w, h, None, c(scratch.data_ptr() + 8), c(out.data_ptr()), None)
    assert rc != 0 and "d_scratch must be 16-byte aligned" in L.rt_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((scratch == 0xA5).all())
