"""CPU tests of rt_denoise_variance_fixed: the CPU twin (hc_denoise_variance of librt_hostcheck.so: hc_denoise_dual's walk over
rtcuda_amd/csrc/rt_denoise.h on one frame and the caller's variance) is held to the numpy restatement of the header's text
(tests/temporal_moments_expected.py) bit for bit; what step 2 makes of a NaN, a negative, an infinite and a huge variance is
shown; fed with rt_denoise_dual_fixed's own step-2 variance it is that filter, bit for bit; the entry point is declared / exported
/ bound / refuses bad arguments.  Everything that runs a kernel is in tests/test_gpu_denoise_variance.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import aov_expected as ae
import denoise_expected as de
import denoise_dual_expected as dd
import temporal_moments_expected as tm

F32 = np.float32
OTHER = dict(sigma_variance=F32(1.5), sigma_depth=F32(0.3))
SIZES = ((1, 1), (2, 3), (33, 17), (97, 19))


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


@pytest.fixture(scope="module")
def hc(api):
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.hc_denoise_variance.argtypes = [vp, ci, vp, vp, ci, ci, ci, ci, cf, cf, ci, vp, vp]
    return L


def twin(hc, beauty, spp, variance, aov, aov_spp, w, h, passes=None, sigma_variance=None, sigma_depth=None, normal_power_log2=None, expect_rc=0,
         with_variance=False):
    dp = dd.default_params()
    beauty, aov, variance = np.ascontiguousarray(beauty, np.int64), np.ascontiguousarray(aov, np.int64), np.ascontiguousarray(variance, np.float32)
    assert beauty.shape == (w * h, 3) and aov.shape == (w * h, ae.CHANNELS) and variance.shape == (w * h,)
    out = np.full((w * h, 3), -7, np.float32)
    var = np.full(w * h, -7, np.float32)
    rc = hc.hc_denoise_variance(beauty.ctypes.data, spp, variance.ctypes.data, aov.ctypes.data, aov_spp, w, h,
                                dp["passes"] if passes is None else passes, dp["sigma_variance"] if sigma_variance is None else sigma_variance,
                                dp["sigma_depth"] if sigma_depth is None else sigma_depth,
                                dp["normal_power_log2"] if normal_power_log2 is None else normal_power_log2, out.ctypes.data, var.ctypes.data)
    assert rc == expect_rc
    return (out, var) if with_variance else out


def assert_same_bits(got, want):
    g, w = dd.bits(got), dd.bits(want)
    assert g.shape == w.shape
    bad = np.flatnonzero((g != w).reshape(-1))
    assert bad.size == 0, (bad.size, bad[:5], np.asarray(got).reshape(-1)[bad[:5]], np.asarray(want).reshape(-1)[bad[:5]])


def wild_variance(n, seed=4):
    """Variances over the whole range of the format, with every value step 2 must mend."""
    rng = np.random.default_rng(seed + n)
    v = np.exp2(rng.uniform(-140, 100, n)).astype(np.float32)  # (denormals, zeros by underflow, values beyond 2^87)
    special = np.array([np.nan, -1.0, np.inf, 2.0 ** 100, 0.0, -0.0, -np.inf, 2.0 ** 87, np.nextafter(F32(2.0 ** 87), F32(0))], np.float32)
    v[:min(n, special.size)] = special[:n]
    return v


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kind", ["synthetic", "extreme"])
def test_twin_equals_the_restatement(hc, kind, w, h):
    beauty, spp, aov, aov_spp = de.synthetic_frame(w, h) if kind == "synthetic" else de.extreme_frame(w, h)
    n = w * h
    for variance in (wild_variance(n), np.random.default_rng(n).uniform(0, 0.05, n).astype(np.float32)):
        for passes in (0, 1, 3, 8):
            want, want_v = tm.denoise_variance(beauty, spp, variance, aov, aov_spp, w, h, passes, normal_power_log2=1, with_variance=True, **OTHER)
            assert np.isfinite(want).all() and np.isfinite(want_v).all() and (want_v >= 0).all()
            got, got_v = twin(hc, beauty, spp, variance, aov, aov_spp, w, h, passes, normal_power_log2=1, with_variance=True, **OTHER)
            assert_same_bits(got, want)
            assert_same_bits(got_v, want_v)
        assert_same_bits(twin(hc, beauty, spp, variance, aov, aov_spp, w, h), tm.denoise_variance(beauty, spp, variance, aov, aov_spp, w, h))


def test_step_2_mends_what_is_not_a_variance(hc):
    """NaN, -1, +inf and 2^100 behave as 0, 0, 2^87 and 2^87: with passes = 0 the variance comes back as step 2 left it, and a
    filtered frame is the frame of the mended buffer, bit for bit."""
    w, h = 33, 17
    n = w * h
    beauty, spp, aov, aov_spp = de.synthetic_frame(w, h)
    bad = np.resize(np.array([np.nan, -1.0, np.inf, 2.0 ** 100], np.float32), n)
    mended = np.resize(np.array([0.0, 0.0, 2.0 ** 87, 2.0 ** 87], np.float32), n)
    assert_same_bits(tm.sanitise(bad), mended)
    _, v0 = twin(hc, beauty, spp, bad, aov, aov_spp, w, h, passes=0, with_variance=True)
    assert_same_bits(v0, mended)
    for passes in (1, 3):
        got, got_v = twin(hc, beauty, spp, bad, aov, aov_spp, w, h, passes=passes, with_variance=True)
        want, want_v = twin(hc, beauty, spp, mended, aov, aov_spp, w, h, passes=passes, with_variance=True)
        assert_same_bits(got, want)
        assert_same_bits(got_v, want_v)
        assert np.isfinite(got).all() and np.isfinite(got_v).all()


@pytest.mark.parametrize("passes", [0, 1, 3])
def test_with_the_dual_filters_own_variance_it_is_the_dual_filter(hc, passes):
    """d_variance = rt_denoise_dual_fixed's step-2 v, sum = a + b, num_samples = samples_a + samples_b: the same output bits."""
    for w, h in ((33, 17), (97, 19)):
        for halves in (dd.split_frame(de.synthetic_frame(w, h), 3, 1), dd.extreme_halves(w, h)):
            a, spp_a, b, spp_b, aov, aov_spp = halves
            kv = dd.pass_constants(OTHER["sigma_variance"], OTHER["sigma_depth"], spp_a, spp_b)[2]
            v = dd.prepare_dual(a, spp_a, b, spp_b, aov, aov_spp, kv)[1]
            assert (v <= tm.VAR_MAX).all() and (v > 0).any()
            want = dd.denoise_dual(*halves, w, h, passes, normal_power_log2=2, **OTHER)
            s = dd.wrapped_sum(a, b)
            assert_same_bits(tm.denoise_variance(s, spp_a + spp_b, v, aov, aov_spp, w, h, passes, normal_power_log2=2, **OTHER), want)
            assert_same_bits(twin(hc, s, spp_a + spp_b, v, aov, aov_spp, w, h, passes, normal_power_log2=2, **OTHER), want)


# ----------------------------------------------------------------------------- the surface
def test_new_entry_point_is_declared_exported_bound_and_built(api):
    header = open(os.path.join(ROOT, "include", "rtcuda_amd.h")).read()
    name = "rt_denoise_variance_fixed"
    assert name in api.EXPORTS and re.search(rf"^int {name}\(", header, re.M)
    assert getattr(api.lib(), name).argtypes is not None
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(rf"\bT {name}$", syms, re.M)
    all_syms = subprocess.run(["nm", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" _Z\d+k_dn_prepare_var", all_syms)
    assert callable(api.denoise_variance)
    assert "inline void denoise_variance(" in open(os.path.join(ROOT, "include", "rtcuda", "rtcuda.hpp")).read()


def test_errors_name_the_entry_point_and_write_nothing(api, hc):
    """Every refusal comes before a device is needed: host arrays stand in for the device buffers and stay as they were."""
    L = api.lib()
    n = 4
    s, aov, var, out = np.full(3 * n, 7, np.int64), np.full(11 * n, 7, np.int64), np.full(n, 7, np.float32), np.full(3 * n, 7, np.float32)
    store = np.full(64 * n, 7, np.uint8)
    scratch = (store.ctypes.data + 15) // 16 * 16
    good = dict(passes=2, sigma_variance=4.0, sigma_depth=0.5, normal_power_log2=1, flags=0)
    P = lambda a: a.ctypes.data  # noqa: E731

    def call(a=P(s), na=1, v=P(var), f=P(aov), nf=1, w=2, h=2, sc=scratch, o=P(out), **over):
        p = api.RtDenoiseDualParams(**dict(good, **over))
        rc = L.rt_denoise_variance_fixed(a, na, v, f, nf, w, h, ctypes.byref(p), sc, o, None)
        return rc, L.rt_last_error().decode()

    nan = float("nan")
    cases = [(dict(a=None), "null d_sum_fixed"), (dict(v=None), "null d_variance"), (dict(f=None), "null d_aov_fixed"), (dict(sc=None), "null d_scratch"),
             (dict(o=None), "null d_rgb_out"), (dict(w=0), "width and height"), (dict(w=1 << 20, h=1 << 10), "more than 715827882 pixels"),
             (dict(na=0), "num_samples and aov_samples must be at least 1"), (dict(nf=-1), "num_samples and aov_samples must be at least 1"),
             (dict(sc=scratch + 8), "d_scratch must be 16-byte aligned"), (dict(flags=4), "flags must be 0"), (dict(passes=9), "passes must be 0 .. 8"),
             (dict(normal_power_log2=-1), "normal_power_log2 must be 0 .. 8"), (dict(sigma_variance=nan), "sigma_variance must be finite and positive"),
             (dict(sigma_variance=1e30), "sigma_variance gives a variance constant"), (dict(sigma_depth=0.0), "sigma_depth must be finite and positive"),
             (dict(sigma_depth=1e-30), "sigma_depth gives a depth constant"), (dict(w=1, h=715827882, passes=1), "needs more than 16777215 workgroups")]
    for over, text in cases:
        rc, msg = call(**over)
        assert rc != 0 and msg.startswith("rt_denoise_variance_fixed: ") and text in msg, (over, msg)
    for a in (s, aov, var, out, store):
        assert (a == 7).all()
    beauty, spp, aov2, aov_spp = de.synthetic_frame(3, 2)
    for kw in (dict(passes=9), dict(sigma_variance=nan), dict(sigma_depth=-1.0), dict(normal_power_log2=9)):
        got = twin(hc, beauty, spp, np.zeros(6, np.float32), aov2, aov_spp, 3, 2, expect_rc=1, **kw)
        assert (got == -7).all()


def test_wrapper_rejects_bad_arguments_before_reaching_the_library(api):
    torch = pytest.importorskip("torch")

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    def gpu(x):
        return x.as_subclass(OnGpu)

    a, v, var = gpu(torch.zeros(8, 3, dtype=torch.int64)), gpu(torch.zeros(8, 11, dtype=torch.int64)), gpu(torch.zeros(8))
    f = api.denoise_variance
    cases = [("denoise_variance: beauty_sums must be a torch tensor on a GPU", lambda: f(torch.zeros(8, 3, dtype=torch.int64), 1, var, v, 1, 4, 2)),
             ("denoise_variance: variance must be a torch tensor on the GPU", lambda: f(a, 1, torch.zeros(8), v, 1, 4, 2)),
             (r"denoise_variance: variance must be a contiguous \(8,\) torch.float32", lambda: f(a, 1, gpu(torch.zeros(8, 1)), v, 1, 4, 2)),
             ("denoise_variance: spp must be a positive int", lambda: f(a, 0, var, v, 1, 4, 2)),
             (r"denoise_variance: passes must be an int in 0 \.\. 8", lambda: f(a, 1, var, v, 1, 4, 2, passes=9)),
             ("denoise_variance: sigma_variance must be a finite positive number", lambda: f(a, 1, var, v, 1, 4, 2, sigma_variance=0.0))]
    for pattern, call in cases:
        with pytest.raises(api.RtError, match=pattern):
            call()
