"""CPU tests of rt_upsample_fixed / rt_upsample_rgb: the CPU twin (hc_upsample of librt_hostcheck.so: a serial loop over
rtcuda_amd/csrc/rt_upsample.h, the arithmetic of the kernel) is held to the numpy restatement of the header's text
(tests/upsample_expected.py) bit for bit, for both input kinds and both outputs, on oracle-rendered frames at the three factors
and on synthetic sums that force each branch; the entry points are declared / exported / bound / refuse bad arguments.  Everything
that runs the kernel is in tests/test_gpu_upsample.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, default_camera, oracle_scene
import aov_expected as ae
import denoise_expected as de
import upsample_expected as ue

F32 = np.float32
ONE = 1 << 30
ORACLE_SIZES = ((8, 6, 2), (5, 4, 3), (4, 3, 4))  # low width, low height, factor: 16 x 12, 15 x 12, 16 x 12
OTHER = dict(sigma_depth=F32(0.3), normal_power_log2=2)


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


@pytest.fixture(scope="module")
def hc(api):
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.hc_upsample.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, vp, ci, cf, ci, vp, vp, vp]
    return L


def twin(hc, low, spp, aov_lo, aov_spp_lo, lw, lh, factor, aov_hi, aov_spp_hi, sigma_depth=None, normal_power_log2=None, expect_rc=0,
         want=("rgb", "fixed")):
    """hc_upsample -> (rgb, fixed, tent mask, shortcut mask); `low`: int64 sums (rt_upsample_fixed) or float32 radiance (rt_upsample_rgb).
    An output that is not in `want` is not handed over (None comes back)."""
    dp = ue.default_params()
    low = np.ascontiguousarray(low)
    is_rgb = low.dtype == np.float32
    assert is_rgb or low.dtype == np.int64
    aov_lo, aov_hi = np.ascontiguousarray(aov_lo, np.int64), np.ascontiguousarray(aov_hi, np.int64)
    n = factor * factor * lw * lh
    assert low.shape == (lw * lh, 3) and aov_lo.shape == (lw * lh, ae.CHANNELS) and aov_hi.shape == (n, ae.CHANNELS)
    rgb, fixed, form = np.full((n, 3), -7, np.float32), np.full((n, 3), -7, np.int64), np.full(n, 9, np.uint8)
    rc = hc.hc_upsample(None if is_rgb else low.ctypes.data, low.ctypes.data if is_rgb else None, 1 if is_rgb else spp, aov_lo.ctypes.data,
                        aov_spp_lo, lw, lh, factor, aov_hi.ctypes.data, aov_spp_hi, dp["sigma_depth"] if sigma_depth is None else sigma_depth,
                        dp["normal_power_log2"] if normal_power_log2 is None else normal_power_log2,
                        rgb.ctypes.data if "rgb" in want else None, fixed.ctypes.data if "fixed" in want else None, form.ctypes.data)
    assert rc == expect_rc
    if rc:
        assert (rgb == -7).all() and (fixed == -7).all() and (form == 9).all()
        return None
    assert ("rgb" in want) or (rgb == -7).all()
    assert ("fixed" in want) or (fixed == -7).all()
    return rgb if "rgb" in want else None, fixed if "fixed" in want else None, form == ue.TENT, form == ue.SHORTCUT


def assert_same_bits(got, want):
    g, w = ue.bits(got), ue.bits(want)
    assert g.shape == w.shape
    bad = np.flatnonzero((g != w).reshape(-1))
    assert bad.size == 0, (bad.size, bad[:5], np.asarray(got).reshape(-1)[bad[:5]], np.asarray(want).reshape(-1)[bad[:5]])


def assert_twin_is_restatement(hc, low, spp, rest, **prm):
    """Both outputs, each alone and together, the masks, and d_out_fixed == to_fixed(d_rgb_out) element for element."""
    is_rgb = np.asarray(low).dtype == np.float32
    want = ue.upsample_rgb(low, *rest, **prm) if is_rgb else ue.upsample(low, spp, *rest, **prm)
    got = twin(hc, low, spp, *rest, **prm)
    assert_same_bits(got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[1], ae.to_fixed(got[0]).reshape(-1, 3))
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert np.isfinite(got[0]).all()
    alone = twin(hc, low, spp, *rest, want=("rgb",), **prm)
    assert_same_bits(alone[0], want[0])
    alone = twin(hc, low, spp, *rest, want=("fixed",), **prm)
    assert np.array_equal(alone[1], want[1])
    return want


# ----------------------------------------------------------------------------- oracle frames
_classes = {}


@pytest.mark.parametrize("lw,lh,factor", ORACLE_SIZES, ids=["x%d" % s[2] for s in ORACLE_SIZES])
def test_twin_equals_the_restatement_on_oracle_frames(hc, oracle, lw, lh, factor):
    osc = oracle_scene(oracle, "full_bsdf", True)
    w, h, spp = factor * lw, factor * lh, 4
    beauty, _, aov_lo, _ = de.real_frame(oracle, osc, default_camera(oracle, lw / lh), lw, lh, spp)
    aov_hi = ae.frame_expected(oracle, osc, default_camera(oracle, w / h), w, h, 2)[0]
    rest = (aov_lo, spp, lw, lh, factor, aov_hi, 2)
    assert int(beauty.sum()) > 0 and ae.frame_census(aov_hi, 2)[0] > w * h // 2
    for prm in ({}, OTHER):
        want = assert_twin_is_restatement(hc, beauty, spp, rest, **prm)
        rgb_lo = de.denoise(beauty, spp, aov_lo, spp, lw, lh)  # a denoiser's output at the low size
        assert_twin_is_restatement(hc, rgb_lo, None, rest, **prm)
        if not prm:
            tent, shortcut = want[2], want[3]
            _classes[factor] = (int((~tent & ~shortcut).sum()), int(tent.sum()), int(shortcut.sum()))
            print("factor", factor, "guided / tent / shortcut pixels:", _classes[factor])


def test_oracle_frames_hold_every_class_of_pixel(hc, oracle):
    """With the defaults: guided pixels, pixels no low tap shares a feature with (the tent form), pixels no sample hit."""
    for lw, lh, factor in ORACLE_SIZES:
        if factor not in _classes:
            test_twin_equals_the_restatement_on_oracle_frames(hc, oracle, lw, lh, factor)
    total = np.sum([_classes[f] for _, _, f in ORACLE_SIZES], axis=0)
    assert (total > 0).all(), _classes


# ----------------------------------------------------------------------------- synthetic sums, one per branch
def flat_aov(n, normal=(0, 0, 1), depth=1.0, hits=1, albedo=1.0, spp=1):
    """n pixels of one surface: `hits` of `spp` samples hit it."""
    aov = np.zeros((n, ae.CHANNELS), np.int64)
    aov[:, ae.ALBEDO:ae.ALBEDO + 3] = int(albedo * ONE) * hits
    aov[:, ae.NORMAL:ae.NORMAL + 3] = np.rint(np.asarray(normal, np.float64) * ONE).astype(np.int64) * hits
    aov[:, ae.DEPTH] = int(depth * ONE) * hits
    aov[:, ae.HITS] = hits
    return aov


def ramp(n):
    b = np.zeros((n, 3), np.int64)
    b[:, 0] = (np.arange(n) + 1) * (ONE // 4)
    b[:, 1] = ONE // 2
    b[:, 2] = ((np.arange(n) * 7) % 5) * (ONE // 8)
    return b


@pytest.mark.parametrize("factor", ue.FACTORS)
def test_synthetic_frames_equal_the_restatement(hc, factor):
    for lw, lh in ((1, 1), (3, 2), (17, 5), (11, 3)):
        beauty, spp, aov_lo, s_lo, aov_hi, s_hi = ue.synthetic_pair(lw, lh, factor)
        rest = (aov_lo, s_lo, lw, lh, factor, aov_hi, s_hi)
        for prm in ({}, OTHER, dict(sigma_depth=F32(4.0), normal_power_log2=0), dict(sigma_depth=F32(0.5), normal_power_log2=8)):
            want = assert_twin_is_restatement(hc, beauty, spp, rest, **prm)
            assert_twin_is_restatement(hc, ue.wild_rgb(lw * lh), None, rest, **prm)
        if lw * lh > 6:  # (the loose parameters: every class of pixel)
            assert (~want[2] & ~want[3]).any() and want[3].any()
    # sums at the edges of the number formats at both sizes
    lw, lh = 5, 3
    beauty, spp, aov_lo, s_lo = de.extreme_frame(lw, lh)
    aov_hi = ae.synthetic_sums(factor * factor * lw * lh, seed=31)
    got = twin(hc, beauty, spp, aov_lo, s_lo, lw, lh, factor, aov_hi, 5)
    want = ue.upsample(beauty, spp, aov_lo, s_lo, lw, lh, factor, aov_hi, 5)
    assert_same_bits(got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


def test_a_normal_that_opposes_every_tap_takes_the_tent_form(hc):
    lw, lh, factor = 4, 3, 2
    n = factor * factor * lw * lh
    aov_lo, aov_hi = flat_aov(lw * lh), flat_aov(n)
    at = 2 * (factor * lw) + 3
    aov_hi[at] = flat_aov(1, normal=(0, 0, -1))[0]
    want = assert_twin_is_restatement(hc, ramp(lw * lh), 1, (aov_lo, 1, lw, lh, factor, aov_hi, 1))
    assert want[2][at] and want[2].sum() == 1 and not want[3].any()
    # the plain tent filter of the low frame: between the smallest and the largest u of the low pixels, times albedo 1
    lo = ramp(lw * lh)[:, 0] / ONE
    assert lo.min() <= want[0][at, 0] <= lo.max()


def test_a_pixel_no_sample_hit_takes_the_shortcut(hc):
    lw, lh, factor = 4, 3, 3
    n = factor * factor * lw * lh
    aov_lo, aov_hi = flat_aov(lw * lh), flat_aov(n)
    aov_hi[5] = 0
    aov_hi[7] = flat_aov(1, hits=-3)[0]  # (hits <= 0, whatever else the record holds)
    aov_hi[7, ae.EMISSION] = ONE
    want = assert_twin_is_restatement(hc, ramp(lw * lh), 1, (aov_lo, 1, lw, lh, factor, aov_hi, 1))
    assert want[3][5] and want[3][7] and want[3].sum() == 2 and not want[2].any()
    assert (want[0][5] == 0).all() and want[0][7, 0] == 1  # u = 0: what is left is the pixel's own emission


@pytest.mark.parametrize("factor", ue.FACTORS)
def test_a_low_image_of_one_pixel(hc, factor):
    n = factor * factor
    aov_lo, aov_hi = flat_aov(1), flat_aov(n)
    beauty = np.array([[ONE * 4, ONE, ONE // 2]], np.int64)
    want = assert_twin_is_restatement(hc, beauty, 2, (aov_lo, 1, 1, 1, factor, aov_hi, 1))
    assert not want[2].any() and not want[3].any()
    assert_same_bits(want[0], np.tile(np.array([2.0, 0.5, 0.25], F32), (n, 1)))  # one tap and u a power of two: (w * u) / w is u exactly
    for lw, lh in ((1, 4), (5, 1)):
        a_lo, a_hi = flat_aov(lw * lh), flat_aov(n * lw * lh)
        assert_twin_is_restatement(hc, ramp(lw * lh), 1, (a_lo, 1, lw, lh, factor, a_hi, 1))


def test_a_tap_with_the_spatial_weight_zero(hc):
    """factor 3, x = 1: a = 0, fx = 0, and tap j = 2 has k = 1 - 0.5 * 2 = 0: it is visited and adds nothing."""
    x0, fx = ue.position(9, 3)
    assert x0[1] == 0 and fx[1] == 0 and ue.tent(2, fx)[1] == 0 and ue.tent(-1, fx)[1] == F32(0.5)
    assert x0[0] == -1 and fx[0] == F32(4 / 6)
    lw, lh, factor = 3, 3, 3
    aov_lo, aov_hi = flat_aov(9), flat_aov(81)
    beauty = ramp(9)
    want = assert_twin_is_restatement(hc, beauty, 1, (aov_lo, 1, lw, lh, factor, aov_hi, 1))
    # pixel (1, 1) taps low columns -1 .. 2 and rows -1 .. 2; column 2 and row 2 carry k = 0: changing them changes nothing there
    other = beauty.copy()
    other[[2, 5, 6, 7, 8]] += ONE
    moved = twin(hc, other, 1, aov_lo, 1, lw, lh, factor, aov_hi, 1)
    p = 1 * 9 + 1
    assert_same_bits(moved[0][p], want[0][p])
    assert not np.array_equal(ue.bits(moved[0][p + 1]), ue.bits(want[0][p + 1]))


def test_a_depth_gap_drives_the_weight_to_exactly_zero(hc):
    lw, lh, factor = 4, 3, 4
    n = factor * factor * lw * lh
    aov_lo, aov_hi = flat_aov(lw * lh, depth=1.0), flat_aov(n, depth=1.0)
    at = 5 * (factor * lw) + 6
    aov_hi[at] = flat_aov(1, depth=1.5)[0]
    kz = ue.depth_constant(ue.default_params()["sigma_depth"])
    assert de.expnegf(-F32(F32(0.25) * kz)) == 0 and kz == 1024
    want = assert_twin_is_restatement(hc, ramp(lw * lh), 1, (aov_lo, 1, lw, lh, factor, aov_hi, 1))
    assert want[2][at] and want[2].sum() == 1
    # a gap the exponential still resolves stays guided
    aov_hi[at] = flat_aov(1, depth=1.0625)[0]
    want = assert_twin_is_restatement(hc, ramp(lw * lh), 1, (aov_lo, 1, lw, lh, factor, aov_hi, 1))
    assert not want[2].any()


def test_non_finite_radiance_counts_as_zero(hc):
    lw, lh, factor = 4, 3, 2
    n = factor * factor * lw * lh
    rest = (flat_aov(lw * lh), 1, lw, lh, factor, flat_aov(n), 1)
    rgb = (ramp(lw * lh) / ONE).astype(F32)
    bad = rgb.copy()
    bad[1, 0], bad[5, 1], bad[6, 2], bad[7] = np.nan, np.inf, -np.inf, np.nan
    mended = bad.copy()
    mended[~np.isfinite(bad)] = 0
    want = assert_twin_is_restatement(hc, bad, None, rest)
    assert np.isfinite(want[0]).all()
    assert_same_bits(want[0], twin(hc, mended, None, *rest)[0])
    # and a finite frame is the sums' frame: rt_upsample_rgb of the mean == rt_upsample_fixed of the sums
    assert_same_bits(twin(hc, rgb, None, *rest)[0], twin(hc, ramp(lw * lh), 1, *rest)[0])


# ----------------------------------------------------------------------------- the surface
def test_new_entry_points_are_declared_exported_bound_and_built(api):
    header = open(os.path.join(ROOT, "include", "rtcuda_amd.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("rt_upsample_default_params", "rt_upsample_fixed", "rt_upsample_rgb"):
        assert name in api.EXPORTS and re.search(rf"^int {name}\(", header, re.M)
        assert getattr(api.lib(), name).argtypes is not None
        assert re.search(rf"\bT {name}$", syms, re.M)
    assert "typedef struct rt_upsample_params" in header
    all_syms = subprocess.run(["nm", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    kernels = set(re.findall(r" (_Z\d+k_upsampleILi\dELb[01]E\w*)$", all_syms, re.M))
    assert len({re.search(r"ILi(\d)ELb([01])E", k).groups() for k in kernels}) == 6, kernels  # one instance per factor and input kind
    assert ctypes.sizeof(api.RtUpsampleParams) == 12
    assert api.upsample_default_params() == {k: (float(v) if k.startswith("sigma") else v) for k, v in ue.default_params().items()}
    assert callable(api.upsample) and callable(api.upsample_rgb)
    hpp = open(os.path.join(ROOT, "include", "rtcuda", "rtcuda.hpp")).read()
    for text in ("inline void upsample(", "inline void upsample_rgb(", "inline rt_upsample_params upsample_default_params("):
        assert text in hpp


def test_errors_name_the_entry_point_and_write_nothing(api, hc):
    """Every refusal comes before a device is needed: host arrays stand in for the device buffers and stay as they were."""
    L = api.lib()
    s, rgb, lo, hi = np.full(3, 7, np.int64), np.full(3, 7, np.float32), np.full(11, 7, np.int64), np.full(44, 7, np.int64)
    out, fixed = np.full(12, 7, np.float32), np.full(12, 7, np.int64)
    good = dict(sigma_depth=0.5, normal_power_log2=1, flags=0)
    P = lambda a: a.ctypes.data  # noqa: E731

    def call(kind, a="low", ns=1, l=P(lo), nl=1, w=1, h=1, f=2, g=P(hi), nh=1, o=P(out), x=P(fixed), **over):
        p = api.RtUpsampleParams(**dict(good, **over))
        if kind == "fixed":
            rc = L.rt_upsample_fixed(P(s) if a == "low" else a, ns, l, nl, w, h, f, g, nh, ctypes.byref(p), o, x, None)
        else:
            rc = L.rt_upsample_rgb(P(rgb) if a == "low" else a, l, nl, w, h, f, g, nh, ctypes.byref(p), o, x, None)
        return rc, L.rt_last_error().decode()

    nan = float("nan")
    for kind, low_name in (("fixed", "d_sum_lo"), ("rgb", "d_rgb_lo")):
        cases = [(dict(a=None), "null " + low_name), (dict(l=None), "null d_aov_lo"), (dict(g=None), "null d_aov_hi"),
                 (dict(o=None, x=None), "null d_rgb_out and null d_out_fixed"), (dict(f=1), "factor must be 2, 3 or 4"),
                 (dict(f=5), "factor must be 2, 3 or 4"), (dict(w=0), "low_width and low_height must be at least 1"),
                 (dict(h=-1), "low_width and low_height must be at least 1"), (dict(w=1 << 19, h=1 << 9, f=2), "more than 715827882 pixels"),
                 (dict(w=1 << 30, h=1 << 30, f=4), "more than 715827882 pixels"), (dict(nl=0), "aov_samples_hi must be at least 1"),
                 (dict(nh=-1), "aov_samples_hi must be at least 1"), (dict(flags=4), "flags must be 0"),
                 (dict(normal_power_log2=-1), "normal_power_log2 must be 0 .. 8"), (dict(normal_power_log2=9), "normal_power_log2 must be 0 .. 8"),
                 (dict(sigma_depth=nan), "sigma_depth must be finite and positive"), (dict(sigma_depth=0.0), "sigma_depth must be finite and positive"),
                 (dict(sigma_depth=float("inf")), "sigma_depth must be finite and positive"), (dict(sigma_depth=1e-30), "sigma_depth gives a depth constant"),
                 (dict(sigma_depth=1e30), "sigma_depth gives a depth constant"), (dict(w=1, h=44739242, f=4), "needs more than 16777215 workgroups")]
        if kind == "fixed":
            cases.append((dict(ns=0), "num_samples, aov_samples_lo and aov_samples_hi must be at least 1"))
        for over, text in cases:
            rc, msg = call(kind, **over)
            assert rc != 0 and msg.startswith(f"rt_upsample_{kind}: ") and text in msg, (kind, over, msg)
    for a in (s, rgb, lo, hi, out, fixed):
        assert (a == 7).all()
    assert L.rt_upsample_default_params(None) != 0 and L.rt_last_error().decode() == "rt_upsample_default_params: null out"
    beauty, spp, aov_lo, s_lo, aov_hi, s_hi = ue.synthetic_pair(3, 2, 2)
    for kw in (dict(sigma_depth=nan), dict(sigma_depth=-1.0), dict(sigma_depth=1e-30), dict(normal_power_log2=9), dict(normal_power_log2=-1)):
        assert twin(hc, beauty, spp, aov_lo, s_lo, 3, 2, 2, aov_hi, s_hi, expect_rc=1, **kw) is None
    assert twin(hc, beauty, spp, aov_lo, s_lo, 3, 2, 2, aov_hi, s_hi, expect_rc=1, want=()) is None
    assert twin(hc, beauty, 0, aov_lo, s_lo, 3, 2, 2, aov_hi, s_hi, expect_rc=1) is None


def test_cpp_wrappers_link_and_throw_the_library_message():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "upsamplecheck"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "upsample_api_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(l.split("=", 1) for l in out.stdout.splitlines())
    dp = ue.default_params()
    assert lines["defaults"] == "%g %d" % (float(dp["sigma_depth"]), dp["normal_power_log2"])
    assert lines["null_aov_hi"] == "upsample: rt_upsample_fixed: null d_aov_hi"
    assert lines["no_output"] == "upsample: rt_upsample_fixed: null d_rgb_out and null d_out_fixed"
    assert lines["factor"] == "upsample: rt_upsample_fixed: factor must be 2, 3 or 4"
    assert lines["sigma"] == "upsample: rt_upsample_fixed: sigma_depth must be finite and positive"
    assert lines["samples"] == "upsample: rt_upsample_fixed: num_samples, aov_samples_lo and aov_samples_hi must be at least 1"
    assert lines["rgb_null"] == "upsample_rgb: rt_upsample_rgb: null d_rgb_lo"
    assert lines["outputs_untouched"].startswith("1 ")


def test_wrapper_rejects_bad_arguments_before_reaching_the_library(api):
    torch = pytest.importorskip("torch")

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    def gpu(x):
        return x.as_subclass(OnGpu)

    b, lo, hi = gpu(torch.zeros(2, 3, dtype=torch.int64)), gpu(torch.zeros(2, 11, dtype=torch.int64)), gpu(torch.zeros(8, 11, dtype=torch.int64))
    c = gpu(torch.zeros(2, 3))
    f, g = api.upsample, api.upsample_rgb
    cases = [("upsample: beauty_lo must be a torch tensor on a GPU", lambda: f(torch.zeros(2, 3, dtype=torch.int64), 1, lo, 1, 2, 1, 2, hi, 1)),
             (r"upsample: aov_hi must be a contiguous \(18, 11\) torch.int64", lambda: f(b, 1, lo, 1, 2, 1, 3, hi, 1)),
             ("upsample: factor must be 2, 3 or 4", lambda: f(b, 1, lo, 1, 2, 1, 5, hi, 1)),
             ("upsample: spp must be a positive int", lambda: f(b, 0, lo, 1, 2, 1, 2, hi, 1)),
             (r"upsample: normal_power_log2 must be an int in 0 \.\. 8", lambda: f(b, 1, lo, 1, 2, 1, 2, hi, 1, normal_power_log2=9)),
             ("upsample: sigma_depth must be a finite positive number", lambda: f(b, 1, lo, 1, 2, 1, 2, hi, 1, sigma_depth=0.0)),
             ("upsample: at least one of the two outputs", lambda: f(b, 1, lo, 1, 2, 1, 2, hi, 1, rgb=False, fixed=False)),
             (r"upsample_rgb: rgb_lo must be a contiguous \(2, 3\) torch.float32", lambda: g(b, lo, 1, 2, 1, 2, hi, 1)),
             ("upsample_rgb: rgb_lo must be a torch tensor on a GPU", lambda: g(torch.zeros(2, 3), lo, 1, 2, 1, 2, hi, 1)),
             ("upsample_rgb: aov_spp_lo must be a positive int", lambda: g(c, lo, 0, 2, 1, 2, hi, 1))]
    for pattern, call in cases:
        with pytest.raises(api.RtError, match=pattern):
            call()
