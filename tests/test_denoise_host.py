"""CPU tests of the denoiser (rt_denoise_fixed / rt_denoise_default_params / rt_denoise_scratch_bytes): rt_expnegf and the CPU twin
(hc_denoise of librt_hostcheck.so: a serial loop over rtcuda_amd/csrc/rt_denoise.h, the kernels' arithmetic) are held to the numpy
restatement of the header's text (tests/denoise_expected.py) bit for bit, the twin is shown to denoise and to leave a frame without
noise alone, and the entry points are declared / exported / bound / refuse bad arguments.  Everything that runs a kernel is in
tests/test_gpu_denoise.py."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, default_camera, oracle_scene
import aov_expected as ae
import denoise_expected as de

NEW = ("rt_denoise_scratch_bytes", "rt_denoise_default_params", "rt_denoise_fixed")
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
    L.hc_denoise.argtypes = [vp, ci, vp, ci, ci, ci, ci, cf, cf, ci, vp]
    L.hc_expnegf.argtypes = [vp, vp, ci]
    L.hc_expnegf.restype = None
    return L


def twin(hc, frame, w, h, passes=None, sigma_color=None, sigma_depth=None, normal_power_log2=None, expect_rc=0):
    dp = de.default_params()
    beauty, spp, aov, aov_spp = frame
    beauty, aov = np.ascontiguousarray(beauty, np.int64), np.ascontiguousarray(aov, np.int64)
    assert beauty.shape == (w * h, 3) and aov.shape == (w * h, ae.CHANNELS)
    out = np.full((w * h, 3), -7, np.float32)
    rc = hc.hc_denoise(beauty.ctypes.data, spp, aov.ctypes.data, aov_spp, w, h,
                       dp["passes"] if passes is None else passes, dp["sigma_color"] if sigma_color is None else sigma_color,
                       dp["sigma_depth"] if sigma_depth is None else sigma_depth,
                       dp["normal_power_log2"] if normal_power_log2 is None else normal_power_log2, out.ctypes.data)
    assert rc == expect_rc
    return out


def assert_same_bits(got, want):
    g, w = de.bits(got), de.bits(want)
    assert g.shape == w.shape
    bad = np.flatnonzero((g != w).reshape(-1))
    assert bad.size == 0, (bad.size, bad[:5], np.asarray(got).reshape(-1)[bad[:5]], np.asarray(want).reshape(-1)[bad[:5]])


# ----------------------------------------------------------------------------- rt_expnegf
def _exp_inputs():
    x = np.linspace(-87.0, 0.0, 100001).astype(np.float32)
    edge = np.array([-87.0, np.nextafter(F32(-87), F32(0)), np.nextafter(F32(-87), F32(-100)), 0.0, -0.0, -1e-30, -88.0, -1e30,
                     -np.inf, np.nan], np.float32)
    return np.concatenate([x, edge])


def test_expnegf_numpy_and_twin_agree_bit_for_bit(hc):
    x = _exp_inputs()
    y = np.full_like(x, 7)
    hc.hc_expnegf(x.ctypes.data, y.ctypes.data, x.size)
    assert_same_bits(y, de.expnegf(x))
    e = de.expnegf(np.array([0.0, -0.0, -87.0, -88.0, -np.inf, np.nan], np.float32))
    assert de.bits(e).tolist() == [0x3F800000, 0x3F800000, 0, 0, 0, 0]
    assert de.expnegf(np.nextafter(F32(-87), F32(0))) > 0


def test_expnegf_is_within_two_ulp_of_exp():
    x = _exp_inputs()
    x = x[x > -87.0]
    got = de.expnegf(x)
    want = np.exp(x.astype(np.float64))
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want) / ulp
    print("largest error of rt_expnegf over the range, in ulp:", float(err.max()))
    assert err.max() <= 2.0
    assert np.all(got >= np.finfo(np.float32).tiny)  # (normal numbers down to the cut-off: the last product is exact)


# ----------------------------------------------------------------------------- the twin against the restatement
SIZES = ((1, 1), (3, 2), (5, 5), (33, 17))


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kind", ["synthetic", "extreme"])
def test_twin_equals_the_restatement_on_synthetic_and_extreme_sums(hc, kind, w, h):
    frame = de.synthetic_frame(w, h) if kind == "synthetic" else de.extreme_frame(w, h)
    for passes in (0, 1, 5, 8):  # (stride 128 exceeds every one of these images)
        for npow in (0, 8):
            want = de.denoise(*frame, w, h, passes, F32(0.7), F32(0.3), npow)
            assert np.isfinite(want).all()  # (the clamp of w_n: no NaN, whose bits would be the processor's)
            assert_same_bits(twin(hc, frame, w, h, passes, 0.7, 0.3, npow), want)
    assert_same_bits(twin(hc, frame, w, h), de.denoise(*frame, w, h))


def test_twin_equals_the_restatement_on_a_real_frame(hc, oracle):
    w, h, spp = de.REAL_FRAME
    osc = oracle_scene(oracle, "full_bsdf", True)
    frame = de.real_frame(oracle, osc, default_camera(oracle, w / h), w, h, spp)
    assert int(frame[0].sum()) > 0 and ae.frame_census(frame[2], spp)[0] > w * h // 2
    assert_same_bits(twin(hc, frame, w, h), de.denoise(*frame, w, h))
    assert_same_bits(twin(hc, frame, w, h, 5, 1.0, 0.125, 5), de.denoise(*frame, w, h, 5, F32(1.0), F32(0.125), 5))


def test_twin_equals_the_restatement_where_tap_weights_are_denormal(hc):
    (frame, prm), (w, h) = de.denormal_case(), (9, 7)
    # the claim of the case: a direct neighbour's weight is a denormal that is not zero
    u, z, n, _, _ = de.prepare(*frame)
    kc, kz = de.pass_constants(prm["passes"], prm["sigma_color"], prm["sigma_depth"])
    du = (u[1] - u[0]).astype(F32)
    xc = F32(F32(F32(F32(du[0] * du[0]) + F32(du[1] * du[1])) + F32(du[2] * du[2])) * kc[0])
    wt = F32(F32(F32(0.25) * F32(0.375)) * de.expnegf(F32(-xc)))
    assert 0 < wt < np.finfo(np.float32).tiny, (xc, wt)
    want = de.denoise(*frame, w, h, **prm)
    assert_same_bits(twin(hc, frame, w, h, **prm), want)


# ----------------------------------------------------------------------------- what the filter does
def test_defaults_are_the_sweeps_and_the_librarys(api):
    q = json.load(open(os.path.join(ROOT, "profiles", "denoise_quality.json")))
    dp = de.default_params()
    assert {k: float(v) for k, v in dp.items()} == {k: float(v) for k, v in q["defaults"].items()}
    assert api.denoise_default_params() == {k: (int(v) if k in ("passes", "normal_power_log2") else float(v)) for k, v in dp.items()}
    assert q["frames"] == [[64, 48, 4], [64, 48, 16], [192, 144, 4], [192, 144, 16]] and q["reference_spp"] == de.REFERENCE_SPP
    best = q["table"][0]
    assert all(0 < r < 1 for r in q["default_rms_ratios"][:2]) and q["default_score"] <= best["score"] * 1.01


@pytest.mark.parametrize("spp", [4, 16])
def test_it_denoises(hc, oracle, spp):
    """RMS error of the twin's output against the oracle's 1024-spp frame, below that of the undenoised frame (all linear
    means).  The ratios are recorded in profiles/denoise_quality.json; here only the strict inequality."""
    w, h = 64, 48
    osc = oracle_scene(oracle, "full_bsdf", True)
    cam = default_camera(oracle, w / h)
    frame = de.real_frame(oracle, osc, cam, w, h, spp)
    ref = de.reference_mean(oracle, osc, cam, w, h)
    noisy = de.rms(de.noisy_mean(frame[0], spp), ref)
    clean = de.rms(twin(hc, frame, w, h), ref)
    print(f"{w}x{h}x{spp}: rms noisy {noisy:.6f} denoised {clean:.6f} ratio {clean / noisy:.4f}")
    assert clean < noisy


def test_a_frame_without_noise_comes_back_unchanged(hc, oracle):
    """beauty = 2 * albedo on the features of a real frame (emission zeroed).  The derivation of the bound: c = 2 * a exactly
    (a power of two commutes with the rounding of float(sum * 2^-30) * inv), so u = c / d = 2 exactly in every channel of every
    pixel (d = a, or both are the floor's).  In a pass every product w * u_q = 2 * w is exact, so after every tap su = 2 * sw
    exactly -- doubling commutes with each rounded addition, denormal weights included -- and su / sw = 2 exactly: the weights
    normalise without a rounding error.  Remodulation is u * d + 0 = 2 * d = c, exact again.  The bound is therefore 0 ulp, on
    every pixel and a fortiori on those with full coverage."""
    w, h, spp = de.REAL_FRAME
    osc = oracle_scene(oracle, "full_bsdf", True)
    real = de.real_frame(oracle, osc, default_camera(oracle, w / h), w, h, spp)
    frame = de.noise_free_frame(real[2], spp)
    u = de.prepare(*frame)[0]
    assert (u == 2).all()
    full = frame[2][:, ae.HITS] == spp
    assert full.sum() > w * h // 2
    for prm in ({}, dict(passes=5, sigma_color=1.0, sigma_depth=0.125, normal_power_log2=5)):
        out = twin(hc, frame, w, h, **prm)
        assert_same_bits(out[full], de.noisy_mean(frame[0], spp)[full])
        assert_same_bits(out, de.noisy_mean(frame[0], spp))


def test_the_form_table_is_the_measured_one(api):
    """dn_lds_wins (rt_host_denoise.inc) must say what tools/denoise_time.py measured: the `kept` form per stride of
    profiles/denoise_time.json, read back here from the source."""
    t = json.load(open(os.path.join(ROOT, "profiles", "denoise_time.json")))
    src = open(os.path.join(ROOT, "rtcuda_amd", "csrc", "rt_host_denoise.inc")).read()
    body = re.search(r"bool dn_lds_wins\(int stride\) \{ return (.*?); \}", src).group(1)
    for i, kept in enumerate(t["kept"]):
        assert eval(body.replace("||", " or ").replace("&&", " and "), {"stride": 1 << i, "false": False, "true": True}) == (kept == "lds"), (1 << i, kept, body)


# ----------------------------------------------------------------------------- the surface
def test_new_entry_points_are_declared_exported_and_bound(api):
    header = open(os.path.join(ROOT, "include", "rtcuda_amd.h")).read()
    for name in NEW:
        assert name in api.EXPORTS
        assert re.search(rf"^int(64_t)? {name}\(", header, re.M), name
        assert getattr(api.lib(), name).argtypes is not None
    assert "typedef struct rt_denoise_params {" in header
    assert ctypes.sizeof(api.RtDenoiseParams) == 20
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bT {name}$", syms, re.M), name
    for name in ("denoise", "denoise_default_params", "denoise_scratch_bytes"):
        assert callable(getattr(api, name))
    all_syms = subprocess.run(["nm", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for kernel in ("k_dn_prepare", "k_atrous", "k_dn_finish"):
        assert re.search(rf" _Z\d+{kernel}", all_syms), kernel
    assert api.denoise_scratch_bytes(33, 17) == 48 * 33 * 17
    assert api.lib().rt_denoise_scratch_bytes(0, 1) < 0 and api.lib().rt_denoise_scratch_bytes(1 << 20, 1 << 10) < 0
    assert api.lib().rt_denoise_scratch_bytes(715827882, 1) == 48 * 715827882


def test_host_side_errors_name_the_entry_point_and_write_nothing(api):
    """Every refusal comes before a device is needed: host arrays stand in for the device buffers and stay as they were."""
    L = api.lib()
    sums = np.full(3, 7, np.int64)
    aov = np.full(ae.CHANNELS, 7, np.int64)
    scratch = np.full(16, 7, np.int64)  # (8-byte items, 16 of them: holds an aligned 48 bytes wherever it starts)
    sp = (scratch.ctypes.data + 15) // 16 * 16
    out = np.full(3, 7, np.float32)
    good = dict(passes=1, sigma_color=1.0, sigma_depth=1.0, normal_power_log2=1, flags=0)

    def call(s=sums.ctypes.data, spp=1, a=aov.ctypes.data, aspp=1, w=1, h=1, scr=sp, o=out.ctypes.data, **over):
        prm = api.RtDenoiseParams(**dict(good, **over))
        rc = L.rt_denoise_fixed(s, spp, a, aspp, w, h, ctypes.byref(prm), scr, o, None)
        return rc, L.rt_last_error().decode()

    inf, nan = float("inf"), float("nan")
    cases = [
        (dict(s=None), "null d_sum_fixed"), (dict(a=None), "null d_aov_fixed"), (dict(scr=None), "null d_scratch"),
        (dict(o=None), "null d_rgb_out"), (dict(w=0), "width and height"), (dict(h=-3), "width and height"),
        (dict(w=1 << 20, h=1 << 10), "more than 715827882 pixels"), (dict(spp=0), "num_samples and aov_samples"),
        (dict(aspp=0), "num_samples and aov_samples"), (dict(scr=sp + 8), "16-byte aligned"),
        (dict(passes=-1), "passes must be 0 .. 8"), (dict(passes=9), "passes must be 0 .. 8"),
        (dict(normal_power_log2=-1), "normal_power_log2 must be 0 .. 8"), (dict(normal_power_log2=9), "normal_power_log2 must be 0 .. 8"),
        (dict(sigma_color=0.0), "sigma_color must be finite and positive"), (dict(sigma_color=-1.0), "sigma_color must be finite"),
        (dict(sigma_color=inf), "sigma_color must be finite"), (dict(sigma_color=nan), "sigma_color must be finite"),
        (dict(sigma_depth=0.0), "sigma_depth must be finite and positive"), (dict(sigma_depth=nan), "sigma_depth must be finite"),
        (dict(sigma_color=1e-30), "colour constant that is not finite"),  # (sigma^2 underflows to 0: kc = inf)
        (dict(sigma_color=1e30), "colour constant that is not finite"),   # (sigma^2 overflows: kc = 0)
        (dict(sigma_depth=1e-30), "depth constant that is not finite"), (dict(sigma_depth=1e30), "depth constant"),
        (dict(flags=1), "flags must be 0"),
        (dict(w=1, h=715827882), "needs more than 16777215 workgroups in the pass of stride 1"),  # (2^32 threads a launch)
        (dict(w=715827882, h=1, passes=8), "needs more than 16777215 workgroups"),
    ]
    for over, text in cases:
        rc, msg = call(**over)
        assert rc != 0 and msg.startswith("rt_denoise_fixed: ") and text in msg, (over, msg)
    assert L.rt_denoise_default_params(None) != 0
    assert L.rt_last_error().decode() == "rt_denoise_default_params: null out"
    assert (sums == 7).all() and (aov == 7).all() and (scratch == 7).all() and (out == 7).all()
    # the twin refuses the same parameters
    frame = de.synthetic_frame(3, 2)
    hcl = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    hcl.hc_denoise.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_int] * 3 + [ctypes.c_float] * 2 + [ctypes.c_int, ctypes.c_void_p]
    for kw in (dict(passes=9), dict(normal_power_log2=9), dict(sigma_color=0.0), dict(sigma_depth=float("nan")), dict(sigma_color=1e-30)):
        assert (twin(hcl, frame, 3, 2, expect_rc=1, **kw) == -7).all()


def test_wrapper_rejects_bad_tensors_before_reaching_the_library(api):
    torch = pytest.importorskip("torch")

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    def gpu(x):
        return x.as_subclass(OnGpu)

    b, a = gpu(torch.zeros(8, 3, dtype=torch.int64)), gpu(torch.zeros(8, 11, dtype=torch.int64))
    cases = [
        ("denoise: beauty_sums must be a torch tensor on a GPU", lambda: api.denoise(torch.zeros(8, 3, dtype=torch.int64), 1, a, 1, 4, 2)),
        ("denoise: aov_sums must be a torch tensor on a GPU", lambda: api.denoise(b, 1, np.zeros((8, 11), np.int64), 1, 4, 2)),
        (r"beauty_sums must be a contiguous \(8, 3\) torch.int64", lambda: api.denoise(gpu(torch.zeros(8, 3)), 1, a, 1, 4, 2)),
        (r"beauty_sums must be a contiguous \(6, 3\) torch.int64", lambda: api.denoise(b, 1, a, 1, 3, 2)),
        (r"aov_sums must be a contiguous \(8, 11\) torch.int64", lambda: api.denoise(b, 1, gpu(torch.zeros(8, 10, dtype=torch.int64)), 1, 4, 2)),
        (r"aov_sums must be a contiguous \(8, 11\)", lambda: api.denoise(b, 1, gpu(torch.zeros(11, 8, dtype=torch.int64).t()), 1, 4, 2)),
        ("denoise: spp must be a positive int", lambda: api.denoise(b, 0, a, 1, 4, 2)),
        ("denoise: aov_spp must be a positive int", lambda: api.denoise(b, 1, a, 1.0, 4, 2)),
        ("denoise: width must be a positive int", lambda: api.denoise(b, 1, a, 1, 0, 2)),
        ("denoise: passes must be an int in 0 .. 8", lambda: api.denoise(b, 1, a, 1, 4, 2, passes=9)),
        ("denoise: normal_power_log2 must be an int in 0 .. 8", lambda: api.denoise(b, 1, a, 1, 4, 2, normal_power_log2=-1)),
        ("denoise: sigma_color must be a finite positive number", lambda: api.denoise(b, 1, a, 1, 4, 2, sigma_color=0)),
        ("denoise: sigma_depth must be a finite positive number", lambda: api.denoise(b, 1, a, 1, 4, 2, sigma_depth=float("nan"))),
        ("denoise_scratch_bytes: bad frame size", lambda: api.denoise_scratch_bytes(0, 5)),
        ("denoise_scratch_bytes: width and height must be ints", lambda: api.denoise_scratch_bytes(4.0, 5)),
    ]
    for pattern, call in cases:
        with pytest.raises(api.RtError, match=pattern):
            call()


def test_cpp_wrappers_link_and_throw_the_library_message():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "denoisecheck"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "denoise_api_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(l.split("=", 1) for l in out.stdout.splitlines())
    dp = de.default_params()
    assert lines["scratch"] == str(48 * 33 * 17)
    assert lines["defaults"] == f"{dp['passes']} {dp['normal_power_log2']}"
    assert lines["null_out"] == "denoise: rt_denoise_fixed: null d_rgb_out"
    assert lines["passes"] == "denoise: rt_denoise_fixed: passes must be 0 .. 8, it is 9"
    assert lines["sigma"] == "denoise: rt_denoise_fixed: sigma_depth must be finite and positive"
    assert lines["size"] == "denoise_scratch_bytes: bad frame size 0 x 4"
    assert lines["out"] == "7 7 7"
