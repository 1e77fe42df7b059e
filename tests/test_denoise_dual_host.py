"""CPU tests of the dual-buffer denoiser (rt_denoise_dual_fixed / rt_denoise_dual_default_params / rt_denoise_dual_scratch_bytes):
the CPU twin (hc_denoise_dual of librt_hostcheck.so: a serial loop over rtcuda_amd/csrc/rt_denoise.h, the kernels' arithmetic) is
held to the numpy restatement of the header's text (tests/denoise_dual_expected.py) bit for bit; it is shown to absorb a firefly
that rt_denoise_fixed protects, to leave a frame without noise alone and to denoise; the entry points are declared / exported /
bound / refuse bad arguments.  Everything that runs a kernel is in tests/test_gpu_denoise_dual.py."""
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
import denoise_dual_expected as dd

NEW = ("rt_denoise_dual_scratch_bytes", "rt_denoise_dual_default_params", "rt_denoise_dual_fixed")
F32 = np.float32
OTHER = dict(sigma_variance=F32(1.5), sigma_depth=F32(0.3))


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


@pytest.fixture(scope="module")
def hc(api):
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.hc_denoise_dual.argtypes = [vp, ci, vp, ci, vp, ci, ci, ci, ci, cf, cf, ci, vp, vp]
    L.hc_denoise.argtypes = [vp, ci, vp, ci, ci, ci, ci, cf, cf, ci, vp]
    return L


def twin(hc, halves, w, h, passes=None, sigma_variance=None, sigma_depth=None, normal_power_log2=None, expect_rc=0, variance=False):
    dp = dd.default_params()
    a, spp_a, b, spp_b, aov, aov_spp = halves
    a, b, aov = np.ascontiguousarray(a, np.int64), np.ascontiguousarray(b, np.int64), np.ascontiguousarray(aov, np.int64)
    assert a.shape == (w * h, 3) and b.shape == (w * h, 3) and aov.shape == (w * h, ae.CHANNELS)
    out = np.full((w * h, 3), -7, np.float32)
    var = np.full(w * h, -7, np.float32)
    rc = hc.hc_denoise_dual(a.ctypes.data, spp_a, b.ctypes.data, spp_b, aov.ctypes.data, aov_spp, w, h,
                            dp["passes"] if passes is None else passes,
                            dp["sigma_variance"] if sigma_variance is None else sigma_variance,
                            dp["sigma_depth"] if sigma_depth is None else sigma_depth,
                            dp["normal_power_log2"] if normal_power_log2 is None else normal_power_log2, out.ctypes.data, var.ctypes.data)
    assert rc == expect_rc
    return (out, var) if variance else out


def single(hc, beauty, spp, aov, aov_spp, w, h, **prm):
    """hc_denoise, the twin of rt_denoise_fixed, parameters left out being its defaults."""
    p = dict(de.default_params(), **prm)
    beauty, aov = np.ascontiguousarray(beauty, np.int64), np.ascontiguousarray(aov, np.int64)
    out = np.full((w * h, 3), -7, np.float32)
    assert hc.hc_denoise(beauty.ctypes.data, spp, aov.ctypes.data, aov_spp, w, h, p["passes"], p["sigma_color"], p["sigma_depth"],
                         p["normal_power_log2"], out.ctypes.data) == 0
    return out


def assert_same_bits(got, want):
    g, w = dd.bits(got), dd.bits(want)
    assert g.shape == w.shape
    bad = np.flatnonzero((g != w).reshape(-1))
    assert bad.size == 0, (bad.size, bad[:5], np.asarray(got).reshape(-1)[bad[:5]], np.asarray(want).reshape(-1)[bad[:5]])


# ----------------------------------------------------------------------------- the twin against the restatement
SIZES = ((1, 1), (2, 3), (5, 5), (33, 17), (97, 19))


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kind", ["equal-halves", "unequal-halves", "extreme"])
def test_twin_equals_the_restatement(hc, kind, w, h):
    if kind == "extreme":
        halves = dd.extreme_halves(w, h)
        assert (np.abs(halves[0]) > 1 << 62).any() and (np.abs(halves[2]) > 1 << 62).any()
        s = halves[0].astype(object) + halves[2].astype(object)
        assert any(not -(1 << 63) <= int(v) < 1 << 63 for v in s.reshape(-1))  # (some sum wraps)
    else:
        halves = dd.split_frame(de.synthetic_frame(w, h), *((2, 2) if kind == "equal-halves" else (3, 1)))
    for passes in (0, 1, 2, 5, 8):  # (stride 128 exceeds every one of these images)
        for npow in (0, 8):
            want, want_v = dd.denoise_dual(*halves, w, h, passes, normal_power_log2=npow, with_variance=True, **OTHER)
            assert np.isfinite(want).all() and np.isfinite(want_v).all() and (want_v >= 0).all()
            got, got_v = twin(hc, halves, w, h, passes, normal_power_log2=npow, variance=True, **OTHER)
            assert_same_bits(got, want)
            assert_same_bits(got_v, want_v)
    assert_same_bits(twin(hc, halves, w, h), dd.denoise_dual(*halves, w, h))


def test_twin_equals_the_restatement_where_w_squared_and_v_are_denormal(hc):
    (halves, prm), (w, h) = dd.denormal_case(), (9, 7)
    tiny = np.finfo(np.float32).tiny
    ks, kz, kv = dd.pass_constants(prm["sigma_variance"], prm["sigma_depth"], 1, 1)
    u, v, z, n, _, _ = dd.prepare_dual(*halves, kv)
    # the claims of the case: a direct neighbour's w * w is a denormal that is not zero, and so is v after a pass
    g = dd.variance_blur(v, w, h)
    r = F32(F32(1) / F32(F32(ks * g[0, 0]) + dd.VAR_EPS))
    du = (u[1] - u[0]).astype(F32)
    xv = F32(F32(F32(F32(du[0] * du[0]) + F32(du[1] * du[1])) + F32(du[2] * du[2])) * r)
    wt = F32(F32(F32(0.25) * F32(0.375)) * de.expnegf(F32(-xv)))
    assert 0 < F32(wt * wt) < tiny, (xv, wt)
    assert (v[v > 0] >= tiny).all() and (v > 0).any()
    v1 = dd.atrous_var_pass(u, v, z, n, w, h, 1, ks, kz, 1)[1]
    assert ((v1 > 0) & (v1 < tiny)).any(), v1
    want, want_v = dd.denoise_dual(*halves, w, h, with_variance=True, **prm)
    got, got_v = twin(hc, halves, w, h, variance=True, **prm)
    assert_same_bits(got, want)
    assert_same_bits(got_v, want_v)
    assert ((want_v > 0) & (want_v < tiny)).any()


def test_no_passes_is_rt_denoise_fixed_on_the_sum(hc):
    for w, h, halves in ((33, 17, dd.split_frame(de.synthetic_frame(33, 17), 3, 1)), (5, 5, dd.extreme_halves(5, 5))):
        a, spp_a, b, spp_b, aov, aov_spp = halves
        assert_same_bits(twin(hc, halves, w, h, passes=0), single(hc, dd.wrapped_sum(a, b), spp_a + spp_b, aov, aov_spp, w, h, passes=0))


def test_swapping_equal_halves_changes_nothing(hc):
    w, h = 33, 17
    a, spp_a, b, spp_b, aov, aov_spp = dd.split_frame(de.synthetic_frame(w, h), 2, 2)
    for prm in ({}, dict(OTHER, passes=5, normal_power_log2=2)):
        assert_same_bits(twin(hc, (a, 2, b, 2, aov, aov_spp), w, h, **prm), twin(hc, (b, 2, a, 2, aov, aov_spp), w, h, **prm))


# ----------------------------------------------------------------------------- what the filter does
def test_a_firefly_is_absorbed_where_the_fixed_colour_stop_protects_it(hc):
    """A flat frame at radiance 2, one pixel of half A at 128: the whole frame has 65 there, 63 above its surroundings.  With
    passes 3, sigma_variance 4, sigma_depth 0.5, normal_power_log2 1 the dual filter must leave less than a tenth of that
    deviation (a float64 prototype of the arithmetic left 0.30); rt_denoise_fixed at its defaults leaves 65 exactly, every other
    tap's colour weight being exp(-3 * 63^2 * 64) = 0."""
    (halves, prm, p), (w, h) = dd.firefly_case(), (33, 17)
    a, _, b, _, aov, _ = halves
    assert (de.noisy_mean(dd.wrapped_sum(a, b), 2)[p] == 65).all()
    out = twin(hc, halves, w, h, **prm)
    dev = np.abs(out[p].astype(np.float64) - 2).max()
    print("deviation from 2 at the firefly after the dual filter:", dev, "largest anywhere:", np.abs(out.astype(np.float64) - 2).max())
    assert dev < 6.3
    assert_same_bits(out, dd.denoise_dual(*halves, w, h, **prm))
    fixed = single(hc, dd.wrapped_sum(a, b), 2, aov, 1, w, h)
    assert (fixed[p] == 65.0).all()


def test_equal_halves_of_a_frame_without_noise_come_back_unchanged(hc, oracle):
    """A == B and u = 2 in every channel of every pixel (denoise_expected.noise_free_frame on the features of a real frame, as
    each half at the frame's sample count): v = 0 exactly, and tests/test_denoise_host.py's argument holds tap for tap -- every
    w * u_q = 2 * w is exact, so su = 2 * sw after every tap and su / sw = 2; sv stays 0.  The bound is 0 ulp."""
    w, h, spp = de.REAL_FRAME
    osc = oracle_scene(oracle, "full_bsdf", True)
    real = de.real_frame(oracle, osc, default_camera(oracle, w / h), w, h, spp)
    beauty, _, aov, _ = de.noise_free_frame(real[2], spp)
    halves = (beauty, spp, beauty, spp, aov, spp)
    for prm in ({}, dict(passes=5, sigma_variance=0.5, sigma_depth=0.5, normal_power_log2=1)):
        out, var = twin(hc, halves, w, h, variance=True, **prm)
        assert_same_bits(out, de.noisy_mean(beauty, spp))
        assert (var == 0).all()


def _oracle_halves(oracle, osc, cam, w, h, spp):
    from oracle.oracle import usable_cpus
    halves = []
    for r in (0, 1):
        fixed = np.zeros((h, w, 3), np.int64)
        osc.render(cam, w, h, spp, threads=usable_cpus(), fixed_out=fixed, rng_mode="per_sample", shard=(r, 2))
        halves.append(fixed.reshape(-1, 3))
    return halves


@pytest.mark.parametrize("spp", [4, 16])
def test_it_denoises(hc, oracle, spp):
    """RMS and relMSE of the twin's output at the defaults against the oracle's 1024-spp frame, strictly below the noisy
    frame's.  The halves are the oracle's shards (0, 2) and (1, 2) of the per-sample frame; their sum is that frame."""
    w, h = 64, 48
    osc = oracle_scene(oracle, "full_bsdf", True)
    cam = default_camera(oracle, w / h)
    whole = de.real_frame(oracle, osc, cam, w, h, spp)
    a, b = _oracle_halves(oracle, osc, cam, w, h, spp)
    assert np.array_equal(a + b, whole[0])
    ref = de.reference_mean(oracle, osc, cam, w, h)
    noisy = de.noisy_mean(whole[0], spp)
    out = twin(hc, (a, spp // 2, b, spp // 2, whole[2], spp), w, h)

    def relmse(x):
        return float(np.mean((x.astype(np.float64) - ref) ** 2 / (ref ** 2 + 0.01)))

    print(f"{w}x{h}x{spp}: rms noisy {de.rms(noisy, ref):.6f} denoised {de.rms(out, ref):.6f}; relmse noisy {relmse(noisy):.6f} denoised {relmse(out):.6f}")
    assert de.rms(out, ref) < de.rms(noisy, ref)
    assert relmse(out) < relmse(noisy)


def test_defaults_are_the_sweeps_and_the_librarys(api):
    q = json.load(open(os.path.join(ROOT, "profiles", "denoise_dual_quality.json")))
    dp = dd.default_params()
    assert {k: float(v) for k, v in dp.items()} == {k: float(v) for k, v in q["defaults"].items()}
    assert api.denoise_dual_default_params() == {k: (int(v) if k in ("passes", "normal_power_log2") else float(v)) for k, v in q["defaults"].items()}
    assert q["frames"] == [[64, 48, 4], [64, 48, 16], [192, 144, 4], [192, 144, 16]] and q["reference_spp"] == de.REFERENCE_SPP
    assert all(0 < r < 1 for r in q["default_rms_ratios"][:2]) and q["default_score"] <= q["table"][0]["score"] * 1.01
    single_q = json.load(open(os.path.join(ROOT, "profiles", "denoise_quality.json")))
    assert q["default_score"] < single_q["default_score"]
    assert q["rt_denoise_fixed_defaults"]["score"] == single_q["default_score"]


def test_the_form_table_is_the_measured_one():
    """dn_dual_lds_wins and dn_dual_inline_g_wins (rt_host_denoise.inc) must say what tools/denoise_dual_time.py measured: the
    `kept` form and placement per stride of profiles/denoise_dual_time.json, read back here from the source."""
    t = json.load(open(os.path.join(ROOT, "profiles", "denoise_dual_time.json")))
    src = open(os.path.join(ROOT, "rtcuda_amd", "csrc", "rt_host_denoise.inc")).read()
    env = {"false": False, "true": True}

    def ev(body, **names):
        return eval(body.replace("||", " or ").replace("&&", " and "), dict(env, **names))

    lds = re.search(r"bool dn_dual_lds_wins\(int stride\) \{ return (.*?); \}", src).group(1)
    inl = re.search(r"bool dn_dual_inline_g_wins\(int form, int stride\) \{ return (.*?); \}", src).group(1)
    assert len(t["kept"]) == 8
    for i, kept in enumerate(t["kept"]):
        assert ev(lds, stride=1 << i) == (kept == "lds"), (1 << i, kept, lds)
        for form, name in ((1, "direct"), (2, "lds")):
            assert ev(inl, form=form, stride=1 << i) == (t["kept_g"][name][i] == "inline"), (name, 1 << i, inl)


# ----------------------------------------------------------------------------- the surface
def test_new_entry_points_are_declared_exported_bound_and_built(api):
    header = open(os.path.join(ROOT, "include", "rtcuda_amd.h")).read()
    for name in NEW:
        assert name in api.EXPORTS
        assert re.search(rf"^int(64_t)? {name}\(", header, re.M), name
        assert getattr(api.lib(), name).argtypes is not None
    assert "typedef struct rt_denoise_dual_params {" in header
    assert ctypes.sizeof(api.RtDenoiseDualParams) == 20
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bT {name}$", syms, re.M), name
    for name in ("denoise_dual", "denoise_dual_default_params", "denoise_dual_scratch_bytes"):
        assert callable(getattr(api, name))
    all_syms = subprocess.run(["nm", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for kernel in ("k_dn_prepare_dual", "k_dn_var_blur", "k_atrous_varIL", "k_atrous_var_ldsIL", "k_dn_finish_dual"):
        assert re.search(rf" _Z\d+{kernel}", all_syms), kernel
    tools = open(os.path.join(ROOT, "include", "rtcuda_amd_tools.h")).read()
    assert re.search(r"^int rt_denoise_dual_pass_time\(", tools, re.M) and "rt_denoise_dual_pass_time" in api.TOOLS_EXPORTS
    tsyms = subprocess.run(["nm", "-D", "--defined-only", api.TOOLS_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT rt_denoise_dual_pass_time$", tsyms, re.M)
    hpp = open(os.path.join(ROOT, "include", "rtcuda", "rtcuda.hpp")).read()
    assert "inline void denoise_dual(" in hpp and "inline int64_t denoise_dual_scratch_bytes(" in hpp
    per_pixel = api.denoise_dual_scratch_bytes(1, 1)
    assert per_pixel >= 48 and api.denoise_dual_scratch_bytes(33, 17) == per_pixel * 33 * 17
    assert api.lib().rt_denoise_dual_scratch_bytes(0, 1) < 0 and api.lib().rt_denoise_dual_scratch_bytes(1 << 20, 1 << 10) < 0
    assert api.lib().rt_denoise_dual_scratch_bytes(715827882, 1) == per_pixel * 715827882


def test_host_side_errors_name_the_entry_point_and_write_nothing(api, hc):
    """Every refusal comes before a device is needed: host arrays stand in for the device buffers and stay as they were."""
    L = api.lib()
    sa, sb = np.full(3, 7, np.int64), np.full(3, 7, np.int64)
    aov = np.full(ae.CHANNELS, 7, np.int64)
    scratch = np.full(16, 7, np.int64)  # (8-byte items, 16 of them: holds an aligned 64 bytes wherever it starts)
    sp = (scratch.ctypes.data + 15) // 16 * 16
    out = np.full(3, 7, np.float32)
    good = dict(passes=1, sigma_variance=1.0, sigma_depth=1.0, normal_power_log2=1, flags=0)

    def call(a=sa.ctypes.data, na=1, b=sb.ctypes.data, nb=1, v=aov.ctypes.data, aspp=1, w=1, h=1, scr=sp, o=out.ctypes.data, **over):
        prm = api.RtDenoiseDualParams(**dict(good, **over))
        rc = L.rt_denoise_dual_fixed(a, na, b, nb, v, aspp, w, h, ctypes.byref(prm), scr, o, None)
        return rc, L.rt_last_error().decode()

    inf, nan = float("inf"), float("nan")
    cases = [
        (dict(a=None), "null d_sum_a"), (dict(b=None), "null d_sum_b"), (dict(v=None), "null d_aov_fixed"), (dict(scr=None), "null d_scratch"),
        (dict(o=None), "null d_rgb_out"), (dict(w=0), "width and height"), (dict(h=-3), "width and height"),
        (dict(w=1 << 20, h=1 << 10), "more than 715827882 pixels"), (dict(na=0), "samples_a, samples_b and aov_samples"),
        (dict(nb=-1), "samples_a, samples_b and aov_samples"), (dict(aspp=0), "samples_a, samples_b and aov_samples"),
        (dict(na=0x7fffffff, nb=1), "must fit an int32"), (dict(na=1 << 30, nb=1 << 30), "must fit an int32"),
        (dict(scr=sp + 8), "16-byte aligned"),
        (dict(passes=-1), "passes must be 0 .. 8"), (dict(passes=9), "passes must be 0 .. 8"),
        (dict(normal_power_log2=-1), "normal_power_log2 must be 0 .. 8"), (dict(normal_power_log2=9), "normal_power_log2 must be 0 .. 8"),
        (dict(sigma_variance=0.0), "sigma_variance must be finite and positive"), (dict(sigma_variance=-1.0), "sigma_variance must be finite"),
        (dict(sigma_variance=inf), "sigma_variance must be finite"), (dict(sigma_variance=nan), "sigma_variance must be finite"),
        (dict(sigma_depth=0.0), "sigma_depth must be finite and positive"), (dict(sigma_depth=nan), "sigma_depth must be finite"),
        (dict(sigma_variance=1e-30), "variance constant that is not finite"),  # (ks underflows to 0)
        (dict(sigma_variance=1e30), "variance constant that is not finite"),   # (ks overflows)
        (dict(sigma_depth=1e-30), "depth constant that is not finite"), (dict(sigma_depth=1e30), "depth constant"),
        (dict(flags=1), "flags must be 0"),
        (dict(w=1, h=715827882), "needs more than 16777215 workgroups in the pass of stride 1"),
        (dict(w=715827882, h=1, passes=8), "needs more than 16777215 workgroups"),
    ]
    for over, text in cases:
        rc, msg = call(**over)
        assert rc != 0 and msg.startswith("rt_denoise_dual_fixed: ") and text in msg, (over, msg)
    assert L.rt_denoise_dual_default_params(None) != 0
    assert L.rt_last_error().decode() == "rt_denoise_dual_default_params: null out"
    assert (sa == 7).all() and (sb == 7).all() and (aov == 7).all() and (scratch == 7).all() and (out == 7).all()
    # the twin refuses the same parameters
    halves = dd.split_frame(de.synthetic_frame(3, 2), 2, 2)
    for kw in (dict(passes=9), dict(normal_power_log2=9), dict(sigma_variance=0.0), dict(sigma_depth=float("nan")), dict(sigma_variance=1e-30)):
        assert (twin(hc, halves, 3, 2, expect_rc=1, **kw) == -7).all()
    assert (twin(hc, halves[:1] + (0,) + halves[2:], 3, 2, expect_rc=1) == -7).all()


def test_wrapper_rejects_bad_arguments_before_reaching_the_library(api):
    torch = pytest.importorskip("torch")

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    def gpu(x):
        return x.as_subclass(OnGpu)

    a, b, v = (gpu(torch.zeros(8, 3, dtype=torch.int64)), gpu(torch.zeros(8, 3, dtype=torch.int64)), gpu(torch.zeros(8, 11, dtype=torch.int64)))
    f = api.denoise_dual
    cases = [
        ("denoise_dual: beauty_a must be a torch tensor on a GPU", lambda: f(torch.zeros(8, 3, dtype=torch.int64), 1, b, 1, v, 1, 4, 2)),
        ("denoise_dual: beauty_b must be a torch tensor on a GPU", lambda: f(a, 1, np.zeros((8, 3), np.int64), 1, v, 1, 4, 2)),
        ("denoise_dual: aov_sums must be a torch tensor on a GPU", lambda: f(a, 1, b, 1, np.zeros((8, 11), np.int64), 1, 4, 2)),
        (r"denoise_dual: beauty_a must be a contiguous \(8, 3\) torch.int64", lambda: f(gpu(torch.zeros(8, 3)), 1, b, 1, v, 1, 4, 2)),
        (r"denoise_dual: beauty_b must be a contiguous \(6, 3\) torch.int64", lambda: f(gpu(torch.zeros(6, 3, dtype=torch.int64)), 1, b, 1, v, 1, 3, 2)),
        (r"denoise_dual: aov_sums must be a contiguous \(8, 11\) torch.int64", lambda: f(a, 1, b, 1, gpu(torch.zeros(8, 10, dtype=torch.int64)), 1, 4, 2)),
        ("denoise_dual: spp_a must be a positive int", lambda: f(a, 0, b, 1, v, 1, 4, 2)),
        ("denoise_dual: spp_b must be a positive int", lambda: f(a, 1, b, True, v, 1, 4, 2)),
        ("denoise_dual: aov_spp must be a positive int", lambda: f(a, 1, b, 1, v, 1.0, 4, 2)),
        ("denoise_dual: spp_a \\+ spp_b must fit an int32", lambda: f(a, 0x7fffffff, b, 1, v, 1, 4, 2)),
        ("denoise_dual: width must be a positive int", lambda: f(a, 1, b, 1, v, 1, 0, 2)),
        ("denoise_dual: passes must be an int in 0 .. 8", lambda: f(a, 1, b, 1, v, 1, 4, 2, passes=9)),
        ("denoise_dual: normal_power_log2 must be an int in 0 .. 8", lambda: f(a, 1, b, 1, v, 1, 4, 2, normal_power_log2=-1)),
        ("denoise_dual: sigma_variance must be a finite positive number", lambda: f(a, 1, b, 1, v, 1, 4, 2, sigma_variance=0)),
        ("denoise_dual: sigma_depth must be a finite positive number", lambda: f(a, 1, b, 1, v, 1, 4, 2, sigma_depth=float("nan"))),
        ("denoise_dual_scratch_bytes: bad frame size", lambda: api.denoise_dual_scratch_bytes(0, 5)),
        ("denoise_dual_scratch_bytes: width and height must be ints", lambda: api.denoise_dual_scratch_bytes(4.0, 5)),
    ]
    for pattern, call in cases:
        with pytest.raises(api.RtError, match=pattern):
            call()


def test_cpp_wrappers_link_and_throw_the_library_message(api):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "denoisedualcheck"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "denoise_dual_api_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(l.split("=", 1) for l in out.stdout.splitlines())
    dp = dd.default_params()
    assert lines["scratch"] == str(api.denoise_dual_scratch_bytes(33, 17))
    assert lines["defaults"] == f"{dp['passes']} {dp['normal_power_log2']}"
    assert lines["null_out"] == "denoise_dual: rt_denoise_dual_fixed: null d_rgb_out"
    assert lines["passes"] == "denoise_dual: rt_denoise_dual_fixed: passes must be 0 .. 8, it is 9"
    assert lines["sigma"] == "denoise_dual: rt_denoise_dual_fixed: sigma_variance must be finite and positive"
    assert lines["samples"] == "denoise_dual: rt_denoise_dual_fixed: samples_a, samples_b and aov_samples must be at least 1"
    assert lines["size"] == "denoise_dual_scratch_bytes: bad frame size 0 x 4"
    assert lines["out"] == "7 7 7"
