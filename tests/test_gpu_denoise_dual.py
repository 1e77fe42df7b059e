"""GPU tests of the dual-buffer denoiser (rt_denoise_dual_fixed through api.denoise_dual).  Run with -m gpu.

What the call must return comes from tests/denoise_dual_expected.py, the numpy restatement of the header's text that
tests/test_denoise_dual_host.py holds the CPU twin to.  Every comparison of an image is EQUALITY of all output floats as bit
patterns: no tolerance, no masked pixel.  A pass has two forms (the direct k_atrous_var and the LDS k_atrous_var_lds, a 32 x 8
tile per workgroup in both: rt_denoise_fixed's pass bodies and tap loop, dn_filter_pixel, with the variance channel switched on)
and two placements of the 3 x 3 variance prefilter (in the pass, or k_dn_var_blur before it); the
knobs RT_DENOISE_FORM and RT_DENOISE_DUAL_G force each, and test_every_form_and_placement_at_every_stride runs all four at
strides 1 to 128 on 33 x 17 and 97 x 19: below, at and beyond a tile, halos and 3 x 3 taps across the image edge, strides beyond
the image."""
import ctypes

import numpy as np
import pytest

from conftest import default_camera, oracle_scene
import aov_expected as ae
import denoise_expected as de
import denoise_dual_expected as dd

pytestmark = pytest.mark.gpu

F32 = np.float32
OTHER = dict(sigma_variance=F32(1.5), sigma_depth=F32(0.3), normal_power_log2=3)


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


def _halves(kind, w, h):
    k = ("halves", kind, w, h)
    if k not in _expected:
        if kind == "extreme":
            _expected[k] = dd.extreme_halves(w, h)
        elif kind == "denormal":
            _expected[k] = dd.denormal_case(w, h)[0]
        else:
            _expected[k] = dd.split_frame(de.synthetic_frame(w, h), *((2, 2) if kind == "equal" else (3, 1)))
        for t in _expected[k]:
            if isinstance(t, np.ndarray):
                t.setflags(write=False)
    return _expected[k]


def _want(kind, w, h, **prm):
    """The restatement's image, computed once per session and never modified."""
    k = (kind, w, h, tuple(sorted((n, float(v)) for n, v in prm.items())))
    if k not in _expected:
        _expected[k] = dd.denoise_dual(*_halves(kind, w, h), w, h, **prm)
        _expected[k].setflags(write=False)
    return _expected[k]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _prm(kw):
    return {k: (float(v) if k.startswith("sigma") else v) for k, v in kw.items()}


def _run(api, torch, halves, w, h, **kw):
    a, spp_a, b, spp_b, aov, aov_spp = halves
    return api.denoise_dual(_dev(torch, a), int(spp_a), _dev(torch, b), int(spp_b), _dev(torch, aov), int(aov_spp), w, h, **_prm(kw))


def _assert_same_bits(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    g, w = dd.bits(got), dd.bits(want)
    assert g.shape == w.shape
    bad = g != w
    print(what, "floats that differ:", int(bad.sum()), "of", bad.size)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[bad][:6].tolist(), np.asarray(want)[bad][:6].tolist())


# ---- 1. sizes and pass counts
SIZES = [(1, 1), (2, 3), (5, 5), (33, 17), (97, 19)]


@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_sizes_and_pass_counts_equal_the_restatement(api, torch, w, h):
    _assert_same_bits(_run(api, torch, _halves("equal", w, h), w, h), _want("equal", w, h), ("defaults", w, h))
    for passes in (0, 1, 2, 5, 8):
        for kind, npow in (("equal", 0), ("unequal", 8)):
            prm = dict(OTHER, passes=passes, normal_power_log2=npow)
            _assert_same_bits(_run(api, torch, _halves(kind, w, h), w, h, **prm), _want(kind, w, h, **prm), (kind, passes, npow, w, h))


# ---- 2. each form and each placement of the prefilter forced, at every stride
@pytest.mark.parametrize("g_place", [1, 2], ids=["g-in-pass", "g-prepass"])
@pytest.mark.parametrize("form", [1, 2], ids=["direct", "lds"])
def test_every_form_and_placement_at_every_stride(api, torch, monkeypatch, form, g_place):
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "1")
    monkeypatch.setenv("RT_DENOISE_FORM", str(form))
    monkeypatch.setenv("RT_DENOISE_DUAL_G", str(g_place))
    prm = dict(OTHER, passes=8)
    for w, h in ((33, 17), (97, 19)):
        _assert_same_bits(_run(api, torch, _halves("unequal", w, h), w, h, **prm), _want("unequal", w, h, **prm), (form, g_place, w, h))
    for w, h in ((1, 1), (5, 5)):
        _assert_same_bits(_run(api, torch, _halves("equal", w, h), w, h, **prm), _want("equal", w, h, **prm), (form, g_place, w, h))
    dprm = dd.denormal_case()[1]
    _assert_same_bits(_run(api, torch, _halves("denormal", 9, 7), 9, 7, **dprm), _want("denormal", 9, 7, **dprm), (form, g_place, "denormal"))
    xprm = dict(OTHER, passes=8, normal_power_log2=8)
    _assert_same_bits(_run(api, torch, _halves("extreme", 33, 17), 33, 17, **xprm), _want("extreme", 33, 17, **xprm), (form, g_place, "extreme"))
    # poisoned scratch and output: every pixel is written by the forced form as well
    w, h = 97, 19
    a, spp_a, b, spp_b, aov, aov_spp = _halves("unequal", w, h)
    scratch = torch.full((api.denoise_dual_scratch_bytes(w, h),), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full((h * w, 3), float("nan"), dtype=torch.float32, device="cuda")
    api.denoise_dual(_dev(torch, a), spp_a, _dev(torch, b), spp_b, _dev(torch, aov), aov_spp, w, h, scratch=scratch, out=out, **_prm(prm))
    _assert_same_bits(out, _want("unequal", w, h, **prm), (form, g_place, "poisoned"))


def test_pass_timer_of_the_lab_runs_every_form_and_placement_to_the_same_bits(api, torch):
    """rt_denoise_dual_pass_time (what tools/denoise_dual_time.py times the kernels with): all four leave the restatement's pass,
    u and v."""
    w, h = 97, 19
    a, spp_a, b, spp_b, aov, aov_spp = _halves("unequal", w, h)
    n = w * h
    scratch = torch.zeros(api.denoise_dual_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    api.denoise_dual(_dev(torch, a), spp_a, _dev(torch, b), spp_b, _dev(torch, aov), aov_spp, w, h, passes=0, scratch=scratch)
    ks, kz, kv = dd.pass_constants(F32(1.5), F32(0.3), spp_a, spp_b)
    u, v, z, nn, _, _ = dd.prepare_dual(a, spp_a, b, spp_b, aov, aov_spp, kv)
    T = api.tools_lib()
    ms = (ctypes.c_float * 2)()
    for stride in (1, 4, 128):
        want_u, want_v = dd.atrous_var_pass(u, v, z, nn, w, h, stride, ks, kz, 3)
        for form in (1, 2):
            for g_place in (1, 2):
                scratch[16 * n:32 * n] = 0xFF
                assert T.rt_denoise_dual_pass_time(scratch.data_ptr(), w, h, stride, form, g_place, 1.5, 0.3, 3, 2, ms) == 0, T.rt_last_error()
                got = scratch[16 * n:32 * n].view(torch.float32).reshape(n, 4).cpu().numpy()
                _assert_same_bits(got[:, :3], want_u, ("pass u", stride, form, g_place))
                _assert_same_bits(got[:, 3], want_v, ("pass v", stride, form, g_place))
                assert ms[0] > 0 and ms[1] > 0
    assert T.rt_denoise_dual_pass_time(scratch.data_ptr(), w, h, 3, 1, 1, 1.5, 0.3, 3, 2, ms) != 0
    assert T.rt_denoise_dual_pass_time(scratch.data_ptr(), w, h, 4, 1, 3, 1.5, 0.3, 3, 2, ms) != 0


# ---- 3. real frames: the GPU's own half frames, against the restatement applied to those sums copied back
def _gpu_scene(api):
    if "scene" not in _expected:
        from rtcuda_amd import scenes
        _expected["scene"] = api.Scene(scenes.cornell_bunny("full_bsdf"))
    return _expected["scene"]


def _gpu_frames(api, torch, w, h, spp, wide=False):
    """(A, B, whole, aov): shards (0, 2) and (1, 2) and the whole-frame call, each into a zeroed buffer."""
    cam = ae.wide_camera(api.make_camera, w / h) if wide else api.make_camera(aspect=w / h)
    bufs = []
    for rank, of in ((0, 2), (1, 2), (0, 1)):
        t = torch.zeros((h * w, 3), dtype=torch.int64, device="cuda")
        _gpu_scene(api).render_shard_fixed(cam, w, h, spp, rank, of, t.data_ptr(), flags=api.FLAG_RNG_PER_SAMPLE)
        bufs.append(t)
    aov, _, _ = _gpu_scene(api).render_aov(cam, w, h, spp, flags=api.FLAG_WATERTIGHT)
    torch.cuda.synchronize()
    return bufs[0], bufs[1], bufs[2], aov


@pytest.mark.parametrize("wide", [False, True], ids=["64x48x4", "wide-32x24x2"])
def test_the_gpus_own_half_frames(api, torch, oracle, wide):
    w, h, spp = ae.WIDE_FRAME if wide else de.REAL_FRAME
    ta, tb, whole, aov = _gpu_frames(api, torch, w, h, spp, wide)
    a, b, s, v = ta.cpu().numpy(), tb.cpu().numpy(), whole.cpu().numpy(), aov.cpu().numpy()
    assert np.array_equal(a + b, s) and a.any() and b.any() and not np.array_equal(a, b)
    if not wide:  # the whole frame is the CPU's
        osc = oracle_scene(oracle, "full_bsdf", True)
        assert np.array_equal(s, de.real_frame(oracle, osc, default_camera(oracle, w / h), w, h, spp)[0])
    for prm in ({}, dict(OTHER, passes=5)):
        got = api.denoise_dual(ta, spp // 2, tb, spp // 2, aov, spp, w, h, **_prm(prm))
        _assert_same_bits(got, dd.denoise_dual(a, spp // 2, b, spp // 2, v, spp, w, h, **prm), ("real", wide, prm))
    assert np.array_equal(ta.cpu().numpy(), a) and np.array_equal(tb.cpu().numpy(), b) and np.array_equal(aov.cpu().numpy(), v)
    # passes = 0 is rt_denoise_fixed on the summed buffer
    _assert_same_bits(api.denoise_dual(ta, spp // 2, tb, spp // 2, aov, spp, w, h, passes=0), api.denoise(whole, spp, aov, spp, w, h, passes=0).cpu().numpy(),
                      "passes = 0")
    # A == B is legal
    got = api.denoise_dual(ta, spp // 2, ta, spp // 2, aov, spp, w, h)
    _assert_same_bits(got, dd.denoise_dual(a, spp // 2, a, spp // 2, v, spp, w, h), "A is B")


# ---- 4. the contract: inputs only read, scratch and output contents before the call do not matter, streams, repeats
def test_inputs_scratch_output_stream_and_repeat(api, torch):
    w, h = 97, 19
    a, spp_a, b, spp_b, aov, aov_spp = _halves("unequal", w, h)
    prm = dict(OTHER, passes=4)
    want = _want("unequal", w, h, **prm)
    ta, tb, tv = _dev(torch, a), _dev(torch, b), _dev(torch, aov)
    need = api.denoise_dual_scratch_bytes(w, h)
    scratch = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")  # (all-ones bits: NaNs wherever a float is read)
    out = torch.full((h * w, 3), float("nan"), dtype=torch.float32, device="cuda")
    got = api.denoise_dual(ta, spp_a, tb, spp_b, tv, aov_spp, w, h, scratch=scratch, out=out, **_prm(prm))
    assert got is out
    _assert_same_bits(out, want, "poisoned scratch and output")
    assert (scratch[need:] == 0xFF).all()  # (nothing past the bytes asked for)
    assert np.array_equal(ta.cpu().numpy(), a) and np.array_equal(tb.cpu().numpy(), b) and np.array_equal(tv.cpu().numpy(), aov)
    again = api.denoise_dual(ta, spp_a, tb, spp_b, tv, aov_spp, w, h, scratch=scratch, **_prm(prm))  # (the scratch as the last call left it)
    _assert_same_bits(again, want, "second call")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    other = api.denoise_dual(ta, spp_a, tb, spp_b, tv, aov_spp, w, h, stream=side, **_prm(prm))  # (synchronous on its stream at return)
    _assert_same_bits(other, want, "non-default stream")
    assert api.denoise_dual_default_params() == {k: (float(v) if k.startswith("sigma") else v) for k, v in dd.default_params().items()}


def test_errors_with_device_buffers_write_nothing(api, torch):
    w, h = 5, 5
    a, spp_a, b, spp_b, aov, aov_spp = _halves("equal", w, h)
    ta, tb, tv = _dev(torch, a), _dev(torch, b), _dev(torch, aov)
    scratch = torch.full((api.denoise_dual_scratch_bytes(w, h),), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((h * w, 3), -7.0, dtype=torch.float32, device="cuda")
    L = api.lib()

    def call(na=spp_a, nb=spp_b, width=w, scr=scratch.data_ptr(), **over):
        prm = api.RtDenoiseDualParams(**dict(dict(passes=2, sigma_variance=1.0, sigma_depth=1.0, normal_power_log2=1, flags=0), **over))
        rc = L.rt_denoise_dual_fixed(ta.data_ptr(), na, tb.data_ptr(), nb, tv.data_ptr(), aov_spp, width, h, ctypes.byref(prm), scr, out.data_ptr(), None)
        return rc, L.rt_last_error().decode()

    for over in (dict(na=0), dict(nb=0), dict(na=0x7fffffff), dict(width=0), dict(scr=scratch.data_ptr() + 4), dict(passes=9),
                 dict(normal_power_log2=-1), dict(sigma_variance=float("nan")), dict(sigma_depth=0.0), dict(sigma_variance=1e-30), dict(flags=2)):
        rc, msg = call(**over)
        assert rc != 0 and msg.startswith("rt_denoise_dual_fixed: "), (over, msg)
    with pytest.raises(api.RtError, match="denoise_dual: scratch must be a contiguous torch.uint8 tensor of at least"):
        api.denoise_dual(ta, spp_a, tb, spp_b, tv, aov_spp, w, h, scratch=scratch[:-1], out=out)
    with pytest.raises(api.RtError, match=r"denoise_dual: out must be a contiguous \(25, 3\) torch.float32"):
        api.denoise_dual(ta, spp_a, tb, spp_b, tv, aov_spp, w, h, scratch=scratch, out=out[:-1])
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (scratch == 0x5A).all()
    assert np.array_equal(ta.cpu().numpy(), a) and np.array_equal(tb.cpu().numpy(), b) and np.array_equal(tv.cpu().numpy(), aov)
    rc, _ = call()  # and the same call with nothing wrong succeeds
    assert rc == 0 and not (out == -7.0).any()
