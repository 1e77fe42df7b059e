"""GPU tests of the denoiser (rt_denoise_fixed through api.denoise).  Run with -m gpu.

What the call must return comes from tests/denoise_expected.py, the numpy restatement of the header's text that
tests/test_denoise_host.py holds the CPU twin to.  Every comparison of an image is EQUALITY of all output floats as bit patterns:
no tolerance, no masked pixel.  The pass has two forms, the direct k_atrous and the LDS k_atrous_lds (a 32 x 8 tile per workgroup in
both, of pixels and of one residue's sub-image; both are wrappers of one tap loop, dn_filter_pixel, which the dual filter's pass
kernels share); the sizes put the image edge, the tile edge and every stride on both sides of
each other, and test_both_forms_at_every_stride forces each form (the RT_DENOISE_FORM knob) whatever the library would choose."""
import ctypes

import numpy as np
import pytest

from conftest import default_camera, oracle_scene
import aov_expected as ae
import denoise_expected as de

pytestmark = pytest.mark.gpu

F32 = np.float32
OTHER = dict(sigma_color=F32(0.7), sigma_depth=F32(0.3), normal_power_log2=3)  # (wider than the defaults: more taps carry weight)


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


def _want(key, frame, w, h, **prm):
    """The restatement's image, computed once per session and never modified."""
    k = (key, w, h, tuple(sorted((n, float(v)) for n, v in prm.items())))
    if k not in _expected:
        _expected[k] = de.denoise(*frame, w, h, **prm)
        _expected[k].setflags(write=False)
    return _expected[k]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(api, torch, frame, w, h, **kw):
    beauty, spp, aov, aov_spp = frame
    prm = {k: (float(v) if k.startswith("sigma") else v) for k, v in kw.items()}
    return api.denoise(_dev(torch, beauty), int(spp), _dev(torch, aov), int(aov_spp), w, h, **prm)


def _assert_same_bits(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    g, w = de.bits(got), de.bits(want)
    assert g.shape == w.shape
    bad = g != w
    print(what, "floats that differ:", int(bad.sum()), "of", bad.size)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[bad][:6].tolist(), np.asarray(want)[bad][:6].tolist())


# ---- 1. sizes: one pixel, smaller than the kernel, one tile and its edge, several tiles, a width one past a multiple of the tile
SIZES = [(1, 1), (3, 2), (5, 5), (31, 7), (33, 17), (64, 48), (97, 19)]


@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d%s" % (w, h, "-tile32x8-plus-one" if (w, h) == (97, 19) else "") for w, h in SIZES])
def test_sizes_equal_the_restatement(api, torch, w, h):
    frame = de.synthetic_frame(w, h)
    _assert_same_bits(_run(api, torch, frame, w, h), _want("syn", frame, w, h), ("defaults", w, h))
    prm = dict(OTHER, passes=3)
    _assert_same_bits(_run(api, torch, frame, w, h, **prm), _want("syn", frame, w, h, **prm), ("3 passes", w, h))


# ---- 2. every stride, at sizes where its halo crosses the image edge (stride 128 exceeds both images)
@pytest.mark.parametrize("w,h", [(33, 17), (64, 48)])
@pytest.mark.parametrize("passes", [0, 1, 2, 5, 8])
def test_every_pass_count_equals_the_restatement(api, torch, passes, w, h):
    frame = de.synthetic_frame(w, h)
    for npow in (0, 8) if (w, h) == (33, 17) else (3,):
        prm = dict(OTHER, passes=passes, normal_power_log2=npow)
        _assert_same_bits(_run(api, torch, frame, w, h, **prm), _want("syn", frame, w, h, **prm), (passes, npow, w, h))


# ---- 2b. each form forced, at every stride: sizes below, at and beyond a tile, halos that cross the image edge, strides beyond the image
@pytest.mark.parametrize("form", [1, 2], ids=["direct", "lds"])
def test_both_forms_at_every_stride(api, torch, monkeypatch, form):
    monkeypatch.setenv("RT_DENOISE_FORM", str(form))
    for w, h in ((1, 1), (5, 5), (33, 17), (64, 48), (97, 19), (130, 70)):
        frame = de.synthetic_frame(w, h)
        prm = dict(OTHER, passes=8)
        _assert_same_bits(_run(api, torch, frame, w, h, **prm), _want("syn", frame, w, h, **prm), (form, w, h))
    (frame, prm), (w, h) = de.denormal_case(), (9, 7)
    _assert_same_bits(_run(api, torch, frame, w, h, **prm), _want("denormal", frame, w, h, **prm), (form, "denormal weights"))
    frame = de.extreme_frame(33, 17)
    prm = dict(OTHER, passes=8, normal_power_log2=8)
    _assert_same_bits(_run(api, torch, frame, 33, 17, **prm), _want("extreme", frame, 33, 17, **prm), (form, "extreme"))
    # poisoned scratch and output: every pixel is written by the forced form as well
    w, h = 130, 70
    frame = de.synthetic_frame(w, h)
    scratch = torch.full((api.denoise_scratch_bytes(w, h),), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full((h * w, 3), float("nan"), dtype=torch.float32, device="cuda")
    api.denoise(_dev(torch, frame[0]), frame[1], _dev(torch, frame[2]), frame[3], w, h, passes=8, sigma_color=0.7, sigma_depth=0.3,
                normal_power_log2=3, scratch=scratch, out=out)
    _assert_same_bits(out, _want("syn", frame, w, h, **dict(OTHER, passes=8)), (form, "poisoned"))


def test_pass_timer_of_the_lab_runs_both_forms_to_the_same_bits(api, torch):
    """rt_denoise_pass_time (what tools/denoise_time.py times the kernels with): both forms leave the restatement's pass."""
    w, h = 97, 19
    frame = de.synthetic_frame(w, h)
    n = w * h
    scratch = torch.zeros(api.denoise_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    api.denoise(_dev(torch, frame[0]), frame[1], _dev(torch, frame[2]), frame[3], w, h, passes=0, scratch=scratch)
    u, z, nn, _, _ = de.prepare(*frame)
    T = api.tools_lib()
    ms = (ctypes.c_float * 2)()
    for stride in (1, 4, 128):
        kc, kz = de.pass_constants(stride.bit_length(), F32(0.7), F32(0.3))
        want = de.atrous_pass(u, z, nn, w, h, stride, kc[-1], kz, 3)
        for form in (1, 2):
            scratch[16 * n:32 * n] = 0xFF
            assert T.rt_denoise_pass_time(scratch.data_ptr(), w, h, stride, form, 0.7, 0.3, 3, 2, ms) == 0, T.rt_last_error()
            got = scratch[16 * n:32 * n].view(torch.float32).reshape(n, 4).cpu().numpy()
            _assert_same_bits(got[:, :3], want, ("pass", stride, form))
            assert ms[0] > 0 and ms[1] > 0
    assert T.rt_denoise_pass_time(scratch.data_ptr(), w, h, 3, 1, 0.7, 0.3, 3, 2, ms) != 0


# ---- 3. real frames: the GPU's own sums, denoised, against the restatement applied to those sums copied back
def _gpu_scene(api):
    if "scene" not in _expected:
        from rtcuda_amd import scenes
        _expected["scene"] = api.Scene(scenes.cornell_bunny("full_bsdf"))
    return _expected["scene"]


def _gpu_frame(api, torch, w, h, spp, wide=False):
    cam = ae.wide_camera(api.make_camera, w / h) if wide else api.make_camera(aspect=w / h)
    beauty = torch.zeros((h * w, 3), dtype=torch.int64, device="cuda")
    _gpu_scene(api).render_shard_fixed(cam, w, h, spp, 0, 1, beauty.data_ptr(), flags=api.FLAG_RNG_PER_SAMPLE)
    aov, _, _ = _gpu_scene(api).render_aov(cam, w, h, spp, flags=api.FLAG_WATERTIGHT)
    torch.cuda.synchronize()
    return beauty, aov


@pytest.mark.parametrize("wide", [False, True], ids=["64x48x4", "wide-32x24x2"])
def test_real_frames_equal_the_restatement_of_their_own_sums(api, torch, oracle, wide):
    w, h, spp = ae.WIDE_FRAME if wide else de.REAL_FRAME
    beauty, aov = _gpu_frame(api, torch, w, h, spp, wide)
    b, a = beauty.cpu().numpy(), aov.cpu().numpy()
    full, partial, empty = ae.frame_census(a, spp)
    if wide:
        assert empty >= w * h // 20 and partial > 0 and full > 0  # (many misses and partial coverage)
    else:
        # the sums are the CPU's: the oracle's per-sample frame and the helper's AOV frame
        osc = oracle_scene(oracle, "full_bsdf", True)
        cb, _, ca, _ = de.real_frame(oracle, osc, default_camera(oracle, w / h), w, h, spp)
        assert np.array_equal(b, cb) and np.array_equal(a, ca)
    for prm in ({}, dict(OTHER, passes=5)):
        got = api.denoise(beauty, spp, aov, spp, w, h, **{k: (float(v) if k.startswith("sigma") else v) for k, v in prm.items()})
        _assert_same_bits(got, de.denoise(b, spp, a, spp, w, h, **prm), ("real", wide, prm))
    assert np.array_equal(beauty.cpu().numpy(), b) and np.array_equal(aov.cpu().numpy(), a)


def test_it_denoises_the_gpus_own_frame(api, torch, oracle):
    """The quality inequality of tests/test_denoise_host.py once more, on the sums the GPU rendered."""
    w, h, spp = de.REAL_FRAME
    beauty, aov = _gpu_frame(api, torch, w, h, spp)
    osc = oracle_scene(oracle, "full_bsdf", True)
    ref = de.reference_mean(oracle, osc, default_camera(oracle, w / h), w, h)
    noisy = de.rms(de.noisy_mean(beauty.cpu().numpy(), spp), ref)
    clean = de.rms(api.denoise(beauty, spp, aov, spp, w, h).cpu().numpy(), ref)
    print(f"{w}x{h}x{spp}: rms noisy {noisy:.6f} denoised {clean:.6f} ratio {clean / noisy:.4f}")
    assert clean < noisy


# ---- 4. the edges of the number formats
def test_denormal_weights_and_extreme_sums_equal_the_restatement(api, torch):
    (frame, prm), (w, h) = de.denormal_case(), (9, 7)
    _assert_same_bits(_run(api, torch, frame, w, h, **prm), _want("denormal", frame, w, h, **prm), "denormal weights")
    for w, h in ((33, 17), (5, 5)):
        frame = de.extreme_frame(w, h)
        for passes, npow in ((0, 0), (1, 8), (5, 0), (8, 8)):
            prm = dict(OTHER, passes=passes, normal_power_log2=npow)
            _assert_same_bits(_run(api, torch, frame, w, h, **prm), _want("extreme", frame, w, h, **prm), ("extreme", w, h, passes, npow))


# ---- 5. the contract: inputs only read, scratch and output contents before the call do not matter, streams, repeats
def test_inputs_scratch_output_stream_and_repeat(api, torch):
    w, h = 97, 19
    frame = de.synthetic_frame(w, h)
    prm = dict(passes=4, sigma_color=0.7, sigma_depth=0.3, normal_power_log2=3)
    want = _want("syn", frame, w, h, **dict(OTHER, passes=4))
    beauty, aov = _dev(torch, frame[0]), _dev(torch, frame[2])
    need = api.denoise_scratch_bytes(w, h)
    scratch = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")  # (all-ones bits: NaNs wherever a float is read)
    out = torch.full((h * w, 3), float("nan"), dtype=torch.float32, device="cuda")
    got = api.denoise(beauty, frame[1], aov, frame[3], w, h, scratch=scratch, out=out, **prm)
    assert got is out
    _assert_same_bits(out, want, "poisoned scratch and output")  # (every output float was written: no NaN is left)
    assert (scratch[need:] == 0xFF).all()  # (nothing past the bytes asked for)
    assert np.array_equal(beauty.cpu().numpy(), frame[0]) and np.array_equal(aov.cpu().numpy(), frame[2])
    again = api.denoise(beauty, frame[1], aov, frame[3], w, h, scratch=scratch, **prm)  # (the scratch as the last call left it)
    _assert_same_bits(again, want, "second call")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    other = api.denoise(beauty, frame[1], aov, frame[3], w, h, stream=side, **prm)  # (synchronous on its stream at return)
    _assert_same_bits(other, want, "non-default stream")
    assert api.denoise_default_params() == {k: (float(v) if k.startswith("sigma") else v) for k, v in de.default_params().items()}


def test_errors_with_device_buffers_write_nothing(api, torch):
    w, h = 5, 5
    frame = de.synthetic_frame(w, h)
    beauty, aov = _dev(torch, frame[0]), _dev(torch, frame[2])
    scratch = torch.full((api.denoise_scratch_bytes(w, h),), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((h * w, 3), -7.0, dtype=torch.float32, device="cuda")
    L = api.lib()

    def call(spp=frame[1], width=w, scr=scratch.data_ptr(), **over):
        prm = api.RtDenoiseParams(**dict(dict(passes=2, sigma_color=1.0, sigma_depth=1.0, normal_power_log2=1, flags=0), **over))
        rc = L.rt_denoise_fixed(beauty.data_ptr(), spp, aov.data_ptr(), frame[3], width, h, ctypes.byref(prm), scr, out.data_ptr(), None)
        return rc, L.rt_last_error().decode()

    for over in (dict(spp=0), dict(width=0), dict(scr=scratch.data_ptr() + 4), dict(passes=9), dict(normal_power_log2=-1),
                 dict(sigma_color=float("nan")), dict(sigma_depth=0.0), dict(sigma_color=1e-30), dict(flags=2)):
        rc, msg = call(**over)
        assert rc != 0 and msg.startswith("rt_denoise_fixed: "), (over, msg)
    with pytest.raises(api.RtError, match="denoise: scratch must be a contiguous torch.uint8 tensor of at least"):
        api.denoise(beauty, frame[1], aov, frame[3], w, h, scratch=scratch[:-1], out=out)
    with pytest.raises(api.RtError, match=r"denoise: out must be a contiguous \(25, 3\) torch.float32"):
        api.denoise(beauty, frame[1], aov, frame[3], w, h, scratch=scratch, out=out[:-1])
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (scratch == 0x5A).all()
    assert np.array_equal(beauty.cpu().numpy(), frame[0]) and np.array_equal(aov.cpu().numpy(), frame[2])
    rc, _ = call()  # and the same call with nothing wrong succeeds
    assert rc == 0 and not (out == -7.0).any()
