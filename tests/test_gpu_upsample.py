"""GPU tests of rt_upsample_fixed / rt_upsample_rgb (through api.upsample / api.upsample_rgb).  Run with -m gpu.

What a call must return comes from tests/upsample_expected.py, the numpy restatement of the header's text that
tests/test_upsample_host.py holds the CPU twin to.  Every comparison is EQUALITY: of all output floats as bit patterns, of all
int64 sums.  The shapes are the smallest at which k_upsample can still go wrong:
    17 x 5 -> 34 x 10 (x 2)   a second tile in x and in y, both partial; the footprint's halo clipped on all four sides
    11 x 3 -> 33 x 9  (x 3)   the second tile starts at x = 32, not a multiple of 3: a footprint origin that no tile / factor gives
     9 x 3 -> 36 x 12 (x 4)   two tiles each way
     1 x 1 ->  2 x 2  (x 2)   one low pixel
The inputs are the library's own renders of the bunny at both sizes, and seeded random sums."""
import ctypes
import os

import numpy as np
import pytest

import aov_expected as ae
import denoise_expected as de
import upsample_expected as ue

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(17, 5, 2), (11, 3, 3), (9, 3, 4), (1, 1, 2)]
IDS = ["%dx%dx%d" % s for s in SHAPES]
OTHER = dict(sigma_depth=F32(0.3), normal_power_log2=2)
POISON = -7


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()  # raises if the HIP library is missing: there is no fallback
    return _api


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    return _torch


_cache = {}


def _frozen(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _random_pair(lw, lh, factor):
    """(beauty_lo, spp, aov_lo, aov_spp_lo, aov_hi, aov_spp_hi, rgb_lo), made once per session and never modified."""
    k = ("random", lw, lh, factor)
    if k not in _cache:
        _cache[k] = _frozen(ue.synthetic_pair(lw, lh, factor) + (ue.wild_rgb(lw * lh),))
    return _cache[k]


def _rendered_pair(api, torch, lw, lh, factor):
    """The same tuple from the library's own renders of one camera at both sizes (rgb_lo: the low frame's mean)."""
    k = ("rendered", lw, lh, factor)
    if k not in _cache:
        if "scene" not in _cache:
            from rtcuda_amd import scenes
            _cache["scene"] = api.Scene(scenes.cornell_bunny("full_bsdf"))
        scene, spp = _cache["scene"], 4
        cam = api.make_camera(aspect=lw / lh)
        beauty = torch.zeros((lh * lw, 3), dtype=torch.int64, device="cuda")
        scene.render_shard_fixed(cam, lw, lh, spp, 0, 1, beauty.data_ptr(), flags=api.FLAG_RNG_PER_SAMPLE)
        aov_lo, _, _ = scene.render_aov(cam, lw, lh, spp, flags=api.FLAG_WATERTIGHT)
        aov_hi, _, _ = scene.render_aov(cam, factor * lw, factor * lh, 2, flags=api.FLAG_WATERTIGHT)
        torch.cuda.synchronize()
        b = beauty.cpu().numpy()
        _cache[k] = _frozen((b, spp, aov_lo.cpu().numpy(), spp, aov_hi.cpu().numpy(), 2, de.noisy_mean(b, spp)))
    return _cache[k]


def _want(key, pair, lw, lh, factor, kind, **prm):
    k = ("want", key, lw, lh, factor, kind, tuple(sorted((n, float(v)) for n, v in prm.items())))
    if k not in _cache:
        beauty, spp, aov_lo, s_lo, aov_hi, s_hi, rgb_lo = pair
        rest = (aov_lo, s_lo, lw, lh, factor, aov_hi, s_hi)
        _cache[k] = _frozen(ue.upsample(beauty, spp, *rest, **prm) if kind == "fixed" else ue.upsample_rgb(rgb_lo, *rest, **prm))
    return _cache[k]


def _dev(torch, a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()  # (the session's frames are read-only)


def _prm(kw):
    return {k: (float(v) if k.startswith("sigma") else v) for k, v in kw.items()}


def _run(api, torch, pair, lw, lh, factor, kind, outputs=("rgb", "fixed"), stream=None, **kw):
    """-> (rgb tensor or None, fixed tensor or None, the device inputs)"""
    beauty, spp, aov_lo, s_lo, aov_hi, s_hi, rgb_lo = pair
    n = factor * factor * lw * lh
    out = torch.full((n, 3), float(POISON), dtype=torch.float32, device="cuda") if "rgb" in outputs else None
    out_fixed = torch.full((n, 3), POISON, dtype=torch.int64, device="cuda") if "fixed" in outputs else None
    d_lo, d_hi = _dev(torch, aov_lo), _dev(torch, aov_hi)
    common = dict(out=out, out_fixed=out_fixed, rgb="rgb" in outputs, fixed="fixed" in outputs, stream=stream, **_prm(kw))
    if kind == "fixed":
        low = _dev(torch, beauty)
        got = api.upsample(low, int(spp), d_lo, int(s_lo), lw, lh, factor, d_hi, int(s_hi), **common)
    else:
        low = _dev(torch, rgb_lo)
        got = api.upsample_rgb(low, d_lo, int(s_lo), lw, lh, factor, d_hi, int(s_hi), **common)
    assert got[0] is out and got[1] is out_fixed
    return out, out_fixed, (low, d_lo, d_hi)


def _assert_same_bits(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    g, w = ue.bits(got), ue.bits(want)
    assert g.shape == w.shape
    bad = g != w
    print(what, "floats that differ:", int(bad.sum()), "of", bad.size)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[bad][:6].tolist(), np.asarray(want)[bad][:6].tolist())


def _assert_is(rgb, fixed, want, what):
    if rgb is not None:
        _assert_same_bits(rgb, want[0], what)
    if fixed is not None:
        f = fixed.cpu().numpy()
        bad = f != want[1]
        print(what, "sums that differ:", int(bad.sum()), "of", bad.size)
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:6].tolist())


@pytest.mark.parametrize("lw,lh,factor", SHAPES, ids=IDS)
@pytest.mark.parametrize("kind", ["fixed", "rgb"])
def test_random_sums_equal_the_restatement(api, torch, kind, lw, lh, factor):
    pair = _random_pair(lw, lh, factor)
    for prm in ({}, OTHER):
        want = _want("random", pair, lw, lh, factor, kind, **prm)
        _assert_is(*_run(api, torch, pair, lw, lh, factor, kind, **prm)[:2], want, (kind, lw, lh, factor, sorted(prm)))
    if lw * lh > 1:
        want = _want("random", pair, lw, lh, factor, kind, **OTHER)
        assert want[3].any() and (~want[2] & ~want[3]).any()  # pixels no sample hit and guided pixels


@pytest.mark.parametrize("lw,lh,factor", SHAPES, ids=IDS)
def test_the_librarys_own_renders_equal_the_restatement(api, torch, lw, lh, factor):
    pair = _rendered_pair(api, torch, lw, lh, factor)
    for kind in ("fixed", "rgb"):
        want = _want("rendered", pair, lw, lh, factor, kind)
        _assert_is(*_run(api, torch, pair, lw, lh, factor, kind)[:2], want, ("rendered", kind, lw, lh, factor))
    # the mean of the sums is the same frame whichever way it comes in
    _assert_same_bits(_want("rendered", pair, lw, lh, factor, "rgb")[0], _want("rendered", pair, lw, lh, factor, "fixed")[0])


@pytest.mark.parametrize("outputs", [("rgb",), ("fixed",)], ids=["rgb-alone", "fixed-alone"])
def test_each_output_alone(api, torch, outputs):
    for lw, lh, factor in SHAPES[:3]:
        pair = _random_pair(lw, lh, factor)
        for kind in ("fixed", "rgb"):
            rgb, fixed, _ = _run(api, torch, pair, lw, lh, factor, kind, outputs=outputs)
            assert (rgb is None) != (fixed is None)
            _assert_is(rgb, fixed, _want("random", pair, lw, lh, factor, kind), (outputs, kind, lw, lh, factor))


def test_inputs_are_only_read_and_a_side_stream_orders_the_work(api, torch):
    """The call is enqueued on a side stream behind a fill of its own input, which the test puts there: a call that ran ahead of
    its stream would read the poison."""
    lw, lh, factor = 17, 5, 2
    pair = _random_pair(lw, lh, factor)
    beauty, spp, aov_lo, s_lo, aov_hi, s_hi, rgb_lo = pair
    n = factor * factor * lw * lh
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    src_hi, src_lo = _dev(torch, aov_hi), _dev(torch, aov_lo)
    d_hi = torch.full((n, ae.CHANNELS), POISON, dtype=torch.int64, device="cuda")
    d_lo = torch.full((lw * lh, ae.CHANNELS), POISON, dtype=torch.int64, device="cuda")
    d_b = _dev(torch, beauty)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_hi.copy_(src_hi, non_blocking=True)
        d_lo.copy_(src_lo, non_blocking=True)
    out, out_fixed = api.upsample(d_b, int(spp), d_lo, int(s_lo), lw, lh, factor, d_hi, int(s_hi), stream=side)
    _assert_is(out, out_fixed, _want("random", pair, lw, lh, factor, "fixed"), "side stream")
    assert np.array_equal(d_b.cpu().numpy(), beauty) and np.array_equal(d_lo.cpu().numpy(), aov_lo) and np.array_equal(d_hi.cpu().numpy(), aov_hi)
    rgb, fixed, (low, a, b) = _run(api, torch, pair, lw, lh, factor, "rgb")
    assert np.array_equal(ue.bits(low.cpu().numpy()), ue.bits(rgb_lo)) and np.array_equal(a.cpu().numpy(), aov_lo) and np.array_equal(b.cpu().numpy(), aov_hi)


def test_a_refused_call_leaves_the_outputs_sentinel_bytes(api, torch):
    lw, lh, factor = 9, 3, 4
    pair = _random_pair(lw, lh, factor)
    beauty, spp, aov_lo, s_lo, aov_hi, s_hi, rgb_lo = pair
    n = factor * factor * lw * lh
    d_b, d_c, d_lo, d_hi = _dev(torch, beauty), _dev(torch, rgb_lo), _dev(torch, aov_lo), _dev(torch, aov_hi)
    out = torch.full((n, 3), float(POISON), dtype=torch.float32, device="cuda")
    out_fixed = torch.full((n, 3), POISON, dtype=torch.int64, device="cuda")
    with pytest.raises(api.RtError, match="rt_upsample_fixed: sigma_depth gives a depth constant"):
        api.upsample(d_b, int(spp), d_lo, int(s_lo), lw, lh, factor, d_hi, int(s_hi), out=out, out_fixed=out_fixed, sigma_depth=1e-30)
    with pytest.raises(api.RtError, match="rt_upsample_rgb: sigma_depth gives a depth constant"):
        api.upsample_rgb(d_c, d_lo, int(s_lo), lw, lh, factor, d_hi, int(s_hi), out=out, out_fixed=out_fixed, sigma_depth=1e30)
    L, c = api.lib(), ctypes.c_void_p
    rc = L.rt_upsample_fixed(c(d_b.data_ptr()), int(spp), c(d_lo.data_ptr()), int(s_lo), lw, lh, 5, c(d_hi.data_ptr()), int(s_hi), None,
                             c(out.data_ptr()), c(out_fixed.data_ptr()), None)
    assert rc != 0 and L.rt_last_error().decode() == "rt_upsample_fixed: factor must be 2, 3 or 4"
    rc = L.rt_upsample_rgb(c(d_c.data_ptr()), None, int(s_lo), lw, lh, factor, c(d_hi.data_ptr()), int(s_hi), None, c(out.data_ptr()),
                           c(out_fixed.data_ptr()), None)
    assert rc != 0 and L.rt_last_error().decode() == "rt_upsample_rgb: null d_aov_lo"
    rc = L.rt_upsample_fixed(c(d_b.data_ptr()), 0, c(d_lo.data_ptr()), int(s_lo), lw, lh, factor, c(d_hi.data_ptr()), int(s_hi), None,
                             c(out.data_ptr()), c(out_fixed.data_ptr()), None)
    assert rc != 0 and "must be at least 1" in L.rt_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((out_fixed == POISON).all())


def test_an_upsampled_frame_chains_into_the_denoiser(api, torch):
    """denoise(out_fixed, 1, aov_hi, ...) on the GPU equals hc_denoise on the CPU twin's out_fixed, bit for bit."""
    lw, lh, factor = 17, 5, 2
    w, h = factor * lw, factor * lh
    pair = _rendered_pair(api, torch, lw, lh, factor)
    beauty, spp, aov_lo, s_lo, aov_hi, s_hi, _ = pair
    hc = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    hc.hc_upsample.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, vp, ci, cf, ci, vp, vp, vp]
    hc.hc_denoise.argtypes = [vp, ci, vp, ci, ci, ci, ci, cf, cf, ci, vp]
    up, dn = ue.default_params(), de.default_params()
    b, lo, hi = (np.ascontiguousarray(a, np.int64) for a in (beauty, aov_lo, aov_hi))
    twin_fixed = np.zeros((w * h, 3), np.int64)
    assert hc.hc_upsample(b.ctypes.data, None, spp, lo.ctypes.data, s_lo, lw, lh, factor, hi.ctypes.data, s_hi, up["sigma_depth"],
                          up["normal_power_log2"], None, twin_fixed.ctypes.data, None) == 0
    twin_clean = np.zeros((w * h, 3), np.float32)
    assert hc.hc_denoise(twin_fixed.ctypes.data, 1, hi.ctypes.data, s_hi, w, h, dn["passes"], dn["sigma_color"], dn["sigma_depth"],
                         dn["normal_power_log2"], twin_clean.ctypes.data) == 0
    _, out_fixed, (_, _, d_hi) = _run(api, torch, pair, lw, lh, factor, "fixed", outputs=("fixed",))
    assert np.array_equal(out_fixed.cpu().numpy(), twin_fixed)
    _assert_same_bits(api.denoise(out_fixed, 1, d_hi, int(s_hi), w, h), twin_clean, "upsample -> denoise")
    assert np.isfinite(twin_clean).all() and float(twin_clean.max()) > 0
