"""GPU tests of the followed AOVs (rt_render_aov_follow_fixed / rt_render_aov_follow_rays_fixed_device).  Run with -m gpu.

What a frame must hold comes from tests/aov_follow_expected.py (numpy, the oracle's trace_closest and mat_step; held to the
oracle's own paths by tests/test_aov_follow_host.py -- ray for ray to the literal frame's log, chain end for chain end to the
per-sample frame -- which also shows that the frames used here hold chains of every kind).  Every comparison is EQUALITY of all 11 int64 channels on all pixels: no tolerance, no masked pixel."""
import ctypes
import os

import numpy as np
import pytest

from conftest import oracle_scene
import aov_expected as ae
import aov_follow_expected as fe
import denoise_expected as de
import denoise_dual_expected as dd
import raytable_keyed as rk

pytestmark = pytest.mark.gpu

POISON = -7
CAPS = (1, 2, 3, 4, 5)


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


def _gpu(api):
    if "full_bsdf" not in _cache:
        from rtcuda_amd import scenes
        _cache["full_bsdf"] = api.Scene(scenes.cornell_bunny("full_bsdf"))
    return _cache["full_bsdf"]


def _modes(api):
    """(name, flags, the oracle's watertight switch)"""
    return [("default", 0, False), ("reference-walk", api.FLAG_REFERENCE_WALK, False), ("watertight", api.FLAG_WATERTIGHT, True)]


def _view(make_camera, w, h, view):
    return ae.wide_camera(make_camera, w / h) if view == "wide" else fe.close_camera(make_camera, w / h)


def _frame(oracle, w, h, spp, cap, watertight, view="wide", shard=(0, 1)):
    """The helper's frame on full_bsdf, computed once per session and argument tuple and never modified."""
    key = (w, h, spp, cap, watertight, view, shard)
    if key not in _cache:
        osc = oracle_scene(oracle, "full_bsdf", watertight)
        sums, ids, chains, _ = fe.frame_expected(oracle, osc, _view(oracle.camera, w, h, view), w, h, spp, cap, shard=shard)
        sums.setflags(write=False)
        ids.setflags(write=False)
        _cache[key] = (sums, ids, chains)
    return _cache[key]


def _assert_sums(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    bad = got != want
    print(what, "sums that differ:", int(bad.sum()), "of", bad.size)
    assert not bad.any(), (what, "sums that differ: %d of %d" % (int(bad.sum()), bad.size), "first (pixel, channel):",
                           np.argwhere(bad)[:6].tolist(), "got", got[bad][:6].tolist(), "want", want[bad][:6].tolist())


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poisoned_ids(torch, n_pixels):
    return torch.full((n_pixels, 2), POISON, dtype=torch.int32, device="cuda")


# ---- 1. a cap of 0 is the first-hit kernel
def test_max_specular_0_is_render_aov_on_the_same_buffers(api, torch):
    gpu = _gpu(api)
    w, h, spp = ae.WIDE_FRAME
    cam = _view(api.make_camera, w, h, "wide")
    for name, flags, _ in _modes(api):
        a, a_ids, a_st = gpu.render_aov(cam, w, h, spp, flags=flags, ids=_poisoned_ids(torch, w * h))
        b, b_ids, b_st = gpu.render_aov_follow(cam, w, h, spp, 0, flags=flags, ids=_poisoned_ids(torch, w * h))
        assert torch.equal(a, b) and torch.equal(a_ids, b_ids), name
        assert b_st["camera_rays"] == b_st["closest_rays"] == a_st["closest_rays"] == w * h * spp
        gpu.render_aov(cam, w, h, spp, flags=flags, out=a)  # added into the same buffers
        gpu.render_aov_follow(cam, w, h, spp, 0, flags=flags, out=b)
        assert torch.equal(a, b), name


# ---- 2. the wide frame at every cap and in every hit mode
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["default", "reference-walk", "watertight"])
@pytest.mark.parametrize("cap", CAPS)
def test_the_wide_frame_is_the_helpers(api, torch, oracle, cap, mode):
    name, flags, watertight = _modes(api)[mode]
    w, h, spp = ae.WIDE_FRAME
    want, want_ids, chains = _frame(oracle, w, h, spp, cap, watertight)
    out, ids, st = _gpu(api).render_aov_follow(_view(api.make_camera, w, h, "wide"), w, h, spp, cap, flags=flags, ids=_poisoned_ids(torch, w * h))
    _assert_sums(out, want, (name, cap))
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert st["camera_rays"] == w * h * spp and st["closest_rays"] == w * h * spp + int(chains["length"].sum()) > w * h * spp
    # the ids are the first hit's, whatever was followed
    assert np.array_equal(want_ids, _frame(oracle, w, h, spp, 1, watertight)[1])


@pytest.mark.parametrize("env", [{"RT_BVH_WIDE": "0"}, {"RT_STACK_CAP": "2"}], ids=["pairs", "wide-overflow"])
def test_the_two_wide_tree_and_the_small_stack(api, torch, oracle, bunny_full_bsdf, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gpu = api.Scene(bunny_full_bsdf)
    w, h, spp = ae.WIDE_FRAME
    for name, flags, watertight in _modes(api):
        for cap in (1, 5):
            out, ids, _ = gpu.render_aov_follow(_view(api.make_camera, w, h, "wide"), w, h, spp, cap, flags=flags, ids=True)
            _assert_sums(out, _frame(oracle, w, h, spp, cap, watertight)[0], (env, name, cap))
            assert np.array_equal(ids.cpu().numpy(), _frame(oracle, w, h, spp, cap, watertight)[1])
    gpu.close()


# ---- 3. splits
def test_shards_add_up_to_the_whole_frame(api, torch, oracle):
    gpu = _gpu(api)
    w, h, spp = ae.WIDE_FRAME
    cam = _view(api.make_camera, w, h, "wide")
    for cap in (2, 5):
        total = torch.zeros((w * h, ae.CHANNELS), dtype=torch.int64, device="cuda")
        for r in range(2):
            out, ids, st = gpu.render_aov_follow(cam, w, h, spp, cap, shard=(r, 2), ids=_poisoned_ids(torch, w * h))
            want, want_ids, _ = _frame(oracle, w, h, spp, cap, False, shard=(r, 2))
            _assert_sums(out, want, ("rank", r, cap))
            assert np.array_equal(ids.cpu().numpy(), want_ids) and (r == 0 or bool((ids == POISON).all()))
            assert st["camera_rays"] == w * h * spp // 2
            gpu.render_aov_follow(cam, w, h, spp, cap, shard=(r, 2), out=total)
        _assert_sums(total, _frame(oracle, w, h, spp, cap, False)[0], ("ranks added", cap))


def test_pinhole_table_chunks_and_a_pixel_array(api, torch, oracle):
    gpu = _gpu(api)
    w, h, spp = ae.WIDE_FRAME
    n = w * h * spp
    cam12 = _view(oracle.camera, w, h, "wide")
    o, d, pixel = rk.keyed_pinhole_table(oracle, cam12, w, h, spp, 1, range(n))
    o, d = _dev(torch, o), _dev(torch, d)
    for name, flags, watertight in _modes(api):
        for cap in (1, 5):
            cam_out, cam_ids, cam_st = gpu.render_aov_follow(_view(api.make_camera, w, h, "wide"), w, h, spp, cap, flags=flags, ids=True)
            out, ids, st = gpu.render_aov_follow_rays(o, d, w * h, cap, rays_per_pixel=spp, flags=flags, ids=True)
            assert torch.equal(out, cam_out) and torch.equal(ids, cam_ids), (name, cap)
            assert st["camera_rays"] == n and st["closest_rays"] == cam_st["closest_rays"]
            _assert_sums(out, _frame(oracle, w, h, spp, cap, watertight)[0], (name, cap, "pinhole table"))
    # (the last mode and cap of the loops above) three uneven chunks into one buffer, forwards and backwards
    cuts = [0, 65, 1000, n]
    pieces = list(zip(cuts[:-1], cuts[1:]))
    for order in (pieces, pieces[::-1]):
        acc = torch.zeros((w * h, ae.CHANNELS), dtype=torch.int64, device="cuda")
        acc_ids = _poisoned_ids(torch, w * h)
        for a, b in order:
            gpu.render_aov_follow_rays(o[a:b].contiguous(), d[a:b].contiguous(), w * h, cap, rays_per_pixel=spp, key_first=a, flags=flags,
                                       out=acc, ids=acc_ids)
        assert torch.equal(acc, cam_out) and torch.equal(acc_ids, cam_ids)
    # a pixel array: the permuted sums
    perm = np.random.default_rng(3).permutation(w * h).astype(np.int32)
    out, ids, _ = gpu.render_aov_follow_rays(o, d, w * h, cap, pixel=_dev(torch, perm[pixel]), flags=flags)
    assert ids is None
    want = np.zeros((w * h, ae.CHANNELS), np.int64)
    want[perm] = _frame(oracle, w, h, spp, cap, watertight)[0]
    _assert_sums(out, want, "permuted d_pixel")
    with pytest.raises(api.RtError, match="ids together with a pixel tensor"):
        gpu.render_aov_follow_rays(o, d, w * h, cap, pixel=_dev(torch, perm[pixel]), ids=True)


def test_the_table_forms_seed_selects_the_streams(api, torch, oracle):
    """The rays of seed 1's close frame under the streams of seed 7: the same first hits, other glass branches."""
    gpu = _gpu(api)
    w, h, spp = fe.SMALL_FRAMES[2]
    n = w * h * spp
    o, d, pixel = rk.keyed_pinhole_table(oracle, _view(oracle.camera, w, h, "close"), w, h, spp, 1, range(n))
    osc = oracle_scene(oracle, "full_bsdf", False)
    want7, _, _ = fe.table_expected(oracle, osc, o, d, pixel, w * h, list(range(n)), fe.FOLLOW_MAX, seed=7)
    want1 = _frame(oracle, w, h, spp, fe.FOLLOW_MAX, False, "close")[0]
    assert not np.array_equal(want7, want1) and np.array_equal(want7[:, ae.EMISSION:ae.EMISSION + 3], want1[:, ae.EMISSION:ae.EMISSION + 3])
    out7, _, _ = gpu.render_aov_follow_rays(_dev(torch, o), _dev(torch, d), w * h, fe.FOLLOW_MAX, seed=7, rays_per_pixel=spp)
    _assert_sums(out7, want7, "seed 7")
    out1, _, _ = gpu.render_aov_follow_rays(_dev(torch, o), _dev(torch, d), w * h, fe.FOLLOW_MAX, rays_per_pixel=spp)
    _assert_sums(out1, want1, "seed 1")


# ---- 4. the walker's new ability at its smallest shapes: fewer samples than a wave, a chunk boundary inside a pixel, whole waves
@pytest.mark.parametrize("w,h,spp", fe.SMALL_FRAMES, ids=["%dx%dx%d" % f for f in fe.SMALL_FRAMES])
def test_small_close_frames_where_lanes_re_arm_next_to_lanes_that_finish(api, torch, oracle, w, h, spp):
    cam = _view(api.make_camera, w, h, "close")
    for name, flags, watertight in _modes(api):
        for cap in (1, 3, 5):
            want, want_ids, chains = _frame(oracle, w, h, spp, cap, watertight, "close")
            out, ids, st = _gpu(api).render_aov_follow(cam, w, h, spp, cap, flags=flags, ids=_poisoned_ids(torch, w * h))
            _assert_sums(out, want, (name, cap, w, h, spp))
            assert np.array_equal(ids.cpu().numpy(), want_ids)
            assert st["closest_rays"] == w * h * spp + int(chains["length"].sum())


# ---- 5. the draws mat() makes behind sample_f depend on the lights
def test_the_skip_follows_the_lights(api, torch, oracle):
    w, h, spp = fe.BOX_FRAME
    base, materials, _, _ = fe.box_scene("mixed")
    gpu = api.Scene(base)
    gpu.set_materials(materials)
    cam = fe.box_camera(api.make_camera, w / h)
    seen = []
    for which in fe.BOX_LIGHTS:
        _, _, lights, tri_light = fe.box_scene(which)
        gpu.set_lights(lights, tri_light)
        arrays = fe.box_arrays(which)
        for name, flags, watertight in _modes(api):
            osc = oracle.scene(arrays).set_watertight(watertight)
            want, want_ids, chains, _ = fe.frame_expected(oracle, osc, fe.box_camera(oracle.camera, w / h), w, h, spp, fe.FOLLOW_MAX)
            out, ids, st = gpu.render_aov_follow(cam, w, h, spp, fe.FOLLOW_MAX, flags=flags, ids=True)
            _assert_sums(out, want, (which, name))
            assert np.array_equal(ids.cpu().numpy(), want_ids)
            assert st["closest_rays"] == w * h * spp + int(chains["length"].sum())
            osc.close()
        seen.append(want)
    # the three frames are three frames: a kernel that skipped alike under every light set would miss two of them
    assert not any(np.array_equal(seen[a], seen[b]) for a, b in ((0, 1), (1, 2), (0, 2)))
    gpu.close()


# ---- 6. refusals
def test_errors_name_the_entry_point_and_leave_the_buffers_untouched(api, torch, oracle):
    gpu = _gpu(api)
    w, h, spp = 8, 8, 4
    n = w * h * spp
    cam = api.make_camera(aspect=w / h)
    o, d, pixel = rk.keyed_pinhole_table(oracle, oracle.camera((0.5, 0.5, 1.5), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8, w / h), w, h, spp, 1, range(n))
    o, d = _dev(torch, o), _dev(torch, d)
    buf = torch.full((w * h, ae.CHANNELS), POISON, dtype=torch.int64, device="cuda")
    ids = _poisoned_ids(torch, w * h)
    c = ctypes.c_void_p

    def untouched():
        torch.cuda.synchronize()
        assert bool((buf == POISON).all()) and bool((ids == POISON).all())

    def refused_camera(fragment, cap=2, flags=0, sums=True):
        rc = gpu.L.rt_render_aov_follow_fixed(gpu.h, cam.ctypes.data, w, h, spp, 1, 0, 1, flags, cap, c(buf.data_ptr() if sums else None),
                                              c(ids.data_ptr()), None, None)
        msg = gpu.L.rt_last_error().decode()
        assert rc != 0 and msg.startswith("rt_render_aov_follow_fixed: ") and fragment in msg, (fragment, rc, msg)
        untouched()

    def refused_rays(fragment, cap=2, flags=0, sums=True, pix=None):
        rc = gpu.L.rt_render_aov_follow_rays_fixed_device(gpu.h, n, c(o.data_ptr()), c(d.data_ptr()), c(None if pix is None else pix.data_ptr()), spp,
                                                          w * h, 1, 0, 1, flags, cap, c(buf.data_ptr() if sums else None), c(ids.data_ptr()),
                                                          None, None)
        msg = gpu.L.rt_last_error().decode()
        assert rc != 0 and msg.startswith("rt_render_aov_follow_rays_fixed_device: ") and fragment in msg, (fragment, rc, msg)
        untouched()

    for refused in (refused_camera, refused_rays):
        refused("max_specular = -1 is outside 0 .. RT_AOV_FOLLOW_MAX", cap=-1)
        refused("max_specular = 6 is outside 0 .. RT_AOV_FOLLOW_MAX", cap=6)
        refused("exclude each other", flags=api.FLAG_REFERENCE_WALK | api.FLAG_WATERTIGHT)
        refused("null d_aov_fixed", sums=False)
    refused_rays("d_ids together with d_pixel", pix=_dev(torch, pixel))
    with pytest.raises(api.RtError, match="rt_render_aov_follow_fixed: max_specular = 6 is outside"):
        gpu.render_aov_follow(cam, w, h, spp, 6)
    with pytest.raises(api.RtError, match="max_specular must be an int"):
        gpu.render_aov_follow(cam, w, h, spp, 1.5)
    # and the scene still renders
    out, _, _ = gpu.render_aov_follow(cam, w, h, spp, 0)
    assert torch.equal(out, gpu.render_aov(cam, w, h, spp)[0])


# ---- 7. the format: the denoisers take followed AOVs as they take first-hit ones
def test_the_denoisers_on_followed_aovs_equal_their_cpu_twins(api, torch):
    hc = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    hc.hc_denoise_dual.argtypes = [vp, ci, vp, ci, vp, ci, ci, ci, ci, cf, cf, ci, vp, vp]
    hc.hc_denoise.argtypes = [vp, ci, vp, ci, ci, ci, ci, cf, cf, ci, vp]
    gpu = _gpu(api)
    w, h, spp = 32, 24, 4
    cam = _view(api.make_camera, w, h, "close")
    halves = []
    for rank in (0, 1):
        t = torch.zeros((h * w, 3), dtype=torch.int64, device="cuda")
        gpu.render_shard_fixed(cam, w, h, spp, rank, 2, t.data_ptr(), flags=api.FLAG_RNG_PER_SAMPLE)
        halves.append(t)
    whole = halves[0] + halves[1]
    first, _, _ = gpu.render_aov(cam, w, h, spp, flags=api.FLAG_WATERTIGHT)
    for cap in (1, 5):
        aov, _, _ = gpu.render_aov_follow(cam, w, h, spp, cap, flags=api.FLAG_WATERTIGHT)
        assert not torch.equal(aov, first)
        a, b, s, v = (np.ascontiguousarray(t.cpu().numpy()) for t in (halves[0], halves[1], whole, aov))
        p1, p2 = de.default_params(), dd.default_params()
        want = np.full((w * h, 3), -7, np.float32)
        assert hc.hc_denoise(s.ctypes.data, spp, v.ctypes.data, spp, w, h, p1["passes"], p1["sigma_color"], p1["sigma_depth"],
                             p1["normal_power_log2"], want.ctypes.data) == 0
        got = api.denoise(whole, spp, aov, spp, w, h).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("denoise", cap)
        want2, var = np.full((w * h, 3), -7, np.float32), np.full(w * h, -7, np.float32)
        assert hc.hc_denoise_dual(a.ctypes.data, spp // 2, b.ctypes.data, spp // 2, v.ctypes.data, spp, w, h, p2["passes"], p2["sigma_variance"],
                                  p2["sigma_depth"], p2["normal_power_log2"], want2.ctypes.data, var.ctypes.data) == 0
        got2 = api.denoise_dual(halves[0], spp // 2, halves[1], spp // 2, aov, spp, w, h).cpu().numpy()
        assert np.array_equal(got2.view(np.uint32), want2.view(np.uint32)), ("denoise_dual", cap)
