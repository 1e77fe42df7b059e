"""CPU tests of the followed AOVs (rt_render_aov_follow_fixed / rt_render_aov_follow_rays_fixed_device): the helper the GPU
tests compare with (tests/aov_follow_expected.py) is held to the oracle's own paths -- every ray of every followed chain
occurs, bit for bit and in path order, among the path rays the oracle's literal frame logs, and every chain's end is what the
per-sample frame of that one sample carries -- the frames the GPU tests
render are shown to hold what they are rendered for, and the entry points are declared / exported / bound / built.  Everything
that renders is in tests/test_gpu_aov_follow.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, oracle_scene
import aov_expected as ae
import aov_follow_expected as fe
import raytable
import raytable_keyed as rk

NEW = ("rt_render_aov_follow_fixed", "rt_render_aov_follow_rays_fixed_device")


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


_frames = {}


def _wide(oracle, max_specular, watertight=True):
    key = (max_specular, watertight)
    if key not in _frames:
        w, h, spp = ae.WIDE_FRAME
        osc = oracle_scene(oracle, "full_bsdf", watertight)
        _frames[key] = fe.frame_expected(oracle, osc, ae.wide_camera(oracle.camera, w / h), w, h, spp, max_specular)
    return _frames[key]


def test_max_specular_0_is_the_first_hit_helper(oracle):
    w, h, spp = ae.WIDE_FRAME
    for watertight in (False, True):
        osc = oracle_scene(oracle, "full_bsdf", watertight)
        cam = ae.wide_camera(oracle.camera, w / h)
        sums, ids, chains, _ = _wide(oracle, 0, watertight)
        want, want_ids, (tri, mat, _, _, _) = ae.frame_expected(oracle, osc, cam, w, h, spp)
        assert np.array_equal(sums, want) and np.array_equal(ids, want_ids)
        assert np.array_equal(chains["tri0"], tri) and np.array_equal(chains["mat0"], mat)
        for shard in ((0, 2), (1, 2)):
            assert np.array_equal(fe.frame_expected(oracle, osc, cam, w, h, spp, 0, shard=shard)[0],
                                  ae.frame_expected(oracle, osc, cam, w, h, spp, shard=shard)[0])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_chains_are_the_logged_paths(oracle, osc, cam, w, h, spp):
    """The oracle's literal frame logs every path ray it traces, round by round.  That frame runs on the slots' streams, not on
    the samples' (the per-sample frame logs nothing), so the helper's `follow` is given the slots' streams: at one generation
    (w * h * spp slots) camera ray c is slot c's first, its stream xorwow_init(seed, c) behind the two jitter draws, and the
    draws that follow are mat()'s.  Every ray of every chain (origin, direction, hit triangle, t) must occur in the log, bit
    for bit and in path order.  -> the chains"""
    n = w * h * spp
    o, d, _ = raytable.pinhole_table(oracle, cam, w, h, spp, 1)
    with np.errstate(over="ignore"):
        st = oracle.xorwow_init_range(1, 0, n).copy()
        raytable._xorwow_next(st)
        raytable._xorwow_next(st)
    chains = fe.follow(oracle, osc, o, d, st, fe.FOLLOW_MAX)
    oracle.raylog_enable(True)
    try:
        osc.render(cam, w, h, spp, max_bounces=6, threads=1)
        log = oracle.raylog_fetch()
    finally:
        oracle.raylog_enable(False)
    od = np.concatenate([_bits(log["closest_o"]), _bits(log["closest_d"])], axis=1)
    where = {}
    for k, row in enumerate(od):
        where.setdefault(row.tobytes(), []).append(k)
    ltri, lt = log["closest_tri"], _bits(log["closest_t"])
    for s in range(n):
        at = -1
        for j, (ro, rd, tri, t) in enumerate(chains["rays"][s]):
            later = [k for k in where.get(np.concatenate([_bits(ro), _bits(rd)]).tobytes(), ()) if k > at]
            assert later, ("a chain ray the oracle's path does not trace", s, j)
            at = later[0]
            assert int(ltri[at]) == tri and (tri < 0 or int(lt[at]) == int(_bits([t])[0])), (s, j, int(ltri[at]), tri)
            assert j > 0 or at == s  # (round 0 logs the camera rays in slot order)
    return chains


def _assert_chain_ends_are_the_per_sample_frames(oracle, osc, cam, w, h, spp, chains, pixel, keys):
    """The tie to the per-sample frame itself, by one-row keyed tables: sample K alone, with max_bounces = the bounce count of
    the vertex its chain ends on + 1, carries the first hit's emission plus what the estimator adds on that last vertex -- which
    Oracle.mat_step says from the stream, beta and hit the chain arrives with (a matte vertex: the light sample, if its shadow
    ray is free; a capped specular one: nothing).  A chain that skipped draws wrongly took other glass branches or draws
    another light sample."""
    o, d, _ = rk.keyed_pinhole_table(oracle, cam, w, h, spp, 1, keys.tolist())
    n_checked = n_lit = 0
    for s in range(len(keys)):
        if chains["ending"][s] == fe.NOTHING:
            continue
        want = chains["vals"][s, ae.EMISSION:ae.EMISSION + 3].copy()
        if chains["ending"][s] != fe.MISS and chains["end_flags"][s] & 2:
            words = chains["end_words"][s]
            so, sd, tmax = words[6:9].copy().view(np.float32), words[9:12].copy().view(np.float32), words[12:13].copy().view(np.float32)
            occluded = osc.trace_any(so[None], sd[None], tmax, np.array([words[16]], np.uint32).view(np.int32))[0]
            if not occluded:
                want = (want + words[13:16].copy().view(np.float32)).astype(np.float32)
                n_lit += 1
        got, _ = osc.render_table(o[s:s + 1], d[s:s + 1], 1, pixel=np.zeros(1, np.int32), max_bounces=int(chains["length"][s]) + 1, seed=1, keyed=True, key_first=int(keys[s]))
        assert np.array_equal(got[0], ae.to_fixed(want)), (s, int(chains["length"][s]), int(chains["ending"][s]), got[0].tolist(), ae.to_fixed(want).tolist())
        n_checked += 1
    return n_checked, n_lit


def test_every_chain_ray_is_a_ray_of_the_oracles_own_path_on_the_wide_view(oracle):
    w, h, spp = ae.WIDE_FRAME
    osc = oracle_scene(oracle, "full_bsdf", True)
    cam = ae.wide_camera(oracle.camera, w / h)
    slot_chains = _assert_chains_are_the_logged_paths(oracle, osc, cam, w, h, spp)
    assert int((slot_chains["length"] == fe.FOLLOW_MAX).sum()) > 0
    _, _, chains, (pixel, keys) = _wide(oracle, fe.FOLLOW_MAX)
    n_checked, n_lit = _assert_chain_ends_are_the_per_sample_frames(oracle, osc, cam, w, h, spp, chains, pixel, keys)
    print("ends checked", n_checked, "of them lit", n_lit)
    assert n_lit > 0


@pytest.mark.parametrize("which", fe.BOX_LIGHTS)
def test_every_chain_ray_is_a_ray_of_the_oracles_own_path_in_the_box(oracle, which):
    """The test of the draw skipping: without lights, with a point light alone and with area lights plus a point light mat()
    draws differently behind sample_f, and a chain that skipped wrongly leaves the oracle's path at its next glass vertex."""
    w, h, spp = fe.BOX_FRAME
    osc = oracle.scene(fe.box_arrays(which)).set_watertight(True)
    cam = fe.box_camera(oracle.camera, w / h)
    _assert_chains_are_the_logged_paths(oracle, osc, cam, w, h, spp)
    _, _, chains, (pixel, keys) = fe.frame_expected(oracle, osc, cam, w, h, spp, fe.FOLLOW_MAX)
    census = fe.chain_census(chains, pixel)
    print(which, census)
    assert census["glass_samples"] >= 0.2 * census["samples"], census
    # a glass step BEHIND a specular vertex: its Schlick draw is the draw that the skipping at that vertex decides
    assert sum(1 for s in chains["steps"] if any(b >= 0 for b in s[1:])) >= 0.05 * census["samples"]
    n_checked, n_lit = _assert_chain_ends_are_the_per_sample_frames(oracle, osc, cam, w, h, spp, chains, pixel, keys)
    assert n_checked > 0 and (which == "none") == (n_lit == 0)
    osc.close()


def test_the_three_light_sets_give_three_different_box_frames(oracle):
    """So that the GPU test of the light-dependent skip cannot pass on a kernel that skips alike under every light set."""
    w, h, spp = fe.BOX_FRAME
    for watertight in (False, True):
        sums = []
        for which in fe.BOX_LIGHTS:
            osc = oracle.scene(fe.box_arrays(which)).set_watertight(watertight)
            sums.append(fe.frame_expected(oracle, osc, fe.box_camera(oracle.camera, w / h), w, h, spp, fe.FOLLOW_MAX)[0])
            osc.close()
        assert not any(np.array_equal(sums[a], sums[b]) for a, b in ((0, 1), (1, 2), (0, 2)))


def test_the_wide_frame_holds_every_kind_of_chain(oracle):
    _, _, chains, (pixel, _) = _wide(oracle, fe.FOLLOW_MAX)
    c = fe.chain_census(chains, pixel)
    print(c)
    assert c["specular_first"] >= 0.05 * c["samples"], c
    assert all(c["lengths"][k] > 0 for k in range(1, fe.FOLLOW_MAX + 1)), c
    assert all(c["endings"][k] > 0 for k in (fe.DIFFUSE, fe.CAP, fe.MISS)), c
    assert all(c["branches"][k] > 0 for k in (fe.REFLECT, fe.REFRACT, fe.CANNOT_REFRACT)), c
    assert c["mixed_pixels"] > 0, c
    # a chain that misses behind a specular vertex adds no hit; the caps below FOLLOW_MAX end more chains early
    sums = _wide(oracle, fe.FOLLOW_MAX)[0]
    assert int(sums[:, ae.HITS].sum()) == c["endings"][fe.DIFFUSE] + c["endings"][fe.CAP]
    for cap in range(1, fe.FOLLOW_MAX):
        assert fe.chain_census(_wide(oracle, cap)[2])["endings"][fe.CAP] > 0


@pytest.mark.parametrize("w,h,spp", fe.SMALL_FRAMES)
def test_the_close_view_re_arms_lanes_next_to_lanes_that_finish(oracle, w, h, spp):
    """In every small frame: samples that re-arm, and (but for the frame of three samples) samples of other chain lengths, so
    that the lanes of one wave re-arm, deposit and refill in the same pass."""
    osc = oracle_scene(oracle, "full_bsdf", False)
    _, _, chains, _ = fe.frame_expected(oracle, osc, fe.close_camera(oracle.camera, w / h), w, h, spp, fe.FOLLOW_MAX)
    c = fe.chain_census(chains)
    print((w, h, spp), c)
    assert c["specular_first"] > 0
    if w * h * spp > 64:
        assert sum(1 for k in range(fe.FOLLOW_MAX + 1) if c["lengths"][k] > 0) >= 3, c
        assert c["specular_first"] >= 0.5 * c["samples"], c


def test_new_entry_points_are_declared_exported_and_bound(api):
    header = open(os.path.join(ROOT, "include", "rtcuda_amd.h")).read()
    for name in NEW:
        assert name in api.EXPORTS
        assert f"int {name}(" in header
        assert getattr(api.lib(), name).argtypes is not None
    assert "#define RT_AOV_FOLLOW_MAX 5" in header and api.AOV_FOLLOW_MAX == fe.FOLLOW_MAX == 5
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bT {name}$", syms, re.M), name
    for name in ("render_aov_follow", "render_aov_follow_rays"):
        assert callable(getattr(api.Scene, name))


def test_symbol_table_has_the_ten_builds_of_k_aov_follow(api):
    syms = subprocess.run(["nm", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for src in ("9AovCamera", "13KeyedRayTable"):
        for wide, literal, verify in ((1, 0, 1), (0, 0, 1), (1, 0, 0), (0, 0, 0), (0, 1, 0)):
            assert f" _Z12k_aov_followI{src}Lb{wide}ELb{literal}ELb{verify}EE" in syms, (src, wide, literal, verify)


def test_null_scene_is_refused_under_the_entry_points_own_name(api):
    """What the library refuses before it needs a device."""
    import ctypes
    L = api.lib()
    buf = (ctypes.c_int64 * 11)(*([7] * 11))
    cam = (ctypes.c_float * 12)()
    rays = (ctypes.c_float * 6)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    assert L.rt_render_aov_follow_fixed(None, p(cam), 1, 1, 1, 1, 0, 1, 0, 1, p(buf), None, None, None) != 0
    assert L.rt_last_error().decode() == "rt_render_aov_follow_fixed: null scene"
    assert L.rt_render_aov_follow_rays_fixed_device(None, 1, p(rays), p(rays), None, 1, 1, 1, 0, 1, 0, 1, p(buf), None, None, None) != 0
    assert L.rt_last_error().decode() == "rt_render_aov_follow_rays_fixed_device: null scene"
    assert list(buf) == [7] * 11


def test_cpp_wrappers_link_and_throw_the_library_message():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "aovfollowcheck"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "aov_follow_api_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(l.split("=", 1) for l in out.stdout.splitlines())
    assert lines["render_aov_follow"] == "render_aov_follow: rt_render_aov_follow_fixed: null scene"
    assert lines["render_aov_follow_rays"] == "render_aov_follow_rays: rt_render_aov_follow_rays_fixed_device: null scene"
    assert lines["out"] == "7 7 7"
