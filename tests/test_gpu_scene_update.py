"""Scenes whose vertices move: rt_scene_update / rt_scene_update_device refit the BVH on the GPU.  Run with -m gpu.

The bar is exact: scene A is created and then updated, scene B is created from scratch with the same vertices, and A must
give B's bits -- every ray's hit triangle, t, u, v and occlusion flag in every mode, every RT_FLAG_DETERMINISTIC pixel and
every event total.  Hits never depend on the product's own tree (include/rtcuda_amd.h, "WHICH HITS A RAY FINDS"), so the
refit tree, B's freshly built tree and the padding either is given must all lead to the same answers.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import raygen
from test_scene_update_host import deform

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028234663852886e38)
EVENTS = ("shade_events", "any_rays", "emission_adds", "shadow_adds", "rr_draws")
LOOKFROM, LOOKAT = np.array([0.5, 0.5, 1.5]), np.array([0.5, 0.5, 0.0])


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


def _with(arrays, tris):
    return dataclasses.replace(arrays, tris=np.ascontiguousarray(tris, np.float32).reshape(-1, 9))


def _moved(tris, case):
    """(new vertices, camera transform) of a test case: the camera moves with the scene where the scene is moved as a whole."""
    t = np.asarray(tris, np.float32).reshape(-1, 9)
    if case == "deform":
        return deform(t), (1.0, np.zeros(3))
    if case == "translate":
        return (t + np.array([100.0, 0.0, 0.0] * 3, np.float32)).astype(np.float32), (1.0, np.array([100.0, 0.0, 0.0]))
    if case == "scale":
        return (t * np.float32(10.0)).astype(np.float32), (10.0, np.zeros(3))
    raise ValueError(case)


def _camera(api, xform, aspect=1.0):
    s, shift = xform
    return api.make_camera(tuple(LOOKFROM * s + shift), tuple(LOOKAT * s + shift), aspect=aspect)


def _rays(api, xform, n=100_000, seed=7):
    """Camera rays of the (moved) view, and rays from far outside the new bounds aimed at the scene: 30 - 60 scene sizes
    away, which makes the updated scene re-pad its records from the refit boxes (ensure_origin_radius)."""
    s, shift = xform
    cam = _camera(api, xform, 16 / 9)
    o, d = raygen.camera_rays(cam, 1920, 1080, n - n // 5, seed=seed)
    rng = np.random.default_rng(seed + 1)
    m = n // 5
    target = (rng.uniform(0.1, 0.9, (m, 3)) * np.array([1.0, 1.0, -1.0])) * s + shift
    dirs = rng.normal(size=(m, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    fo = target - dirs * s * rng.uniform(30.0, 60.0, (m, 1))
    fd = target - fo.astype(np.float32).astype(np.float64)
    fd = (fd / np.linalg.norm(fd, axis=1, keepdims=True)).astype(np.float32)
    return np.concatenate([o, fo.astype(np.float32)]), np.concatenate([d, fd])


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _assert_same_hits(api, a, b, o, d):
    tmax = np.full(len(o), FLT_MAX, np.float32)
    for flags in (0, api.FLAG_WATERTIGHT, api.FLAG_REFERENCE_WALK):
        ta, xa, ua, va = a.trace_closest(o, d, tmax, flags)
        tb, xb, ub, vb = b.trace_closest(o, d, tmax, flags)
        assert np.array_equal(ta, tb), (flags, int((ta != tb).sum()))
        hit = ta >= 0
        assert hit.mean() > 0.3, hit.mean()
        for x, y in ((xa, xb), (ua, ub), (va, vb)):  # (undefined on a miss)
            assert np.array_equal(_bits(x[hit]), _bits(y[hit])), flags
        # shadow-style rays: from the hit points in random directions, the hit triangle excluded
        o2, d2 = raygen.bounce_rays(o, d, xa, hit, seed=flags + 3, eps=0.0)
        ex = ta[hit]
        t2 = np.full(len(o2), FLT_MAX, np.float32)
        oa = a.trace_any(o2, d2, t2, ex, flags)
        ob = b.trace_any(o2, d2, t2, ex, flags)
        assert np.array_equal(oa, ob), (flags, int((oa != ob).sum()))
        assert 0.05 < oa.mean() < 0.95


def _render(sc, cam, flags, w=128, h=128, spp=8):
    img, st = sc.render(cam, w, h, spp, flags=flags)
    return img, {k: st[k] for k in EVENTS}


def _assert_same_renders(api, a, b, cam):
    for flags in (api.FLAG_DETERMINISTIC, api.FLAG_DETERMINISTIC | api.FLAG_WATERTIGHT):
        ia, ea = _render(a, cam, flags)
        ib, eb = _render(b, cam, flags)
        assert ea == eb, (flags, ea, eb)
        assert ia.tobytes() == ib.tobytes(), (flags, float(np.abs(ia - ib).max()))


def _update(api, sc, tris, via):
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    if via == "host":
        sc.update(tris)
        return
    import torch
    dev = torch.from_numpy(tris).cuda()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        sc.update_device(dev.data_ptr(), stream=stream.cuda_stream)
    torch.cuda.synchronize()


@pytest.mark.parametrize("via", ["host", "device"])
@pytest.mark.parametrize("case", ["deform", "translate", "scale"])
def test_updated_scene_traces_like_a_fresh_one(api, bunny_matte, case, via):
    new, xform = _moved(bunny_matte.tris, case)
    a = api.Scene(bunny_matte)
    _update(api, a, new, via)
    b = api.Scene(_with(bunny_matte, new))
    o, d = _rays(api, xform)
    _assert_same_hits(api, a, b, o, d)
    info = a.refit_info()
    assert info["refits"] == 1 and 0.0 < info["seconds_last"] < 0.05
    assert (0.9 < info["sah_ratio"] < 1.2) if case == "deform" else abs(info["sah_ratio"] - 1.0) < 0.01


@pytest.mark.parametrize("via", ["host", "device"])
def test_updated_scene_renders_like_a_fresh_one(api, bunny_full_bsdf, via):
    new = deform(bunny_full_bsdf.tris)
    a = api.Scene(bunny_full_bsdf)
    cam = _camera(api, (1.0, np.zeros(3)))
    _render(a, cam, api.FLAG_DETERMINISTIC)  # (a render before the update: the reference's tree of the old vertices is built)
    _update(api, a, new, via)
    b = api.Scene(_with(bunny_full_bsdf, new))
    _assert_same_renders(api, a, b, cam)


@pytest.mark.parametrize("case", ["translate", "scale"])
def test_moved_scene_renders_like_a_fresh_one(api, bunny_full_bsdf, case):
    new, xform = _moved(bunny_full_bsdf.tris, case)
    a = api.Scene(bunny_full_bsdf)
    a.update(new)
    b = api.Scene(_with(bunny_full_bsdf, new))
    _assert_same_renders(api, a, b, _camera(api, xform))


def test_moving_the_area_light_triangle(api, bunny_full_bsdf):
    """The light-triangle records, areas and normals live in the shading tables: they must follow the light's vertices."""
    light_tris = np.flatnonzero(bunny_full_bsdf.tri_light >= 0)
    assert len(light_tris) > 0
    new = np.array(bunny_full_bsdf.tris, np.float32).reshape(-1, 9)
    v = new[light_tris].reshape(-1, 3)
    c = v.mean(axis=0)
    new[light_tris] = ((v - c) * np.float32(1.3) + c - np.array([0.05, 0.02, 0.1], np.float32)).reshape(-1, 9)
    a = api.Scene(bunny_full_bsdf)
    cam = _camera(api, (1.0, np.zeros(3)))
    before, _ = _render(a, cam, api.FLAG_DETERMINISTIC)
    a.update(new)
    b = api.Scene(_with(bunny_full_bsdf, new))
    _assert_same_renders(api, a, b, cam)
    after, _ = _render(a, cam, api.FLAG_DETERMINISTIC)
    assert before.tobytes() != after.tobytes()


def test_device_built_scene(api, bunny_matte, bunny_full_bsdf):
    a = api.Scene(bunny_full_bsdf, device_bvh=True)
    am = api.Scene(bunny_matte, device_bvh=True)
    assert a.info()["builder"] == "ploc" and am.info()["builder"] == "ploc"
    new_full, new_matte = deform(bunny_full_bsdf.tris), deform(bunny_matte.tris)
    a.update(new_full)
    am.update(new_matte)
    _assert_same_renders(api, a, api.Scene(_with(bunny_full_bsdf, new_full)), _camera(api, (1.0, np.zeros(3))))
    o, d = _rays(api, (1.0, np.zeros(3)), n=50_000)
    _assert_same_hits(api, am, api.Scene(_with(bunny_matte, new_matte)), o, d)


def test_four_bunnies(api):
    from rtcuda_amd import scenes
    arrays = scenes.cornell_bunny("four_bunnies")
    new = deform(arrays.tris, amp=0.005)
    a = api.Scene(arrays)
    a.update(new)
    o, d = _rays(api, (1.0, np.zeros(3)), n=50_000)
    _assert_same_hits(api, a, api.Scene(_with(arrays, new)), o, d)


def test_back_to_the_original_and_ten_chained_updates(api, bunny_full_bsdf):
    cam = _camera(api, (1.0, np.zeros(3)))
    a = api.Scene(bunny_full_bsdf)
    orig = {f: _render(a, cam, f) for f in (api.FLAG_DETERMINISTIC, api.FLAG_DETERMINISTIC | api.FLAG_WATERTIGHT)}
    a.update(deform(bunny_full_bsdf.tris, amp=0.03))
    a.update(bunny_full_bsdf.tris)
    for f, (img, ev) in orig.items():
        img2, ev2 = _render(a, cam, f)
        assert ev2 == ev and img2.tobytes() == img.tobytes(), f
    assert a.refit_info()["sah_ratio"] == pytest.approx(1.0, abs=1e-9)
    last = None
    for k in range(10):
        last = deform(bunny_full_bsdf.tris, amp=0.003 * (k + 1))
        a.update(last)
    assert a.refit_info()["refits"] == 12
    _assert_same_renders(api, a, api.Scene(_with(bunny_full_bsdf, last)), cam)


def test_error_paths_leave_the_scene_as_it_was(api, bunny_matte, monkeypatch):
    cam = _camera(api, (1.0, np.zeros(3)))
    a = api.Scene(bunny_matte)
    want = _render(a, cam, api.FLAG_DETERMINISTIC)
    n = bunny_matte.n_tris
    L = api.lib()
    with pytest.raises(api.RtError, match="triangles"):
        a.update(np.asarray(bunny_matte.tris, np.float32)[:-1])
    assert L.rt_scene_update(a.h, None, n) != 0
    assert L.rt_scene_update(None, np.ascontiguousarray(bunny_matte.tris, np.float32).ctypes.data, n) != 0
    with pytest.raises(api.RtError, match="device memory"):
        a.update_device(np.ascontiguousarray(bunny_matte.tris, np.float32).ctypes.data)  # (a HOST pointer)
    assert L.rt_scene_update_device(a.h, None, n, None) != 0
    r, s, q = ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
    assert L.rt_scene_refit_info(None, ctypes.byref(r), ctypes.byref(s), ctypes.byref(q)) != 0
    assert a.refit_info()["refits"] == 0
    img, ev = _render(a, cam, api.FLAG_DETERMINISTIC)
    assert ev == want[1] and img.tobytes() == want[0].tobytes()
    # the 2-wide experiment format is refused
    monkeypatch.setenv("RT_BVH_WIDE", "0")
    two = api.Scene(bunny_matte)
    monkeypatch.delenv("RT_BVH_WIDE")
    with pytest.raises(api.RtError, match="2-wide"):
        two.update(deform(bunny_matte.tris))
    img, ev = _render(two, cam, api.FLAG_DETERMINISTIC)
    assert ev == want[1] and img.tobytes() == want[0].tobytes()


def test_render_multi_after_an_update(api, bunny_full_bsdf):
    """Replicas made by rt_render_multi before an update are dropped by it: the next multi-device render uses the new vertices.
    (A device listed twice; replicas on a second physical GPU are exercised only where there is one.)"""
    import torch
    cam = _camera(api, (1.0, np.zeros(3)))
    devices = [0, 1] if torch.cuda.device_count() >= 2 else [0, 0]
    a = api.Scene(bunny_full_bsdf)
    a.render_multi(cam, 64, 64, 4, devices, flags=api.FLAG_DETERMINISTIC)  # (replicas of the old geometry, where any)
    new = deform(bunny_full_bsdf.tris)
    a.update(new)
    multi, st = a.render_multi(cam, 128, 128, 8, devices, flags=api.FLAG_DETERMINISTIC)
    single, ev = _render(api.Scene(_with(bunny_full_bsdf, new)), cam, api.FLAG_DETERMINISTIC)
    assert multi.tobytes() == single.tobytes()
    assert {k: st[k] for k in EVENTS} == ev
