"""A BVH built on the GPU (PLOC): rt_scene_create_flags(RT_SCENE_DEVICE_BVH), rt_scene_rebuild and rt_scene_rebuild_device.
Run with -m gpu.

The bar is exact.  Scene A has a device-built or rebuilt tree, scene B is host-built from the same vertices, and A must give
B's bits: every ray's hit triangle, t, u, v and occlusion flag in every mode, every RT_FLAG_DETERMINISTIC pixel sum and every
event total.  Hits never depend on the product's own tree (include/rtcuda_amd.h, "WHICH HITS A RAY FINDS").  The device
tree itself must be its host twin's (rt_host_check.cpp) bit for bit.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

import placed_scenes
import raygen
from table_scenes import table_scene
from test_scene_update_host import deform

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028234663852886e38)
EVENTS = ("shade_events", "any_rays", "emission_adds", "shadow_adds", "rr_draws")


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


def _with(arrays, tris):
    return dataclasses.replace(arrays, tris=np.ascontiguousarray(tris, np.float32).reshape(-1, 9))


def _camera(api, aspect=1.0):
    return api.make_camera((0.5, 0.5, 1.5), (0.5, 0.5, 0.0), aspect=aspect)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _view_rays(api, n=100_000, seed=7):
    o, d = raygen.camera_rays(_camera(api, 16 / 9), 1920, 1080, n, seed=seed)
    return o, d


def _aimed_rays(tris, n, seed):
    """Rays from all around aimed at random points on the triangles (tiny scenes: most rays hit)."""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    rng = np.random.default_rng(seed)
    c = np.einsum("nk,nka->na", rng.dirichlet((1.0, 1.0, 1.0), n), t[rng.integers(0, len(t), n)])
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    o = (c - 2.0 * dirs).astype(np.float32)
    d = c - o.astype(np.float64)
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _assert_same_hits(api, a, b, o, d, min_hit=0.3):
    tmax = np.full(len(o), FLT_MAX, np.float32)
    for flags in (0, api.FLAG_WATERTIGHT, api.FLAG_REFERENCE_WALK):
        ta, xa, ua, va = a.trace_closest(o, d, tmax, flags)
        tb, xb, ub, vb = b.trace_closest(o, d, tmax, flags)
        assert np.array_equal(_bits(ta), _bits(tb)), (flags, int((ta != tb).sum()))
        hit = ta >= 0
        assert hit.mean() >= min_hit, hit.mean()
        for x, y in ((xa, xb), (ua, ub), (va, vb)):  # (undefined on a miss)
            assert np.array_equal(_bits(x[hit]), _bits(y[hit])), flags
        if not hit.any():
            continue
        o2, d2 = raygen.bounce_rays(o, d, xa, hit, seed=flags + 3, eps=0.0)
        ex = ta[hit]
        t2 = np.full(len(o2), FLT_MAX, np.float32)
        assert np.array_equal(a.trace_any(o2, d2, t2, ex, flags), b.trace_any(o2, d2, t2, ex, flags)), flags


def _render(sc, cam, flags, w=400, h=300, spp=20):
    img, st = sc.render(cam, w, h, spp, flags=flags)
    return img, {k: st[k] for k in EVENTS}, st


def _assert_same_renders(api, a, b, cam, **kw):
    for flags in (api.FLAG_DETERMINISTIC, api.FLAG_DETERMINISTIC | api.FLAG_WATERTIGHT):
        ia, ea, _ = _render(a, cam, flags, **kw)
        ib, eb, _ = _render(b, cam, flags, **kw)
        assert ea == eb, (flags, ea, eb)
        assert ia.tobytes() == ib.tobytes(), (flags, float(np.abs(ia - ib).max()))


# ---------------------------------------------------------------------------------------------- the tree against its twin
def _twin(tris):
    from rtcuda_amd import api
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    L.rt_ploc_build.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    out = np.zeros(4, np.int64)
    assert L.rt_ploc_build(t.ctypes.data, t.shape[0], None, 0, None, out.ctypes.data) == 0
    recs = np.zeros((int(out[0]), 16), np.uint32)
    order = np.zeros(t.shape[0], np.int32)
    assert L.rt_ploc_build(t.ctypes.data, t.shape[0], recs.ctypes.data, len(recs), order.ctypes.data, out.ctypes.data) == 0
    return recs, order, out


def _device_tree(api, sc):
    T = sc.L
    out = np.zeros(2, np.int64)
    assert T.rt_scene_tree_copy(sc.h, None, 0, None, 0, out.ctypes.data) == 0
    recs = np.zeros((int(out[0]), 16), np.uint32)
    order = np.zeros(int(out[1]), np.int32)
    assert T.rt_scene_tree_copy(sc.h, recs.ctypes.data, len(recs), order.ctypes.data, len(order), out.ctypes.data) == 0
    return recs, order


@pytest.mark.parametrize("variant", ["matte", "four_bunnies"])
def test_device_tree_is_the_host_twins(api, variant):
    from rtcuda_amd import scenes
    arrays = scenes.cornell_bunny(variant)
    recs, order, info = _twin(arrays.tris)
    created = api.Scene(arrays, library=api.tools_lib(), device_bvh=True)
    assert created.info()["builder"] == "ploc"
    r, o = _device_tree(api, created)
    assert np.array_equal(o, order)
    assert r.shape == recs.shape and np.array_equal(r, recs), int((r != recs).any(axis=1).sum())
    rebuilt = api.Scene(arrays, library=api.tools_lib())
    assert rebuilt.info()["builder"] == "sah"
    rebuilt.rebuild()
    r2, o2 = _device_tree(api, rebuilt)
    assert np.array_equal(o2, order) and np.array_equal(r2, recs)
    inf = created.info()
    print(f"{variant}: {inf['build_seconds'] * 1e3:.2f} ms device build, {int(info[1])} iterations, depth {int(info[2])}")


# ---------------------------------------------------------------------------------------------- creation option
@pytest.mark.parametrize("variant", ["matte", "full_bsdf", "four_bunnies", "sixteen_lights"])
def test_device_built_scene_traces_and_renders_like_a_host_built_one(api, variant):
    from rtcuda_amd import scenes
    arrays = scenes.cornell_bunny(variant)
    a = api.Scene(arrays, device_bvh=True)
    b = api.Scene(arrays)
    assert a.info()["builder"] == "ploc" and a.info()["tris"] == arrays.n_tris
    o, d = _view_rays(api, n=100_000 if variant == "matte" else 30_000)
    _assert_same_hits(api, a, b, o, d)
    _assert_same_renders(api, a, b, _camera(api, 4 / 3))


def test_table_scene_with_renumbered_light_triangles(api):
    arrays = table_scene(65, 65, seed=1)
    a = api.Scene(arrays)
    a.rebuild()
    b = api.Scene(arrays)
    _assert_same_renders(api, a, b, _camera(api, 4 / 3))
    _assert_same_renders(api, api.Scene(arrays, device_bvh=True), b, _camera(api, 4 / 3), w=160, h=120, spp=8)


# ---------------------------------------------------------------------------------------------- rebuild
def test_update_then_rebuild_resets_the_sah_ratio_and_keeps_the_reference_tree(api, bunny_full_bsdf):
    cam = _camera(api, 4 / 3)
    new = deform(bunny_full_bsdf.tris, amp=0.03)
    a = api.Scene(bunny_full_bsdf)
    a.update(new)
    assert a.refit_info()["sah_ratio"] != 1.0
    _, _, st = _render(a, cam, api.FLAG_DETERMINISTIC, w=64, h=48, spp=2)  # (builds the reference's tree of the new vertices)
    assert st["seconds_reference_tree"] > 0
    a.rebuild()
    assert a.refit_info()["sah_ratio"] == pytest.approx(1.0, abs=1e-12)
    assert a.info()["builder"] == "ploc"
    ia, ea, st = _render(a, cam, api.FLAG_DETERMINISTIC)
    assert st["seconds_reference_tree"] == 0
    ib, eb, _ = _render(api.Scene(_with(bunny_full_bsdf, new)), cam, api.FLAG_DETERMINISTIC)
    assert ea == eb and ia.tobytes() == ib.tobytes()
    o, d = _view_rays(api, n=50_000)
    _assert_same_hits(api, a, api.Scene(_with(bunny_full_bsdf, new)), o, d)


@pytest.mark.parametrize("via", ["host", "device"])
def test_rebuild_from_new_vertices(api, bunny_full_bsdf, via):
    new = deform(bunny_full_bsdf.tris, amp=0.02)
    a = api.Scene(bunny_full_bsdf)
    cam = _camera(api, 4 / 3)
    _render(a, cam, api.FLAG_DETERMINISTIC, w=64, h=48, spp=2)  # (the reference's tree of the old vertices)
    if via == "host":
        a.rebuild(new)
    else:
        import torch
        dev = torch.from_numpy(np.ascontiguousarray(new, np.float32)).cuda()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            a.rebuild_device(dev.data_ptr(), stream=stream.cuda_stream)
        torch.cuda.synchronize()
    b = api.Scene(_with(bunny_full_bsdf, new))
    _assert_same_renders(api, a, b, cam)
    o, d = _view_rays(api, n=50_000)
    _assert_same_hits(api, a, b, o, d)


def test_rebuild_then_update_then_render(api, bunny_full_bsdf):
    a = api.Scene(bunny_full_bsdf)
    a.rebuild(deform(bunny_full_bsdf.tris, amp=0.02))
    new = deform(bunny_full_bsdf.tris, amp=0.01)
    a.update(new)
    assert a.refit_info()["sah_ratio"] == pytest.approx(1.0, abs=0.2)
    _assert_same_renders(api, a, api.Scene(_with(bunny_full_bsdf, new)), _camera(api, 4 / 3))


def test_render_multi_after_a_rebuild(api, bunny_full_bsdf):
    import torch
    cam = _camera(api)
    devices = [0, 1] if torch.cuda.device_count() >= 2 else [0, 0]
    a = api.Scene(bunny_full_bsdf)
    a.render_multi(cam, 64, 64, 4, devices, flags=api.FLAG_DETERMINISTIC)  # (replicas of the old tree, where any)
    new = deform(bunny_full_bsdf.tris)
    a.rebuild(new)
    multi, st = a.render_multi(cam, 128, 128, 8, devices, flags=api.FLAG_DETERMINISTIC)
    single, ev, _ = _render(api.Scene(_with(bunny_full_bsdf, new)), cam, api.FLAG_DETERMINISTIC, w=128, h=128, spp=8)
    assert multi.tobytes() == single.tobytes()
    assert {k: st[k] for k in EVENTS} == ev


def _tiny(arrays, tris):
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    n = t.shape[0]
    return dataclasses.replace(arrays, tris=t, tri_material=np.zeros(n, np.int32), tri_light=np.full(n, -1, np.int32),
                               lights=arrays.lights[:0])


TINY_CASES = ["1", "2", "3", "5", "8", "9", "coincident", "bare_box", "deformed_bunny"]


def _tiny_case(bunny_matte, case):
    from rtcuda_amd import scenes
    bt = np.asarray(bunny_matte.tris, np.float32).reshape(-1, 9)
    if case.isdigit():
        return _tiny(bunny_matte, bt[::997][: int(case)])
    if case == "coincident":
        return _tiny(bunny_matte, np.repeat(bt[100:101], 40, axis=0))
    if case == "bare_box":
        return scenes.cornell_bunny("matte", bunny=False)
    if case == "deformed_bunny":
        return _with(bunny_matte, deform(bt, amp=0.05))
    return placed_scenes.scene(case)[0]  # (equal boxes by the hundred: refused before the builders learned to cut them)


@pytest.mark.parametrize("case", TINY_CASES + ["points_200", "copies_1000"])
def test_tiny_and_degenerate_scenes(api, bunny_matte, case):
    arrays = _tiny_case(bunny_matte, case)
    recs, order, _ = _twin(arrays.tris)
    a = api.Scene(arrays, library=api.tools_lib(), device_bvh=True)
    r, o = _device_tree(api, a)
    assert np.array_equal(o, order) and np.array_equal(r, recs)
    b = api.Scene(arrays, library=api.tools_lib())
    o3, d3 = _view_rays(api, n=20_000) if case in ("bare_box", "deformed_bunny", "points_200", "copies_1000") else _aimed_rays(arrays.tris, 20_000, seed=5)
    _assert_same_hits(api, a, b, o3, d3, min_hit=0.2)
    b.rebuild()
    _assert_same_hits(api, a, b, o3, d3, min_hit=0.2)


def test_errors_leave_the_scene_rendering_its_old_bits(api, bunny_matte, monkeypatch):
    cam = _camera(api)
    a = api.Scene(bunny_matte)
    want = _render(a, cam, api.FLAG_DETERMINISTIC, w=128, h=128, spp=8)[:2]
    n = bunny_matte.n_tris
    L = api.lib()
    with pytest.raises(api.RtError, match="triangles"):
        a.rebuild(np.asarray(bunny_matte.tris, np.float32)[:-1])
    assert L.rt_scene_rebuild(None, None, n) != 0
    with pytest.raises(api.RtError, match="device memory"):
        a.rebuild_device(np.ascontiguousarray(bunny_matte.tris, np.float32).ctypes.data)  # (a HOST pointer)
    assert a.info()["builder"] == "sah"
    img, ev, _ = _render(a, cam, api.FLAG_DETERMINISTIC, w=128, h=128, spp=8)
    assert ev == want[1] and img.tobytes() == want[0].tobytes()
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "1")
    monkeypatch.setenv("RT_BVH_WIDE", "0")
    two = api.Scene(bunny_matte)
    with pytest.raises(api.RtError, match="4-wide"):
        api.Scene(bunny_matte, device_bvh=True)
    monkeypatch.delenv("RT_BVH_WIDE")
    with pytest.raises(api.RtError, match="2-wide"):
        two.rebuild()
    img, ev, _ = _render(two, cam, api.FLAG_DETERMINISTIC, w=128, h=128, spp=8)
    assert ev == want[1] and img.tobytes() == want[0].tobytes()
