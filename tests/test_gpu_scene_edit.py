"""Editing a scene in place: rt_scene_set_materials, rt_scene_set_lights, rt_scene_set_triangles, rt_scene_set_triangles_device
and rt_scene_create_device.  Run with -m gpu.

The bar is exact, as in tests/test_gpu_scene_rebuild.py (whose helpers these are): the edited scene A must give the bits of
a scene B created by rt_scene_create from the target arrays -- every RT_FLAG_DETERMINISTIC pixel, the five event totals, every
ray's hit triangle, t, u, v and occlusion flag in the three hit modes.  So that the pin does not rest on the product alone, at
least one case per entry point also compares A with the CPU oracle rendering the target arrays: event totals and fixed-point
pixel sums at 160 x 120 x 8.  Nothing here provokes a GPU fault: the error cases pass only arguments the library rejects.
"""
import dataclasses
import re

import numpy as np
import pytest

import raygen
import raytable
import table_scenes as ts
from conftest import default_camera, usable_cpus
from test_gpu_multigen import _assert_same_events
from test_gpu_scene_rebuild import (EVENTS, _aimed_rays, _assert_same_hits, _assert_same_renders, _camera, _device_tree, _render,
                                    _tiny, _twin, _view_rays, _with)
from test_scene_update_host import deform

pytestmark = pytest.mark.gpu

ORACLE_FRAME = (160, 120, 8)
SMALL = dict(w=160, h=120, spp=8)


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


def _variant(name, **kw):
    from rtcuda_amd import scenes
    return scenes.cornell_bunny(name, **kw)


def _fixed(api, sc, flags=0):
    """RT_FLAG_DETERMINISTIC-style fixed-point sums and stats of the oracle frame."""
    import torch
    w, h, spp = ORACLE_FRAME
    buf = torch.zeros(h * w * 3, dtype=torch.int64, device="cuda")
    st = sc.render_shard_fixed(api.make_camera(aspect=w / h), w, h, spp, 0, 1, buf.data_ptr(), flags=flags)
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(h, w, 3), st


def _assert_oracle(api, oracle, sc, arrays):
    """A's event totals and fixed-point sums are the oracle's for `arrays` (default kernels against the literal oracle)."""
    w, h, spp = ORACLE_FRAME
    want = np.zeros((h, w, 3), np.int64)
    _, _, st_c = oracle.scene(arrays).render(default_camera(oracle, w / h), w, h, spp, threads=usable_cpus(), fixed_out=want)
    got, st = _fixed(api, sc)
    _assert_same_events(st, st_c, w * h * spp)
    assert np.array_equal(got, want), int((got != want).sum())


def _tensors(arrays, light=True):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arrays.tris, np.float32).reshape(-1, 9)).cuda()
    m = torch.from_numpy(np.ascontiguousarray(arrays.tri_material, np.int32)).cuda()
    l = torch.from_numpy(np.ascontiguousarray(arrays.tri_light, np.int32)).cuda() if light else None
    return t, m, l


def _on_side_stream(call):
    """As test_rebuild_from_new_vertices does: the call ordered on a stream of its own."""
    import torch
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        call()
    torch.cuda.synchronize()


def _structure(sc):
    inf = sc.info()
    return {k: inf[k] for k in ("pairs", "tris", "max_depth", "leaves", "builder", "build_seconds")}, sc.refit_info()


# ------------------------------------------------------------------------------------------------------------- materials
def test_set_materials(api, oracle, bunny_full_bsdf):
    cam = _camera(api, 4 / 3)
    a = api.Scene(bunny_full_bsdf)
    first, ev_first, st = _render(a, cam, api.FLAG_DETERMINISTIC)  # (default kernels: builds the reference's tree)
    assert st["seconds_reference_tree"] > 0
    before = _structure(a)
    # a permutation that changes the type and the albedo behind every index the triangles name
    perm = np.ascontiguousarray(bunny_full_bsdf.materials[::-1])
    assert (perm["type"] != bunny_full_bsdf.materials["type"]).any() and (perm["albedo"] != bunny_full_bsdf.materials["albedo"]).any()
    target = dataclasses.replace(bunny_full_bsdf, materials=perm)
    a.set_materials(perm)
    assert a.arrays.materials.tobytes() == perm.tobytes()
    img, ev, st = _render(a, cam, api.FLAG_DETERMINISTIC)
    assert st["seconds_reference_tree"] == 0 and _structure(a) == before  # nothing was rebuilt
    assert img.tobytes() != first.tobytes()
    _assert_same_renders(api, a, api.Scene(target), cam)
    _assert_oracle(api, oracle, a, target)
    # a longer table: past the LDS gate (65 materials) and back
    long = ts.padded(target, 65)
    assert not ts.lds_tables(len(long.materials), len(long.lights))
    a.set_materials(long.materials)
    _assert_same_renders(api, a, api.Scene(long), cam)
    img65, ev65, _ = _render(a, cam, api.FLAG_DETERMINISTIC)
    assert ev65 == ev and img65.tobytes() == img.tobytes()  # (padding changes no bit)
    for flags in (api.FLAG_DETERMINISTIC | api.FLAG_REFERENCE_WALK, api.FLAG_DETERMINISTIC | api.FLAG_RNG_PER_SAMPLE):
        ia, sa = a.render(cam, 160, 120, 8, flags=flags)
        ib, sb = api.Scene(long).render(cam, 160, 120, 8, flags=flags)
        assert {k: sa[k] for k in EVENTS} == {k: sb[k] for k in EVENTS} and ia.tobytes() == ib.tobytes(), flags
    a.set_materials(bunny_full_bsdf.materials)
    assert ts.lds_tables(len(a.arrays.materials), len(a.arrays.lights))
    again, ev_again, st = _render(a, cam, api.FLAG_DETERMINISTIC)
    assert ev_again == ev_first and again.tobytes() == first.tobytes()
    assert st["seconds_reference_tree"] == 0 and _structure(a) == before


# ---------------------------------------------------------------------------------------------------------------- lights
def _point(pos, intensity):
    from rtcuda_amd import scenes
    l = np.zeros(1, scenes.LIGHT_DTYPE)
    l[0] = (0, pos, -1, intensity)
    return l


def test_set_lights(api, oracle, bunny_matte):
    cam = _camera(api, 4 / 3)
    a = api.Scene(bunny_matte)
    first, ev_first, st = _render(a, cam, api.FLAG_DETERMINISTIC)
    assert st["seconds_reference_tree"] > 0
    before = _structure(a)

    def check(target, with_oracle=False):
        img, ev, st = _render(a, cam, api.FLAG_DETERMINISTIC)
        assert st["seconds_reference_tree"] == 0 and _structure(a) == before
        _assert_same_renders(api, a, api.Scene(target), cam)
        if with_oracle:
            _assert_oracle(api, oracle, a, target)
        return img

    # a point light added (the assignment of the area lights is kept), then moved and re-coloured
    l1 = np.concatenate([bunny_matte.lights, _point((0.5, 0.9, -0.5), (0.3, 0.3, 0.3))])
    a.set_lights(l1)
    i1 = check(dataclasses.replace(bunny_matte, lights=l1))
    l2 = np.concatenate([bunny_matte.lights, _point((0.2, 0.6, -0.3), (0.1, 0.4, 0.2))])
    a.set_lights(l2)
    i2 = check(dataclasses.replace(bunny_matte, lights=l2), with_oracle=True)
    assert i1.tobytes() != i2.tobytes() and i1.tobytes() != first.tobytes()
    # the two area lights in the other order, the triangles' assignment renumbered with them; the point light first
    l3 = np.concatenate([l2[2:3], l2[1:2], l2[0:1]])
    tl3 = np.array(bunny_matte.tri_light, np.int32)
    tl3[bunny_matte.tri_light == 0] = 2
    a.set_lights(l3, tl3)
    assert a.arrays.tri_light.tobytes() == tl3.tobytes()
    check(dataclasses.replace(bunny_matte, lights=l3, tri_light=tl3))
    # down to no lights at all, and back to the first table
    none = np.full(bunny_matte.n_tris, -1, np.int32)
    a.set_lights(bunny_matte.lights[:0], none)
    check(dataclasses.replace(bunny_matte, lights=bunny_matte.lights[:0], tri_light=none))
    a.set_lights(bunny_matte.lights, bunny_matte.tri_light)
    again = check(bunny_matte)
    assert again.tobytes() == first.tobytes()


@pytest.mark.parametrize("n_mats", [65, 64])
def test_set_lights_across_the_lds_gate(api, oracle, n_mats):
    """65 lights -> 64 -> 66 without touching geometry: a point light is dropped, the triangles' light indices renumbered,
    the area lights keep their triangles; then point lights are appended again.  With 64 materials the light count alone
    decides where the tables live (memory -> LDS -> memory); with 65 they stay in memory throughout."""
    arrays = ts.table_scene(n_mats, 65)
    lights, tl = arrays.lights, np.array(arrays.tri_light, np.int32)
    a = api.Scene(arrays)
    cam = _camera(api, 4 / 3)
    _render(a, cam, api.FLAG_DETERMINISTIC, **SMALL)
    before = _structure(a)
    drop = int(np.flatnonzero(lights["type"] == 0)[0])  # the first point light
    l64 = np.delete(lights, drop)
    tl64 = np.where(tl > drop, tl - 1, tl).astype(np.int32)
    assert len(l64) == 64 and (tl != drop).all() and (l64["type"] == 1).sum() == (lights["type"] == 1).sum()
    a.set_lights(l64, tl64)
    t64 = dataclasses.replace(arrays, lights=l64, tri_light=tl64)
    assert ts.lds_tables(n_mats, 64) == (n_mats == 64)
    _assert_same_renders(api, a, api.Scene(t64), cam, **SMALL)
    _assert_oracle(api, oracle, a, t64)
    l66 = np.concatenate([l64, _point((0.3, 0.7, -0.4), (0.05, 0.05, 0.1)), _point((0.7, 0.5, -0.2), (0.1, 0.02, 0.02))])
    a.set_lights(l66)
    t66 = dataclasses.replace(t64, lights=l66)
    assert not ts.lds_tables(n_mats, 66)
    _assert_same_renders(api, a, api.Scene(t66), cam, **SMALL)
    assert _structure(a) == before


# ------------------------------------------------------------------------------------------------------------- triangles
def _steps(bunny_matte):
    bt = np.asarray(bunny_matte.tris, np.float32).reshape(-1, 9)
    return [("four_bunnies", _variant("four_bunnies")), ("box", _variant("matte", bunny=False)),
            ("one_triangle", _tiny(bunny_matte, bt[100:101])), ("sixteen_lights", _variant("sixteen_lights"))]


@pytest.mark.parametrize("via", ["host", "device"])
def test_set_triangles(api, oracle, bunny_matte, via):
    cam = _camera(api, 4 / 3)
    T = api.tools_lib()
    a = api.Scene(bunny_matte, library=T)
    _render(a, cam, api.FLAG_DETERMINISTIC, **SMALL)  # (the reference's tree of the old triangles)
    refits = a.refit_info()["refits"]
    for name, target in _steps(bunny_matte):
        if via == "host":
            a.set_triangles(target)
            assert a.arrays is target
        else:
            t, m, l = _tensors(target, light=name != "one_triangle")  # (no lights: d_tri_light NULL)
            _on_side_stream(lambda: a.set_triangles_tensors(t, m, l, target.materials, target.lights))
            assert a.arrays is None
        inf = a.info()
        assert inf["tris"] == target.n_tris == a.n_tris() and inf["builder"] == "ploc" and inf["build_seconds"] > 0, name
        ri = a.refit_info()
        assert ri["refits"] == refits and ri["sah_ratio"] == 1.0, name
        recs, order, _ = _twin(target.tris)
        r, o = _device_tree(api, a)
        assert np.array_equal(o, order) and r.shape == recs.shape and np.array_equal(r, recs), name
        b = api.Scene(target, library=T)
        if name == "one_triangle":
            o3, d3 = _aimed_rays(target.tris, 20_000, seed=5)
        else:
            o3, d3 = _view_rays(api, n=30_000)
        _assert_same_hits(api, a, b, o3, d3, min_hit=0.2)
        _assert_same_renders(api, a, b, cam, **({} if name != "four_bunnies" else SMALL))
        img, ev, st = _render(a, cam, api.FLAG_DETERMINISTIC | api.FLAG_REFERENCE_WALK, **SMALL)
        img_b, ev_b, _ = _render(b, cam, api.FLAG_DETERMINISTIC | api.FLAG_REFERENCE_WALK, **SMALL)
        assert ev == ev_b and img.tobytes() == img_b.tobytes(), name
        if name in ("box", "sixteen_lights"):
            _assert_oracle(api, oracle, a, target)


# ------------------------------------------------------------------------------------------------- creation from tensors
@pytest.mark.parametrize("variant", ["matte", "full_bsdf", "four_bunnies", "sixteen_lights"])
def test_from_tensors(api, oracle, variant):
    arrays = _variant(variant)
    T = api.tools_lib()
    t, m, l = _tensors(arrays)
    holder = {}
    _on_side_stream(lambda: holder.update(a=api.Scene.from_tensors(t.reshape(-1, 3, 3), m, l, arrays.materials, arrays.lights, library=T)))
    a = holder["a"]
    c = api.Scene(arrays, library=T, device_bvh=True)
    assert a.info()["builder"] == "ploc" and a.info()["tris"] == arrays.n_tris
    ra, oa = _device_tree(api, a)
    rc, oc = _device_tree(api, c)
    assert np.array_equal(oa, oc) and np.array_equal(ra, rc)
    cam = _camera(api, 4 / 3)
    _assert_same_renders(api, a, c, cam)
    o3, d3 = _view_rays(api, n=30_000)
    _assert_same_hits(api, a, c, o3, d3)
    _assert_same_renders(api, a, api.Scene(arrays), cam, **SMALL)  # (and a host-built scene's)
    if variant == "full_bsdf":
        _assert_oracle(api, oracle, a, arrays)
    img, st = a.render_multi(cam, 128, 96, 8, [0, 0], flags=api.FLAG_DETERMINISTIC)  # (the host mirrors: replicas)
    ib, sb = c.render(cam, 128, 96, 8, flags=api.FLAG_DETERMINISTIC)
    assert img.tobytes() == ib.tobytes() and {k: st[k] for k in EVENTS} == {k: sb[k] for k in EVENTS}


# ---------------------------------------------------------------------------------------------------- life after an edit
@pytest.mark.parametrize("via", ["host", "device"])
def test_life_after_set_triangles(api, oracle, bunny_matte, via):
    import torch
    cam = _camera(api, 4 / 3)
    target = _variant("sixteen_lights")
    a = api.Scene(bunny_matte)
    _, _, st = _render(a, cam, api.FLAG_DETERMINISTIC, **SMALL)
    assert st["seconds_reference_tree"] > 0
    a.render_multi(cam, 64, 64, 4, [0, 0], flags=api.FLAG_DETERMINISTIC)
    if via == "host":
        a.set_triangles(target)
    else:
        t, m, l = _tensors(target)
        a.set_triangles_tensors(t, m, l, target.materials, target.lights)
    b = api.Scene(target)
    # the default kernels read the reference's tree: it must be the new triangles'
    ia, ea, st = _render(a, cam, api.FLAG_DETERMINISTIC)
    ib, eb, _ = _render(b, cam, api.FLAG_DETERMINISTIC)
    assert st["seconds_reference_tree"] > 0 and ea == eb and ia.tobytes() == ib.tobytes()
    # queries (the inverse leaf order of the new tree) and a ray-table render
    o_np, d_np = _view_rays(api, n=40_000)
    o, d = torch.from_numpy(o_np).cuda(), torch.from_numpy(d_np).cuda()
    for flags in (0, api.FLAG_WATERTIGHT):
        ha, hb = a.query_closest(o, d, flags=flags), b.query_closest(o, d, flags=flags)
        for x, y in zip(ha, hb):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), flags
        assert (ha[0] >= 0).float().mean() > 0.3
        o2_np, d2_np = raygen.bounce_rays(o_np, d_np, ha[1].cpu().numpy(), (ha[0] >= 0).cpu().numpy(), seed=3, eps=0.0)
        o2, d2 = torch.from_numpy(o2_np).cuda(), torch.from_numpy(d2_np).cuda()
        ex = ha[0][ha[0] >= 0].contiguous()
        assert torch.equal(a.query_any(o2, d2, None, ex, flags=flags), b.query_any(o2, d2, None, ex, flags=flags)), flags
    w, h, spp = 128, 96, 8
    cam_t = api.make_camera(aspect=w / h)
    to, td, tp = (torch.from_numpy(x).cuda() for x in raytable.pinhole_table(oracle, cam_t, w, h, spp))
    sa, sta = a.render_rays(to, td, w * h, pixel=tp, fixed=True)
    sb, stb = b.render_rays(to, td, w * h, pixel=tp, fixed=True)
    assert torch.equal(sa, sb) and {k: sta[k] for k in EVENTS} == {k: stb[k] for k in EVENTS} and bool(sa.any())
    # several devices (or one listed twice): replicas are made from the host mirrors of the new set
    devices = [0, 1] if torch.cuda.device_count() >= 2 else [0, 0]
    multi, stm = a.render_multi(cam, 128, 96, 8, devices, flags=api.FLAG_DETERMINISTIC)
    single, ev, _ = _render(b, cam, api.FLAG_DETERMINISTIC, w=128, h=96, spp=8)
    assert multi.tobytes() == single.tobytes() and {k: stm[k] for k in EVENTS} == ev
    # moved vertices of the NEW count: refit, then rebuild
    new = deform(target.tris, amp=0.02)
    assert new.shape[0] == target.n_tris != bunny_matte.n_tris
    with pytest.raises(api.RtError, match="triangles"):
        a.update(deform(bunny_matte.tris, amp=0.02))  # (the old count)
    if via == "host":
        a.update(new)
    else:
        dev = torch.from_numpy(np.ascontiguousarray(new, np.float32)).cuda()
        a.update_device(dev.data_ptr())  # (the count comes from the library, not from stale arrays)
    assert a.refit_info()["refits"] == 1
    moved = api.Scene(_with(target, new))
    _assert_same_renders(api, a, moved, cam)
    a.rebuild()
    assert a.refit_info()["sah_ratio"] == pytest.approx(1.0, abs=1e-12)
    _assert_same_renders(api, a, moved, cam, **SMALL)
    newer = deform(target.tris, amp=0.01)
    if via == "host":
        a.rebuild(newer)
    else:
        dev = torch.from_numpy(np.ascontiguousarray(newer, np.float32)).cuda()
        a.rebuild_device(dev.data_ptr())
    _assert_same_renders(api, a, api.Scene(_with(target, newer)), cam, **SMALL)
    # and the tables can still be edited afterwards
    a.set_materials(target.materials[::-1].copy())
    _assert_same_renders(api, a, api.Scene(dataclasses.replace(_with(target, newer), materials=target.materials[::-1].copy())), cam, **SMALL)


# ---------------------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_scene_rendering_its_old_bits(api, bunny_matte, monkeypatch):
    import ctypes
    import torch
    cam = _camera(api)
    a = api.Scene(bunny_matte)
    want = _render(a, cam, api.FLAG_DETERMINISTIC, w=128, h=128, spp=8)[:2]
    info = a.info()
    L, n = api.lib(), bunny_matte.n_tris
    mats, lights = np.ascontiguousarray(bunny_matte.materials), np.ascontiguousarray(bunny_matte.lights)
    t, m, l = _tensors(bunny_matte)
    # index ranges in device buffers: one material and three lights out of range; the message names the counts
    bad_m, bad_l = m.clone(), l.clone()
    bad_m[n // 2] = len(mats)
    bad_l[5], bad_l[n // 3], bad_l[n - 1] = len(lights), -2, 1 << 30
    with pytest.raises(api.RtError, match=r"rt_scene_set_triangles_device: 1 of \d+ triangles have d_tri_material out of range and 3 have d_tri_light"):
        a.set_triangles_tensors(t, bad_m, bad_l, mats, lights)
    with pytest.raises(api.RtError, match=r"rt_scene_create_device: 1 of \d+ triangles .* and 0 have d_tri_light"):
        api.Scene.from_tensors(t, bad_m, l, mats, lights)
    # counts: none, and 2^24 (rejected before a buffer is read)
    c = ctypes.c_void_p
    for count, text in ((0, "at least one triangle"), (1 << 24, "2\\^24"), (-1, "negative count")):
        assert L.rt_scene_set_triangles_device(a.h, c(t.data_ptr()), count, c(m.data_ptr()), c(l.data_ptr()), mats.ctypes.data, len(mats),
                                               lights.ctypes.data, len(lights), None) != 0
        msg = L.rt_last_error().decode()
        assert msg.startswith("rt_scene_set_triangles_device: ") and re.search(text, msg), msg
        tris = np.ascontiguousarray(bunny_matte.tris, np.float32)
        assert L.rt_scene_set_triangles(a.h, tris.ctypes.data, count, bunny_matte.tri_material.ctypes.data,
                                        bunny_matte.tri_light.ctypes.data, mats.ctypes.data, len(mats), lights.ctypes.data, len(lights)) != 0
        assert L.rt_last_error().decode().startswith("rt_scene_set_triangles: ")
    # an area light whose triangle is beyond the NEW count
    box = _variant("matte", bunny=False)
    with pytest.raises(api.RtError, match="rt_scene_set_triangles: area light triangle out of range"):
        a.set_triangles(dataclasses.replace(box, lights=lights))  # (the bunny scene's lights name triangles past the box's)
    with pytest.raises(api.RtError, match="rt_scene_set_lights: area light triangle out of range"):
        bad = lights.copy()
        bad["tri"][0] = n
        a.set_lights(bad)
    # tables that do not cover what the triangles name
    used = int(bunny_matte.tri_material.max()) + 1
    with pytest.raises(api.RtError, match="rt_scene_set_materials: the triangles name materials up to"):
        a.set_materials(mats[: used - 1])
    with pytest.raises(api.RtError, match="rt_scene_set_lights: the kept assignment names lights up to"):
        a.set_lights(lights[:1])
    with pytest.raises(api.RtError, match=r"rt_scene_set_lights: tri_light\[\d+\] out of range"):
        a.set_lights(lights[:1], bunny_matte.tri_light)
    with pytest.raises(api.RtError, match="rt_scene_set_materials: unknown material type"):
        weird = mats.copy()
        weird["type"][0] = 7
        a.set_materials(weird)
    with pytest.raises(api.RtError, match=r"rt_scene_set_triangles: tri_material\[\d+\] out of range"):
        a.set_triangles(dataclasses.replace(bunny_matte, materials=mats[: used - 1]))
    # a HOST pointer passed to a device form is an error, not a fault
    tris = np.ascontiguousarray(bunny_matte.tris, np.float32)
    tm, tl = np.ascontiguousarray(bunny_matte.tri_material, np.int32), np.ascontiguousarray(bunny_matte.tri_light, np.int32)
    for args, text in (((c(tris.ctypes.data), n, c(m.data_ptr()), c(l.data_ptr())), "d_tri_p0p1p2 is not device memory"),
                       ((c(t.data_ptr()), n, c(tm.ctypes.data), c(l.data_ptr())), "d_tri_material is not device memory"),
                       ((c(t.data_ptr()), n, c(m.data_ptr()), c(tl.ctypes.data)), "d_tri_light is not device memory")):
        assert L.rt_scene_set_triangles_device(a.h, *args, mats.ctypes.data, len(mats), lights.ctypes.data, len(lights), None) != 0
        assert text in L.rt_last_error().decode(), L.rt_last_error().decode()
        h = ctypes.c_void_p()
        assert L.rt_scene_create_device(*args, mats.ctypes.data, len(mats), lights.ctypes.data, len(lights), None, ctypes.byref(h)) != 0
        assert text in L.rt_last_error().decode() and not h.value
    # null scene
    assert L.rt_scene_set_materials(None, mats.ctypes.data, len(mats)) != 0 and b"rt_scene_set_materials" in L.rt_last_error()
    assert L.rt_scene_set_lights(None, lights.ctypes.data, len(lights), None) != 0 and b"rt_scene_set_lights" in L.rt_last_error()
    torch.cuda.synchronize()
    assert a.info() == info and a.arrays is bunny_matte
    img, ev, _ = _render(a, cam, api.FLAG_DETERMINISTIC, w=128, h=128, spp=8)
    assert ev == want[1] and img.tobytes() == want[0].tobytes()
    # a 2-wide scene takes new tables but no new triangle set
    monkeypatch.setenv("RT_BVH_WIDE", "0")
    two = api.Scene(bunny_matte)
    monkeypatch.delenv("RT_BVH_WIDE")
    with pytest.raises(api.RtError, match="rt_scene_set_triangles: .*2-wide"):
        two.set_triangles(box)
    img, ev, _ = _render(two, cam, api.FLAG_DETERMINISTIC, w=128, h=128, spp=8)
    assert ev == want[1] and img.tobytes() == want[0].tobytes()
    l1 = np.concatenate([lights, _point((0.5, 0.9, -0.5), (0.3, 0.3, 0.3))])
    two.set_lights(l1)
    ia, ea, _ = _render(two, cam, api.FLAG_DETERMINISTIC, w=128, h=128, spp=8)
    ib, eb, _ = _render(api.Scene(dataclasses.replace(bunny_matte, lights=l1)), cam, api.FLAG_DETERMINISTIC, w=128, h=128, spp=8)
    assert ea == eb and ia.tobytes() == ib.tobytes()
