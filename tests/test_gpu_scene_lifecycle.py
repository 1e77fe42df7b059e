"""The life of a scene's device arrays: whichever entry point builds or replaces a tree (create with either builder, create on
the device, set_triangles*, rebuild*) goes through one build / emit / adopt path in the library, and the table edits hand their
subsets over in the same place.  Two things follow that no other suite pins: an edit gives back what it replaces, and every
way in ends in the same scene.  Run with -m gpu.
"""
import numpy as np
import pytest

from test_gpu_scene_rebuild import EVENTS, _aimed_rays, _assert_same_hits, _camera
from test_scene_update_host import deform

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


def _tensors(arrays):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(arrays.tris, np.float32).reshape(-1, 9)).cuda(),
            torch.from_numpy(np.ascontiguousarray(arrays.tri_material, np.int32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(arrays.tri_light, np.int32)).cuda())


def _free():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


# ---------------------------------------------------------------------------------------------- edits give back what they replace
def test_edits_and_destroy_give_back_what_they_replace(api, bunny_matte):
    """Eight rounds of every edit at constant sizes, two of them rejected after the library has begun its work, may cost at
    most ONE triangle-record array (48 B x n, about 3 MB) of free device memory.  A path that drops a generation of leaf-order
    arrays loses about twenty times that over the rounds, a single per-triangle array never freed at least 2.7 times: the
    bound is a condition, not a measurement.  Then the same bound for creating and destroying the scene."""
    arrays = bunny_matte
    n = len(arrays.tris)
    bound = 48 * n
    moved = deform(arrays.tris, 0.02)
    t, m, l = _tensors(arrays)
    bad_m = m.clone()
    bad_m[n // 2] = len(arrays.materials)
    bad_lights = arrays.lights.copy()
    area = np.flatnonzero(bad_lights["type"] == 1)
    assert len(area) > 0
    bad_lights["tri"][area[0]] = n
    sc = api.Scene(arrays)

    def one_round():
        sc.set_materials(arrays.materials)
        sc.set_lights(arrays.lights)
        sc.set_lights(arrays.lights, arrays.tri_light)
        sc.set_triangles(arrays)
        sc.set_triangles_tensors(t, m, l, arrays.materials, arrays.lights)
        sc.rebuild()
        sc.rebuild(moved)
        sc.update(arrays.tris)
        with pytest.raises(api.RtError, match=r"1 of \d+ triangles have d_tri_material out of range"):
            sc.set_triangles_tensors(t, bad_m, l, arrays.materials, arrays.lights)
        with pytest.raises(api.RtError, match="rt_scene_set_lights: area light triangle out of range"):
            sc.set_lights(bad_lights)

    one_round()  # warm-up: whatever the first use of an entry point keeps (refit levels, code objects) is in place
    before = _free()
    for _ in range(8):
        one_round()
    drift = before - _free()
    print(f"edits: free device memory fell by {drift} B over 8 rounds (bound {bound} B)")
    assert drift <= bound, (drift, bound)

    sc.close()
    before = _free()
    for _ in range(2):
        api.Scene(arrays).close()
    drift = before - _free()
    print(f"create + destroy twice: free device memory fell by {drift} B (bound {bound} B)")
    assert drift <= bound, (drift, bound)


# ---------------------------------------------------------------------------------------------- every way in, the same scene
def _small_scenes():
    from rtcuda_amd import scenes
    box = scenes.cornell_bunny("matte", bunny=False)
    no_lights = np.zeros(0, scenes.LIGHT_DTYPE)
    one = scenes.SceneArrays(tris=box.tris[8:9].copy(), tri_material=np.array([2], np.int32), tri_light=np.array([-1], np.int32),
                             materials=box.materials, lights=no_lights)
    empty = scenes.SceneArrays(tris=np.zeros((0, 9), np.float32), tri_material=np.zeros(0, np.int32), tri_light=np.zeros(0, np.int32),
                               materials=box.materials, lights=no_lights)
    return {"box": box, "one": one, "empty": empty}


def _routes(api, arrays, other):
    """name -> scene, by every entry point that puts a tree into a scene; the first one is the host-built twin"""
    t, m, l = _tensors(arrays)
    out = {"create": api.Scene(arrays), "create_device_bvh": api.Scene(arrays, device_bvh=True),
           "from_tensors": api.Scene.from_tensors(t, m, l, arrays.materials, arrays.lights)}
    out["set_triangles"] = api.Scene(other)
    out["set_triangles"].set_triangles(arrays)
    out["set_triangles_tensors"] = api.Scene(other)
    out["set_triangles_tensors"].set_triangles_tensors(t, m, l, arrays.materials, arrays.lights)
    out["rebuild"] = api.Scene(arrays)
    out["rebuild"].rebuild()
    return out


def _frame(api, sc):
    img, st = sc.render(_camera(api, 64 / 48), 64, 48, 4, flags=api.FLAG_DETERMINISTIC)
    return img.tobytes(), {k: st[k] for k in EVENTS}, st


@pytest.mark.parametrize("name", ["box", "one"])
def test_every_way_in_ends_in_the_same_scene(api, name):
    small = _small_scenes()
    arrays, other = small[name], small["one" if name == "box" else "box"]
    routes = _routes(api, arrays, other)
    twin = routes["create"]
    infos = {r: sc.info() for r, sc in routes.items()}
    assert {r: i["builder"] for r, i in infos.items()} == {r: "sah" if r == "create" else "ploc" for r in routes}
    assert {i["tris"] for i in infos.values()} == {len(arrays.tris)}
    built = [tuple(i[k] for k in ("pairs", "max_depth", "leaves")) for r, i in infos.items() if r != "create"]
    assert len(set(built)) == 1, infos
    o, d = _aimed_rays(arrays.tris, 4000, seed=11)
    want = _frame(api, twin)[:2]
    for r, sc in routes.items():
        if sc is twin:
            continue
        _assert_same_hits(api, sc, twin, o, d)
        assert _frame(api, sc)[:2] == want, r


def test_the_empty_scene_through_every_way_in(api):
    small = _small_scenes()
    empty, box = small["empty"], small["box"]
    a, b = api.Scene(empty), api.Scene(empty, device_bvh=True)
    for sc in (a, b):
        bits, _, st = _frame(api, sc)
        assert not np.frombuffer(bits, np.float32).any() and st["shade_events"] == 0 and st["camera_rays"] == 64 * 48 * 4
    ia, ib = a.info(), b.info()
    assert ia["builder"] == "sah" and ib["builder"] == "ploc" and ib["build_seconds"] == 0
    assert ia["tris"] == ib["tris"] == 0
    # the ways in that need triangles refuse it, each with its own words, and leave the scene as it was
    t, m, l = _tensors(empty)
    with pytest.raises(api.RtError, match="at least one triangle"):
        api.Scene.from_tensors(t, m, l, empty.materials, empty.lights)
    with pytest.raises(api.RtError, match="at least one triangle"):
        api.Scene(box).set_triangles(empty)
    with pytest.raises(api.RtError, match="at least one triangle"):
        api.Scene(box).set_triangles_tensors(t, m, l, empty.materials, empty.lights)
    with pytest.raises(api.RtError, match="no triangles"):
        a.rebuild()
    assert a.info() == ia and not np.frombuffer(_frame(api, a)[0], np.float32).any()
    # ... and the empty scene takes a first triangle set like any other
    want = _frame(api, api.Scene(box))[:2]
    for sc in (a, b):
        sc.set_triangles(box)
        assert sc.info()["tris"] == len(box.tris) and sc.info()["builder"] == "ploc"
        assert _frame(api, sc)[:2] == want
