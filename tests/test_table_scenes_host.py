"""Large shading tables without a GPU: the recipe of tests/table_scenes.py, the premise of its padding test, and the C-ABI's
limits on the material and light counts.  (tests/test_gpu_large_tables.py renders these scenes on the device.)"""
import ctypes

import numpy as np
import pytest

import raygen
import table_scenes as ts
from conftest import default_camera, usable_cpus

SIZES = [(64, 64), (65, 8), (8, 65), (300, 300), (8, 100), (ts.MAX_MATS, ts.MAX_LIGHTS)]


@pytest.mark.parametrize("n_mats,n_lights", SIZES)
def test_table_scene_recipe_is_consistent(n_mats, n_lights):
    a = ts.table_scene(n_mats, n_lights)
    n_bunny = a.meta["n_bunny"]
    assert len(a.materials) == n_mats and len(a.lights) == n_lights
    assert a.tri_material.dtype == np.int32 and a.tri_light.dtype == np.int32
    # every material index is referenced; the highest ones sit on the walls, one per wall triangle, highest first
    assert np.array_equal(np.unique(a.tri_material), np.arange(n_mats))
    for k, w in enumerate(ts.TOP_WALLS):
        assert a.tri_material[n_bunny + w] == n_mats - 1 - k
    # neighbouring materials differ (a table row one off shows)
    alb = a.materials["albedo"]
    assert (np.abs(alb[1:] - alb[:-1]).max(axis=1) > 1e-3).all()
    assert (a.materials["type"] != a.materials["type"][0]).any()
    glass = a.materials["type"] == 2
    assert glass.any() and len(np.unique(a.materials["ior"][glass])) > 0.9 * glass.sum()  # (varied IOR)
    # tri_light and lights[k].tri are inverse maps on the area lights; point lights own no triangle
    area = np.flatnonzero(a.lights["type"] == 1)
    assert len(area) == ts.n_area_lights(n_lights)
    assert np.array_equal(a.tri_light[a.lights["tri"][area]], area)
    lit = np.flatnonzero(a.tri_light >= 0)
    assert len(lit) == len(area) and np.array_equal(a.lights["tri"][a.tri_light[lit]], lit)
    assert (a.lights["tri"][a.lights["type"] == 0] == -1).all()
    # light indices are not in triangle order, and the highest are area lights
    assert not np.array_equal(a.tri_light[lit], np.sort(a.tri_light[lit]))
    assert a.lights["type"][n_lights - 1] == 1 and a.lights["type"][n_lights - 2] == 1
    # neighbouring lights differ in radiance
    rad = a.lights["L"]
    assert (np.abs(rad[1:] - rad[:-1]).max(axis=1) > 0).all()
    # the table sizes: which side of the LDS gate, and how large
    assert ts.tab_dwords(n_mats, n_lights) == 5 * n_mats + 24 * n_lights
    assert ts.lds_tables(n_mats, n_lights) == (n_mats <= 64 and n_lights <= 64)


def test_lds_boundary_scene_fills_the_lds_table_exactly():
    assert ts.lds_tables(64, 64) and not ts.lds_tables(65, 8) and not ts.lds_tables(8, 65)
    assert ts.tab_dwords(64, 64) == 64 * 29 == 1856  # kTabDwordsMax in rtcuda_amd.hip


@pytest.mark.parametrize("n_mats,n_lights", [(64, 64), (65, 8), (ts.MAX_MATS, ts.MAX_LIGHTS)])
def test_the_camera_sees_the_highest_indices(oracle, n_mats, n_lights):
    """The top material indices and the top light indices are what the camera's rays hit first: a packed id or a table
    offset that is wrong for them changes pixels."""
    a = ts.table_scene(n_mats, n_lights)
    osc = oracle.scene(a)
    o, d = raygen.camera_rays(default_camera(oracle, 1.0), 64, 64, 200_000, seed=3)
    tri, _, _, _ = osc.trace_closest(o, d, np.full(len(o), np.float32(3.4e38), np.float32), threads=usable_cpus())
    hit = tri[tri >= 0]
    seen_mats = np.bincount(a.tri_material[hit], minlength=n_mats)
    assert (seen_mats[n_mats - 6:] > 1000).all(), seen_mats[n_mats - 6:]
    seen_lights = np.bincount(a.tri_light[hit][a.tri_light[hit] >= 0], minlength=n_lights)
    top = np.arange(n_lights - min(4, a.meta["n_area"] // 2), n_lights)  # (the top half of the area lights' indices)
    assert (seen_lights[top] > 10).all(), seen_lights[top]


@pytest.mark.parametrize("pad", [65, ts.MAX_MATS])
def test_padding_with_unused_materials_changes_nothing_in_the_oracle(oracle, bunny_full_bsdf, pad):
    """The premise of the GPU's LDS-vs-global padding test: nothing in the estimator reads the material count."""
    w, h, spp = 64, 48, 8
    cam = default_camera(oracle, w / h)
    sums = []
    for arrays in (bunny_full_bsdf, ts.padded(bunny_full_bsdf, pad)):
        fixed = np.zeros((h, w, 3), np.int64)
        _, _, st = oracle.scene(arrays).render(cam, w, h, spp, threads=usable_cpus(), fixed_out=fixed)
        st.pop("seconds_loop"), st.pop("seconds_rng_init")
        sums.append((fixed, st))
    (fa, sa), (fb, sb) = sums
    assert len(ts.padded(bunny_full_bsdf, pad).materials) == pad
    assert fa.any() and np.array_equal(fa, fb)
    it_a, it_b = sa.pop("iter_counts"), sb.pop("iter_counts")
    assert sa == sb and np.array_equal(it_a, it_b)


def test_padded_materials_are_distinct_and_implausible(bunny_full_bsdf):
    p = ts.padded(bunny_full_bsdf, 300)
    assert np.array_equal(p.materials[:6], bunny_full_bsdf.materials)
    extra = p.materials[6:]
    assert (extra["albedo"] > 1).all() and (extra["ior"] == 9).all() and set(extra["type"]) == {0, 1, 2}
    assert len(np.unique(extra["albedo"], axis=0)) == len(extra)
    assert p.tri_material is bunny_full_bsdf.tri_material and p.lights is bunny_full_bsdf.lights


def _create(arrays, n_mats=None, n_lights=None):
    """rt_scene_create on raw arrays -> (return code, rt_last_error()).  These are refused before any device call."""
    from rtcuda_amd import api
    L = api.lib()
    tris = np.ascontiguousarray(arrays.tris, np.float32)
    tm = np.ascontiguousarray(arrays.tri_material, np.int32)
    tl = np.ascontiguousarray(arrays.tri_light, np.int32)
    mats = np.ascontiguousarray(arrays.materials)
    lights = np.ascontiguousarray(arrays.lights)
    h = ctypes.c_void_p()
    rc = L.rt_scene_create(tris.ctypes.data, tris.shape[0], tm.ctypes.data, tl.ctypes.data, mats.ctypes.data,
                           len(mats) if n_mats is None else n_mats, lights.ctypes.data,
                           len(lights) if n_lights is None else n_lights, ctypes.byref(h))
    if rc == 0:
        L.rt_scene_destroy(h)
    return rc, L.rt_last_error().decode()


def test_scene_create_refuses_counts_past_the_packed_id_limits(bunny_full_bsdf):
    import dataclasses
    too_many_mats = ts.padded(bunny_full_bsdf, ts.MAX_MATS + 1)
    rc, err = _create(too_many_mats)
    assert rc != 0 and "at most 65535 materials and 32766 lights" in err, err
    # light 32766 would pack to 32767 << 16: still positive, but the C-ABI keeps one value in reserve
    big = ts.table_scene(8, ts.MAX_LIGHTS)
    extra = np.zeros(1, dtype=big.lights.dtype)
    extra[0] = (0, (0.5, 0.5, -0.5), -1, (0.1, 0.1, 0.1))
    rc, err = _create(dataclasses.replace(big, lights=np.concatenate([big.lights, extra])))
    assert rc != 0 and "at most 65535 materials and 32766 lights" in err, err


def test_scene_create_refuses_an_index_one_past_the_tables(bunny_full_bsdf):
    import dataclasses
    a = ts.table_scene(65, 8)
    tm = a.tri_material.copy()
    tm[a.meta["n_bunny"]] = 65  # == n_mats
    rc, err = _create(dataclasses.replace(a, tri_material=tm))
    assert rc != 0 and f"tri_material[{a.meta['n_bunny']}] out of range" in err, err
    rc, err = _create(a, n_mats=64)  # the same arrays, one material fewer declared: material 64 is out of range
    assert rc != 0 and "out of range" in err, err
    tl = a.tri_light.copy()
    tl[np.flatnonzero(tl >= 0)[0]] = 8  # == n_lights
    rc, err = _create(dataclasses.replace(a, tri_light=tl))
    assert rc != 0 and "tri_light[" in err and "out of range" in err, err
