"""Refit of a scene's BVH to new vertex positions (rt_scene_update), checked on the host.  No GPU needed.

rt_host_check.cpp holds a host twin of the device refit (k_refit_level in rt_build_kernels.inc): the builder's 4-wide records with
exact child boxes recomputed from new vertices, padded by 2 ulps on write.  With the vertices of creation it must give the
builder's records bit for bit; with moved vertices the records must pass the builder's structural checks and the 4-wide walk
must find what exhaustive search finds.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, default_camera
import raygen

SAH_SCALE = 1e-6


def _lib():
    from rtcuda_amd import api
    api.build()
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    L.rt_bvh_refit_check.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p]
    return L


def _refit_check(build_tris, new_tris, ro=None, rd=None):
    b = np.ascontiguousarray(build_tris, np.float32).reshape(-1, 9)
    t = np.ascontiguousarray(new_tris, np.float32).reshape(-1, 9)
    assert b.shape == t.shape
    ro = np.zeros((0, 3), np.float32) if ro is None else np.ascontiguousarray(ro, np.float32)
    rd = np.zeros((0, 3), np.float32) if rd is None else np.ascontiguousarray(rd, np.float32)
    out = np.zeros(6, np.int64)
    rc = _lib().rt_bvh_refit_check(b.ctypes.data, t.ctypes.data, b.shape[0], ro.shape[0], ro.ctypes.data if len(ro) else None,
                                   rd.ctypes.data if len(rd) else None, out.ctypes.data)
    assert rc == 0
    return dict(zip(["records", "differ", "errors", "mismatch", "rays", "sah"], out.tolist()))


def deform(tris, amp=0.01):
    """A smooth per-vertex displacement: a function of the position alone, so shared vertices stay shared."""
    v = np.asarray(tris, np.float64).reshape(-1, 3)
    d = amp * np.stack([np.sin(7.0 * v[:, 1] + 1.0), np.sin(5.0 * v[:, 2] + 2.0), np.sin(6.0 * v[:, 0] + 3.0)], axis=1)
    return (v + d).astype(np.float32).reshape(-1, 9)


def _rays(oracle, ro_shift=(0.0, 0.0, 0.0), scale=1.0, n_cam=1500, n_axis=300):
    """Camera rays of the default view and slab-test edge cases, moved with the scene (o -> scale * o + shift)."""
    cam = default_camera(oracle, 16 / 9)
    o1, d1 = raygen.camera_rays(cam, 1920, 1080, n_cam, seed=11)
    o2, d2 = raygen.axis_aligned_rays(n_axis, seed=12)
    o = np.concatenate([o1, o2]).astype(np.float64) * scale + np.asarray(ro_shift)
    return o.astype(np.float32), np.concatenate([d1, d2])


@pytest.mark.parametrize("variant", ["matte", "four_bunnies"])
def test_refit_with_the_build_vertices_gives_the_builders_records(variant):
    from rtcuda_amd import scenes
    tris = scenes.cornell_bunny(variant).tris
    r = _refit_check(tris, tris)
    assert r["records"] > 1000 and r["errors"] == 0
    assert r["differ"] == 0, f"{r['differ']} of {r['records']} refit records differ from the builder's"


@pytest.mark.parametrize("case", ["deform", "scale10", "translate100"])
def test_refit_after_moving_the_vertices_is_valid_and_walks_like_exhaustive_search(oracle, bunny_matte, case):
    tris = np.asarray(bunny_matte.tris, np.float32).reshape(-1, 9)
    if case == "deform":
        new, (ro, rd) = deform(tris), _rays(oracle)
    elif case == "scale10":
        new, (ro, rd) = (tris * np.float32(10.0)).astype(np.float32), _rays(oracle, scale=10.0)
    else:
        shift = np.array([100.0, 0.0, 0.0] * 3, np.float32)
        new, (ro, rd) = (tris + shift).astype(np.float32), _rays(oracle, ro_shift=(100.0, 0.0, 0.0))
    r = _refit_check(tris, new, ro, rd)
    assert r["errors"] == 0
    assert r["rays"] == len(ro) and r["mismatch"] == 0
    assert r["differ"] > 0  # (the boxes did move)
    base = _refit_check(tris, tris)["sah"]
    ratio = r["sah"] / base
    if case == "deform":
        assert 0.9 < ratio < 1.2  # a mild deformation keeps the tree's quality
    else:
        assert abs(ratio - 1.0) < 0.01  # a scale or a translation changes no relative area (up to rounding)


def test_refit_of_a_scrambled_scene_stays_correct(oracle, bunny_matte):
    """Vertices moved far from where the tree was built for (triangles swapped among each other): the tree is poor, but the
    refit boxes still contain their triangles and the walk still finds every closest hit."""
    tris = np.asarray(bunny_matte.tris, np.float32).reshape(-1, 9)[::8]
    rng = np.random.default_rng(3)
    new = tris[rng.permutation(len(tris))]
    ro, rd = _rays(oracle, n_cam=800, n_axis=200)
    r = _refit_check(tris, new, ro, rd)
    assert r["errors"] == 0 and r["mismatch"] == 0
    assert r["sah"] > 2 * _refit_check(tris, tris)["sah"]


def test_cpp_update_compiles_against_the_host_header(tmp_path):
    """rtcuda::update's signature as a driver would call it (include/rtcuda/rtcuda.hpp)."""
    src = tmp_path / "caller.cpp"
    src.write_text(
        '#include "rtcuda/rtcuda.hpp"\n'
        "void f(Scene &scene, const std::vector<Triangle> &tris) { update(scene, tris); }\n"
        "int g(rt_scene *s, const float *v, int n) {\n"
        "    int64_t refits; double sec, ratio;\n"
        "    return rt_scene_update(s, v, n) | rt_scene_update_device(s, v, n, 0) | rt_scene_refit_info(s, &refits, &sec, &ratio);\n"
        "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])
