"""The device BVH builder (PLOC: rt_scene_rebuild, RT_SCENE_DEVICE_BVH) checked on the host through its twin.  No GPU needed.

rt_host_check.cpp holds a sequential restatement of the device build (k_ploc_* in rt_build_kernels.inc) with the same fp32
expressions (rt_ploc.h): the GPU tests (test_gpu_scene_rebuild.py) show that the device gives the twin's records and leaf
order bit for bit, and this file shows that those make a valid tree -- every triangle in exactly one leaf, every box
containing what lies beneath it, the 4-wide walk finding what exhaustive search finds -- of surface-area quality close to
the host SAH builder's.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, default_camera
import raygen
from test_scene_update_host import deform

SAH_BAR = 1.25  # the twin's 4-wide surface-area cost at most this times the host builder's (with its reinsertion pass)


def _lib():
    from rtcuda_amd import api
    api.build()
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    L.rt_ploc_check.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                ctypes.c_void_p]
    L.rt_ploc_build.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    return L


def _check(tris, ro=None, rd=None, with_host=False):
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    ro = np.zeros((0, 3), np.float32) if ro is None else np.ascontiguousarray(ro, np.float32)
    rd = np.zeros((0, 3), np.float32) if rd is None else np.ascontiguousarray(rd, np.float32)
    out = np.zeros(8, np.int64)
    rc = _lib().rt_ploc_check(t.ctypes.data, t.shape[0], ro.shape[0], ro.ctypes.data if len(ro) else None,
                              rd.ctypes.data if len(rd) else None, int(with_host), out.ctypes.data)
    assert rc == 0
    return dict(zip(["records", "errors", "mismatch", "rays", "sah", "sah_host", "iterations", "max_leaf"], out.tolist()))


def _build(tris):
    L = _lib()
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    out = np.zeros(4, np.int64)
    assert L.rt_ploc_build(t.ctypes.data, t.shape[0], None, 0, None, out.ctypes.data) == 0
    recs = np.zeros((int(out[0]), 16), np.uint32)
    order = np.zeros(t.shape[0], np.int32)
    assert L.rt_ploc_build(t.ctypes.data, t.shape[0], recs.ctypes.data, len(recs), order.ctypes.data, out.ctypes.data) == 0
    return recs, order, dict(zip(["records", "iterations", "depth", "leaves"], out.tolist()))


def _rays(oracle, tris, n_cam=1500, n_axis=300, n_bounce=1500):
    """Camera rays of the default view, slab-test edge cases, and bounce-like rays from random points on the triangles."""
    cam = default_camera(oracle, 16 / 9)
    o1, d1 = raygen.camera_rays(cam, 1920, 1080, n_cam, seed=11)
    o2, d2 = raygen.axis_aligned_rays(n_axis, seed=12)
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    rng = np.random.default_rng(13)
    pick = rng.integers(0, len(t), n_bounce)
    w = rng.dirichlet((1.0, 1.0, 1.0), n_bounce)
    o3 = np.einsum("nk,nka->na", w, t[pick])  # (points on triangles, as bounce origins are)
    d3 = rng.normal(size=(n_bounce, 3))
    d3 /= np.linalg.norm(d3, axis=1, keepdims=True)
    return (np.concatenate([o1, o2, o3.astype(np.float32)]).astype(np.float32),
            np.concatenate([d1, d2, d3.astype(np.float32)]).astype(np.float32))


@pytest.mark.parametrize("variant", ["matte", "four_bunnies", "sixteen_lights"])
def test_twin_tree_is_valid_and_walks_like_exhaustive_search(oracle, variant):
    from rtcuda_amd import scenes
    tris = scenes.cornell_bunny(variant).tris
    ro, rd = _rays(oracle, tris, n_cam=800 if variant == "four_bunnies" else 1500)
    r = _check(tris, ro, rd)
    assert r["records"] > 1000 and r["errors"] == 0
    assert r["rays"] == len(ro) and r["mismatch"] == 0
    assert 1 <= r["max_leaf"] <= 4


@pytest.mark.parametrize("variant", ["matte", "four_bunnies"])
def test_twin_sah_is_close_to_the_host_builders(variant):
    from rtcuda_amd import scenes
    r = _check(scenes.cornell_bunny(variant).tris, with_host=True)
    ratio = r["sah"] / r["sah_host"]
    print(f"{variant}: PLOC SAH {r['sah'] * 1e-6:.4f}, host SAH {r['sah_host'] * 1e-6:.4f}, ratio {ratio:.4f}, "
          f"{r['iterations']} iterations")
    assert ratio <= SAH_BAR, ratio


def test_twin_builds_are_deterministic_and_leaves_are_small(bunny_matte):
    recs, order, info = _build(bunny_matte.tris)
    recs2, order2, info2 = _build(bunny_matte.tris)
    assert recs.tobytes() == recs2.tobytes() and order.tobytes() == order2.tobytes() and info == info2
    assert np.array_equal(np.sort(order), np.arange(bunny_matte.n_tris))
    links = recs[:, 12:14].view(np.int32).ravel()
    leaves = links[(links < 0) & (links != np.int32(-2 ** 31))]
    counts = (~leaves) & 7
    assert counts.min() >= 1 and counts.max() <= 4 and counts.sum() == bunny_matte.n_tris
    assert info["leaves"] == len(leaves)
    inner = links[links >= 0]
    assert np.all(inner % 2 == 0) and len(np.unique(inner)) == len(inner) == len(recs) // 2 - 1
    # breadth first: a child's record comes after its parent's, and the children of a node come in the order of the nodes
    child_of = [(j // 2, l // 2) for j, l in zip(np.repeat(np.arange(len(recs)), 2), links) if l >= 0]
    assert all(c > p for p, c in child_of)
    assert [c for _, c in child_of] == list(range(1, len(recs) // 2))
    print(f"bunny: {info['iterations']} iterations, 4-wide depth {info['depth']}, {info['leaves']} leaves")


def _small(bunny_matte, n):
    return np.asarray(bunny_matte.tris, np.float32).reshape(-1, 9)[::997][:n]


@pytest.mark.parametrize("case", ["1", "2", "3", "5", "8", "9", "coincident", "bare_box", "deformed_bunny"])
def test_degenerate_and_tiny_inputs(oracle, bunny_matte, case):
    from rtcuda_amd import scenes
    if case.isdigit():
        tris = _small(bunny_matte, int(case))
    elif case == "coincident":  # (equal Morton codes: the index bits alone order them)
        tris = np.repeat(np.asarray(bunny_matte.tris, np.float32).reshape(-1, 9)[100:101], 40, axis=0)
    elif case == "bare_box":
        tris = scenes.cornell_bunny("matte", bunny=False).tris
    else:
        tris = deform(bunny_matte.tris, amp=0.05)
    ro, rd = _rays(oracle, tris, n_cam=600, n_axis=100, n_bounce=600)
    r = _check(tris, ro, rd)
    assert r["errors"] == 0 and r["mismatch"] == 0 and r["rays"] == len(ro)
    recs, order, info = _build(tris)
    assert np.array_equal(np.sort(order), np.arange(len(tris)))
    assert recs.tobytes() == _build(tris)[0].tobytes()
    if case == "1":
        assert info["records"] == 2 and info["leaves"] == 1


def test_cpp_rebuild_compiles_against_the_host_header(tmp_path):
    """rtcuda::rebuild's signature as a driver would call it (include/rtcuda/rtcuda.hpp), and the new C-ABI entry points."""
    src = tmp_path / "caller.cpp"
    src.write_text(
        '#include "rtcuda/rtcuda.hpp"\n'
        "void f(Scene &scene, const std::vector<Triangle> &tris) { rebuild(scene, tris); }\n"
        "int g(rt_scene *s, const float *v, int n, rt_scene **out) {\n"
        "    return rt_scene_rebuild(s, v, n) | rt_scene_rebuild(s, nullptr, n) | rt_scene_rebuild_device(s, v, n, 0) |\n"
        "           rt_scene_create_flags(v, n, nullptr, nullptr, nullptr, 0, nullptr, 0, RT_SCENE_DEVICE_BVH, out);\n"
        "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])
