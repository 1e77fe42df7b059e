"""Writes tests/golden/tree_hashes.json: a 64-bit hash of the 4-wide records (`quads`) and of the leaf order of the trees the
project measures, from the host SAH builder (rt_bvh_export) and from the PLOC twin (rt_ploc_build) of librt_hostcheck.so.

    python tests/golden/make_tree_hashes.py [path/to/librt_hostcheck.so]

The committed file was made with the library of the commit BEFORE the builders learned to cut runs of equal boxes (that
commit's rt_bvh.h, rt_ploc.h and twin, plus the rt_bvh_export entry point, which only copies a result out).  To make it
again: take rtcuda_amd/csrc/{rt_bvh.h, rt_ploc.h, rt_ref_tree.h, rt_host_check.cpp} of commit cba1a8f ("Pin the per-sample RNG
mode to an exact CPU oracle, bit for bit") into a directory of their own, paste today's rt_bvh_export into that
rt_host_check.cpp, build it with the Makefile's line for librt_hostcheck.so and give the path of the result to this script.
tests/test_placed_scenes_host.py asserts that the builders of today still give every one of these trees, bit for bit.
Regenerate it only for a change that is MEANT to move the trees.
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

BUILDERS = ("rt_bvh_export", "rt_ploc_build")


def load(path=None):
    L = ctypes.CDLL(path or os.path.join(ROOT, "rtcuda_amd", "librt_hostcheck.so"))
    for name in BUILDERS:
        getattr(L, name).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    return L


def tree(L, builder, tris):
    """(records as (n, 16) uint32, leaf order, out4) of one builder, or None if it refuses the triangles."""
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    fn = getattr(L, builder)
    out = np.zeros(4, np.int64)
    if fn(t.ctypes.data, t.shape[0], None, 0, None, out.ctypes.data) != 0:
        return None
    recs = np.zeros((int(out[0]), 16), np.uint32)
    order = np.zeros(t.shape[0], np.int32)
    assert fn(t.ctypes.data, t.shape[0], recs.ctypes.data, len(recs), order.ctypes.data, out.ctypes.data) == 0
    return recs, order, out.tolist()


def h64(a):
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=8).hexdigest()


def measured_scenes():
    """name -> triangles: the four benchmark scenes, the table scene and the nine tiny / degenerate cases."""
    from rtcuda_amd import scenes
    from table_scenes import table_scene
    from test_gpu_scene_rebuild import TINY_CASES, _tiny_case
    out = {v: scenes.cornell_bunny(v).tris for v in ("matte", "full_bsdf", "four_bunnies", "sixteen_lights")}
    out["table_65_65_1"] = table_scene(65, 65, seed=1).tris
    matte = scenes.cornell_bunny("matte")
    for case in TINY_CASES:
        out["tiny_" + case] = _tiny_case(matte, case).tris
    return out


def hashes(L):
    out = {}
    for name, tris in measured_scenes().items():
        for builder in BUILDERS:
            built = tree(L, builder, tris)
            assert built is not None, f"{builder} refuses the scene {name!r}"
            recs, order, info = built
            out[f"{name}/{builder}"] = {"quads": h64(recs), "order": h64(order), "records": len(recs)}
    return out


if __name__ == "__main__":
    result = hashes(load(sys.argv[1] if len(sys.argv) > 1 else None))
    with open(os.path.join(HERE, "tree_hashes.json"), "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(result)} trees hashed")
