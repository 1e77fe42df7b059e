"""Far-off and duplicated geometry on the CPU (tests/placed_scenes.py): the builders accept it, and the walks keep their answers.

Until this file every scene of the suite sat in [0, 1]^3.  Two things depend on where the geometry sits and how often it repeats:

  * the builders' handling of EQUAL boxes.  The SAH sweep (rt_bvh.h) peeled one triangle per level off a run of equal boxes
    and hit its depth cap (`ok = false`: the scene was refused), and its reinsertion pass strung such runs into chains; the
    PLOC builder (rt_ploc.h, its twin in rt_host_check.cpp) merged one pair per iteration.  fp32 makes such runs out of any
    mesh far from the origin: at 1e5 half of the bunny's triangles are duplicates, many of them points.
  * the default kernels' rare path -- ref_visible, then the literal re-trace through the reference's tree -- which a scene at
    1e4 takes about 10^4 times as often as the scenes in [0, 1]^3 (42 of 20 000 camera rays), here on the CPU twin
    (rt_hostwalk_trace_verified); tests/test_gpu_placed_scenes.py drives the kernels with the same batches.

The bar is the project's usual one: equal bits against the oracle, every ray, nothing excluded, no tolerance.
"""
import json
import os
import re

import numpy as np
import pytest

import placed_scenes
from conftest import ROOT, default_camera
from test_host_logic import _hostcheck, _selfcheck
from test_traversal_audit import HostWalk

FLT_MAX = placed_scenes.FLT_MAX
BUNNY_ITERATIONS = 47  # what the PLOC twin needs for the bunny scene (test_scene_rebuild_host.py prints it) ...
MAX_ITERATIONS = 4 * BUNNY_ITERATIONS  # ... and the bar for a run of equal boxes, which needed one iteration per box

DUPLICATED = ["shift_1e5"] + [f"{kind}_{n}" for kind in ("points", "copies") for n in (8, 70, 200, 1000, 5000)]
HIT_CASES = list(placed_scenes.PLACES) + DUPLICATED[1:]


def _max_stack_bound():
    """kMaxStackBound as the product's source states it (the deepest traversal stack a scene may need)."""
    path = os.path.join(ROOT, "rtcuda_amd", "csrc", "rtcuda_amd.hip")
    with open(path) as fh:
        m = re.search(r"constexpr\s+int\s+kMaxStackBound\s*=\s*(\d+)\s*;", fh.read())
    assert m, f"kMaxStackBound is no longer declared as 'constexpr int kMaxStackBound = N;' in {path}: follow it here"
    return int(m.group(1))


_scene_cache = {}


def _scene(name):
    if name not in _scene_cache:
        _scene_cache.clear()  # (one bunny-sized scene at a time)
        _scene_cache[name] = placed_scenes.scene(name)
    return _scene_cache[name]


# ---------------------------------------------------------------------------------------------- 1, 2: the builders
@pytest.mark.parametrize("name", DUPLICATED)
def test_host_builder_accepts_runs_of_equal_boxes(name):
    arrays = _scene(name)[0]
    HostWalk(arrays)  # (rt_hostwalk_create: asserts a handle)
    r = _selfcheck(_hostcheck(), arrays.tris, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    print(f"{name}: host SAH tree of {r['nodes']} nodes, depth {r['depth']}, stack bound {r['stack_bound']}, largest leaf {r['maxleaf']}")
    assert r["errors"] == 0 and 1 <= r["maxleaf"] <= 7
    assert r["stack_bound"] <= _max_stack_bound()


@pytest.mark.parametrize("name", DUPLICATED)
def test_ploc_twin_accepts_runs_of_equal_boxes(name):
    from test_scene_rebuild_host import _build, _check
    arrays = _scene(name)[0]
    recs, order, info = _build(arrays.tris)  # (asserts rt_ploc_build == 0)
    print(f"{name}: PLOC twin, {info['iterations']} iterations, 4-wide depth {info['depth']}")
    assert np.array_equal(np.sort(order), np.arange(arrays.n_tris))
    assert 3 * info["depth"] + 1 <= _max_stack_bound()
    assert info["iterations"] <= MAX_ITERATIONS
    r = _check(arrays.tris)
    assert r["errors"] == 0 and 1 <= r["max_leaf"] <= 7


# ---------------------------------------------------------------------------------------------- 3: hits
def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", HIT_CASES)
def test_walks_keep_their_answers(oracle, name):
    """Camera rays and bounce rays, 20 000 each.  The product's walk = exhaustive search (hit or miss, t bit for bit) = the
    watertight oracle (the triangle too); the verified walk = the literal oracle (triangle, t, occlusion flag), every ray."""
    arrays, s3, t3 = _scene(name)
    sc = oracle.scene(arrays)
    walk = HostWalk(arrays)
    o, d = placed_scenes.camera_batch(default_camera(oracle, 16 / 9), s3, t3)
    tmax = np.full(len(o), FLT_MAX, np.float32)
    first = sc.trace_closest_brute(o, d, tmax)
    assert 0.2 < (first[0] >= 0).mean() <= 1.0
    o2, d2 = placed_scenes.bounce_batch(o, d, first[1], first[0] >= 0)
    assert len(o2) == len(o) == 20_000
    batches = [("camera", (o, d)), ("bounce", (o2, d2))]
    if name not in placed_scenes.PLACES:  # (the extra triangles come first)
        batches.append(("aimed", placed_scenes.aimed_batch(arrays.tris[:int(name.split("_")[1])])))
    for what, (ro, rd) in batches:
        brute = sc.trace_closest_brute(ro, rd, tmax)
        lit = sc.trace_closest(ro, rd, tmax)
        wt = sc.set_watertight(True).trace_closest(ro, rd, tmax)
        sc.set_watertight(False)
        tri, t = walk.closest(ro, rd)
        hit = brute[0] >= 0
        assert np.array_equal(tri >= 0, hit), what
        assert np.array_equal(_bits(t[hit]), _bits(brute[1][hit])), what
        assert np.array_equal(tri, wt[0]) and np.array_equal(_bits(t[hit]), _bits(wt[1][hit])), what
        vtri, vt, st = walk.closest_verified(ro, rd)
        lhit = lit[0] >= 0
        assert np.array_equal(vtri, lit[0]), what
        assert np.array_equal(_bits(vt[lhit]), _bits(lit[1][lhit])), what
        # (a ray is re-traced once, be its hit lost, tied or -- among the duplicates of shift_1e5 -- both)
        assert max(st["lost_hits"], st["ties"]) <= st["literal_retraces"] <= st["lost_hits"] + st["ties"], (what, st)
        if name in ("shift_1e4", "shift_x_-1e4"):
            assert st["literal_retraces"] == st["lost_hits"] + st["ties"], (what, st)
        print(f"{name} {what}: {st}, literal != watertight on {int((lit[0] != wt[0]).sum())} rays")
        if what == "aimed" and name.startswith("copies"):
            assert st["ties"] >= 0.9 * len(ro), st  # (every hit on the copies is an exact tie: the literal walk decides)
        if what == "camera" and name in ("shift_1e4", "shift_x_-1e4"):
            assert st["lost_hits"] >= 10, st  # (42 measured: the batch really takes the rare path)
        # any hit: the verified walk against the literal oracle's occlusion flag
        o3, d3, tm3, excl = placed_scenes.any_batch(sc, arrays, ro, rd, seed=22, tmax_scale=min(s3))
        occ, st_a = walk.any_verified(o3, d3, tm3, excl)
        want = sc.trace_any(o3, d3, tm3, excl)
        assert np.array_equal(occ, want), what
        assert st_a["literal_retraces"] == st_a["lost_hits"], (what, st_a)
        print(f"{name} {what}: {len(o3)} shadow rays, {want.mean():.3f} occluded, {st_a}")
        if name in ("shift_1e4", "shift_x_-1e4"):  # (the geometry of test_gpu_query.py's batches, moved)
            assert 0.05 < want.mean() < 0.95, what


# ---------------------------------------------------------------------------------------------- 4: the trees of yesterday
def test_measured_scenes_keep_their_trees():
    """Tripwire for the builders' handling of equal boxes: the host SAH tree and the PLOC twin's tree of every scene the
    project measures are, bit for bit, what they were before it changed (tests/golden/make_tree_hashes.py)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_tree_hashes
    finally:
        sys.path.pop(0)
    with open(os.path.join(ROOT, "tests", "golden", "tree_hashes.json")) as fh:
        want = json.load(fh)
    _hostcheck()  # (builds the library)
    got = make_tree_hashes.hashes(make_tree_hashes.load())
    assert len(want) == 2 * (5 + 9) and set(got) == set(want)
    moved = [k for k in sorted(want) if got[k] != want[k]]
    assert not moved, moved
