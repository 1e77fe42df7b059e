"""Rays through vertices, edges and along the axes (tests/ray_families.py) on the CPU: the product's walk, its verified form and
the oracle's watertight walk against exhaustive search and the literal oracle.  No GPU.

Random rays almost never pass exactly through a vertex, an edge, a box face or a box corner; these do, 20 000 per family, on the
bunny in the box and on four of them.  What must hold, with no tolerance:
  * the twin's plain walk (rt_hostwalk_trace: the walk of RT_FLAG_WATERTIGHT) = exhaustive search over all triangles
    (trace_closest_brute / trace_any_brute), every bit of the triangle and of t; ties go to the larger caller index on both sides;
  * the twin's verified walk (the default kernels' procedure) = the literal oracle;
  * the oracle's own set_watertight(True) walk = its own exhaustive search.
Before the cull used 1 / d of the true direction and a distance limit widened for edge-on triangles (rt_bvh.h: kCullDirFloor,
kCullTmaxWiden; profiles/ray_families.md), the first failed on 3 095 of the 20 000 rays down the z axis through vertices, on
every ray with a direction of length 2^-24, and on the two pinned rays; the third failed with it.
The conditions at the end keep a family from passing empty-handed: ties, hits the reference loses and the hit rate, from the
twin's own counters.
"""
import numpy as np
import pytest

from conftest import usable_cpus
import ray_families as rf
from test_traversal_audit import HostWalk

N = 20_000
VARIANTS = ("full_bsdf", "four_bunnies")
FAMILIES = tuple(rf.closest_families(np.zeros((1, 3, 3), np.float32), 1))
SCALED_OF = ("vertex_aimed-fixed",)

_cache = {}


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _scene(oracle, variant):
    """(arrays, literal oracle scene, watertight oracle scene, twin, families) of a variant, made once per session."""
    key = ("scene", variant)
    if key not in _cache:
        from rtcuda_amd import scenes
        arrays = scenes.cornell_bunny(variant)
        fams = rf.closest_families(arrays.tris, N)
        fams["pinned"] = rf.pinned_rays()
        for base in SCALED_OF:
            for s in rf.SCALES:
                fams[f"{base}-x2^{int(np.log2(s))}"] = (fams[base][0], rf.scaled(fams[base][1], s))
        _cache[key] = arrays, oracle.scene(arrays), oracle.scene(arrays).set_watertight(True), HostWalk(arrays), fams
    return _cache[key]


def answers(oracle, variant, family):
    """The oracle's three closest-hit answers for a family, each (tri, t, u, v), computed once per session and left unchanged:
    exhaustive search, the literal walk, the watertight walk."""
    key = ("closest", variant, family)
    if key not in _cache:
        _, lit, wt, _, fams = _scene(oracle, variant)
        o, d = fams[family]
        tm = np.full(len(o), rf.FLT_MAX, np.float32)
        th = usable_cpus()
        _cache[key] = {"o": o, "d": d, "brute": lit.trace_closest_brute(o, d, tm, threads=th),
                       "literal": lit.trace_closest(o, d, tm, threads=th), "watertight": wt.trace_closest(o, d, tm, threads=th)}
    return _cache[key]


def any_answers(oracle, variant, exclude):
    """ends_on_vertex for a variant: the rays and the oracle's occlusion flags (exhaustive search, literal, watertight)."""
    key = ("any", variant, exclude)
    if key not in _cache:
        arrays, lit, wt, _, _ = _scene(oracle, variant)
        o, d, tmax, excl = rf.ends_on_vertex(arrays.tris, N, 200 + (exclude == "owner"), exclude)
        th = usable_cpus()
        _cache[key] = {"o": o, "d": d, "tmax": tmax, "excluded": excl,
                       "brute": (lit.trace_any_brute(o, d, tmax, excl, threads=th) >= 0).astype(np.int32),
                       "literal": lit.trace_any(o, d, tmax, excl, threads=th), "watertight": wt.trace_any(o, d, tmax, excl, threads=th)}
    return _cache[key]


def _mismatches(tri, t, want):
    hit = want[0] >= 0
    return int(((tri != want[0]) | (hit & (_bits(t) != _bits(want[1])))).sum())


def _all_families(variant):
    fams = list(FAMILIES) + [f"{b}-x2^{int(np.log2(s))}" for b in SCALED_OF for s in rf.SCALES]
    return fams + (["pinned"] if variant == "full_bsdf" else [])  # (the pinned rays are rays of that scene)


CASES = [(v, f) for v in VARIANTS for f in _all_families(v)]


@pytest.mark.parametrize("variant,family", CASES)
def test_walks_against_exhaustive_search_and_the_literal_oracle(oracle, variant, family):
    a = answers(oracle, variant, family)
    walk = _scene(oracle, variant)[3]
    tri, t = walk.closest(a["o"], a["d"])
    vtri, vt, st = walk.closest_verified(a["o"], a["d"])
    got = {"product walk != exhaustive search": _mismatches(tri, t, a["brute"]),
           "verified walk != literal oracle": _mismatches(vtri, vt, a["literal"]),
           "oracle's watertight walk != its exhaustive search": _mismatches(a["watertight"][0], a["watertight"][1], a["brute"])}
    print(variant, family, got, st)
    assert got == dict.fromkeys(got, 0)
    # u and v of the watertight walk are the triangle test's on the same triangle: equal to exhaustive search's too
    hit = a["brute"][0] >= 0
    assert np.array_equal(_bits(a["watertight"][2][hit]), _bits(a["brute"][2][hit]))
    assert np.array_equal(_bits(a["watertight"][3][hit]), _bits(a["brute"][3][hit]))
    assert hit.mean() >= 0.99


def test_the_pinned_rays_hit_what_the_issue_recorded(oracle):
    """Rays A and B: exhaustive search finds triangles 62102 and 49408, each seen edge-on (cos 0.007 and 0.0015) and therefore
    at a computed t IN FRONT of its own box, behind which the walk had already found 53058 and 49406."""
    a = answers(oracle, "full_bsdf", "pinned")
    assert a["brute"][0].tolist() == [62102, 49408]
    assert np.array_equal(_bits(a["brute"][1]), _bits(np.array([0.8293686, 0.27941296], np.float32)))


@pytest.mark.parametrize("exclude", ["none", "owner"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_any_hit_rays_that_end_on_a_vertex(oracle, variant, exclude):
    a = any_answers(oracle, variant, exclude)
    walk = _scene(oracle, variant)[3]
    occ = walk.any(a["o"], a["d"], a["tmax"], a["excluded"])
    vocc, st = walk.any_verified(a["o"], a["d"], a["tmax"], a["excluded"])
    got = {"product walk != exhaustive search": int((occ != a["brute"]).sum()),
           "verified walk != literal oracle": int((vocc != a["literal"]).sum()),
           "oracle's watertight walk != its exhaustive search": int((a["watertight"] != a["brute"]).sum())}
    print(variant, exclude, got, st, "occluded", a["brute"].mean())
    assert got == dict.fromkeys(got, 0)
    assert 0.02 < a["brute"].mean() < 0.98  # both answers occur: the vertex itself ends most rays, an occluder in front of it the rest


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_families_are_not_empty_handed(oracle, variant):
    """From the twin's own counters: exact ties at the final distance and hits the reference's box test loses."""
    walk = _scene(oracle, variant)[3]
    floor = {"vertex_aimed-box": (500, 200), "vertex_aimed-fixed": (500, 200), "parallel-vertex": (3000, 500)}
    for family, (ties, lost) in floor.items():
        a = answers(oracle, variant, family)
        _, _, st = walk.closest_verified(a["o"], a["d"])
        print(variant, family, st)
        assert st["ties"] >= ties and st["lost_hits"] >= lost, (family, st)
        assert (a["brute"][0] >= 0).mean() >= 0.99
