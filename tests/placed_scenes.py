"""Scenes away from [0, 1]^3 and scenes of duplicated geometry, with rays to match (numpy only).

Every other scene of the suite is the Cornell box seen from z = 1.5.  The recipes here move and stretch it -- the vertices
are transformed in float64 and rounded ONCE to fp32, so the product and the oracle are fed the same bytes -- and transform
the ray batches of tests/raygen.py the same way (directions renormalised in float64).  What changes with the place:

  * far from the origin the reference's fp32 slab test loses hits about 10^4 times more often than in [0, 1]^3, so the
    default kernels' rare path (ref_visible, then the literal re-trace) runs at a rate a small batch can see;
  * fp32 merges vertices there: at 1e5 half of the bunny's triangles are duplicates, many of them single points;
  * points(n) and copies(n) are that in the small: n equal boxes, which the builders have to cut by count alone.
"""
import dataclasses

import numpy as np

import raygen

FLT_MAX = np.float32(3.4028234663852886e38)

# name -> (scale per axis, shift per axis)
PLACES = {
    "shift_1e4": ((1.0, 1.0, 1.0), (1e4, 1e4, 1e4)),
    "shift_x_-1e4": ((1.0, 1.0, 1.0), (-1e4, 0.0, 0.0)),
    "stretch_x_1e3": ((1e3, 1.0, 1.0), (0.0, 0.0, 0.0)),
    "squash_y_1e-3": ((1.0, 1e-3, 1.0), (0.0, 0.0, 0.0)),
    "shift_1e5": ((1.0, 1.0, 1.0), (1e5, 1e5, 1e5)),
}
IDENTITY = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
QUERY_PLACES = ("shift_1e4", "shift_x_-1e4", "stretch_x_1e3", "squash_y_1e-3")


def _points(p, scale3, shift3):
    return np.asarray(p, np.float64) * np.asarray(scale3, np.float64) + np.asarray(shift3, np.float64)


def placed(arrays, scale3, shift3):
    """New SceneArrays: every vertex (and point-light position) times scale3 plus shift3, in float64, rounded once to fp32."""
    t = _points(np.asarray(arrays.tris, np.float64).reshape(-1, 3, 3), scale3, shift3)
    lights = arrays.lights.copy()
    if len(lights):
        lights["pos"] = _points(lights["pos"], scale3, shift3).astype(np.float32)
    return dataclasses.replace(arrays, tris=np.ascontiguousarray(t.reshape(-1, 9).astype(np.float32)), lights=lights,
                               name=f"{arrays.name}_placed")


def placed_rays(o, d, scale3, shift3):
    """A ray batch moved with the scene: origins like vertices, directions scaled and renormalised in float64."""
    o2 = _points(o, scale3, shift3).astype(np.float32)
    d2 = np.asarray(d, np.float64) * np.asarray(scale3, np.float64)
    d2 = (d2 / np.linalg.norm(d2, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(o2), np.ascontiguousarray(d2)


def placed_camera(make_camera, scale3, shift3, aspect, lookfrom=(0.5, 0.5, 1.5), lookat=(0.5, 0.5, 0.0)):
    """The default view moved with the scene: make_camera(lookfrom, lookat, up, vfov, aspect) -> 12 floats (Oracle.camera).
    The same call on an unstretched scene; a stretched one is seen from the moved eye, not through a stretched lens."""
    return make_camera(tuple(_points(lookfrom, scale3, shift3)), tuple(_points(lookat, scale3, shift3)), (0.0, 1.0, 0.0), 37.8, aspect)


def camera_batch(cam12, scale3, shift3, n=20_000, seed=11):
    """raygen.camera_rays of the default view's camera (cam12 at the unmoved place), moved with the scene."""
    o, d = raygen.camera_rays(cam12, 1920, 1080, n, seed=seed)
    return placed_rays(o, d, scale3, shift3)


def bounce_batch(o, d, t, hit, n=20_000, seed=5):
    """n rays leaving the hit points of (o, d, t) in random directions, the hit points cycled as often as it takes.
    (raygen.bounce_rays with eps = 0: an offset sized for [0, 1]^3 means nothing at 1e4.)"""
    idx = np.resize(np.where(hit)[0], n)
    return raygen.bounce_rays(o, d, t, idx, seed=seed, eps=0.0)


def aimed_batch(tris, n=20_000, seed=7, distance=0.2):
    """n rays from `distance` away, all around, aimed at random points of the given triangles (points(n), copies(n): the view
    rays hardly ever meet the one small triangle; these all cross the run of equal boxes, and on copies(n) every hit is an
    exact tie of n triangles)."""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    rng = np.random.default_rng(seed)
    c = np.einsum("nk,nka->na", rng.dirichlet((1.0, 1.0, 1.0), n), t[rng.integers(0, len(t), n)])
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    o = (c - distance * dirs).astype(np.float32)
    d = c - o.astype(np.float64)
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def any_batch(cpu, arrays, o, d, seed, tmax_scale=1.0):
    """The _any_batch recipe of test_gpu_query.py: bounce rays off the closest hits, tmax uniform in (0.05, 1.2) times
    tmax_scale (the smallest scale factor of the place), the excluded triangle drawn from the light triangles and -1."""
    c = cpu.trace_closest(o, d, np.full(len(o), FLT_MAX, np.float32))
    o2, d2 = raygen.bounce_rays(o, d, c[1], c[0] >= 0, seed=seed, eps=0.0)
    rng = np.random.default_rng(seed + 1)
    tm = (rng.uniform(0.05, 1.2, len(o2)) * tmax_scale).astype(np.float32)
    light_tris = np.where(arrays.tri_light >= 0)[0]
    excl = rng.choice(np.concatenate([light_tris, [-1]]), len(o2)).astype(np.int32)
    return o2, d2, tm, excl


def _with_extra(box, extra):
    """The bare Cornell box with `extra` triangles (material 0, no light) in front of it: the box keeps its indices + len(extra)."""
    n = len(extra)
    lights = box.lights.copy()
    lights["tri"] += n
    return dataclasses.replace(
        box, tris=np.ascontiguousarray(np.concatenate([extra, box.tris]), np.float32),
        tri_material=np.concatenate([np.zeros(n, np.int32), box.tri_material]).astype(np.int32),
        tri_light=np.concatenate([np.full(n, -1, np.int32), box.tri_light]).astype(np.int32), lights=lights)


def _bunny_triangle():
    from rtcuda_amd import scenes
    return np.asarray(scenes.cornell_bunny("matte").tris, np.float32).reshape(-1, 9)[100].copy()


def points(n):
    """n copies of one bunny triangle collapsed to its first vertex, plus the bare box so that rays have something to hit."""
    from rtcuda_amd import scenes
    tri = np.tile(_bunny_triangle()[:3], 3)
    out = _with_extra(scenes.cornell_bunny("matte", bunny=False), np.repeat(tri[None, :], n, axis=0))
    return dataclasses.replace(out, name=f"points_{n}")


def copies(n):
    """n identical copies of one bunny triangle, plus the bare box."""
    from rtcuda_amd import scenes
    out = _with_extra(scenes.cornell_bunny("matte", bunny=False), np.repeat(_bunny_triangle()[None, :], n, axis=0))
    return dataclasses.replace(out, name=f"copies_{n}")


def scene(name, variant="matte"):
    """(arrays, scale3, shift3) of a named case: a key of PLACES, "points_N" or "copies_N"."""
    from rtcuda_amd import scenes
    if name in PLACES:
        s, t = PLACES[name]
        return placed(scenes.cornell_bunny(variant), s, t), s, t
    kind, n = name.split("_")
    return {"points": points, "copies": copies}[kind](int(n)), IDENTITY[0], IDENTITY[1]
