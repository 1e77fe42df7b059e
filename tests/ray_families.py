"""Seeded rays through the places random rays never find: mesh vertices, edges, and along the axes (numpy only).

Every family is a function (tris, n, seed) -> (o, d), both float32 of shape (n, 3); `tris` is the scene's (m, 3, 3) or (m, 9)
float32 vertex array.  Points are computed in float64 and rounded to float32 once.  Such rays pass through box faces and box
corners of any tree built over the mesh (a node's box ends on vertices) and hit several triangles at exactly the same t, which
is where a box test that "only culls" has to be conservative to the last bit and where the tie rule decides the triangle.
"""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
FIXED_ORIGIN = (0.5, 0.5, 1.5)  # the default camera's position
SCALES = (2.0 ** -10, 2.0 ** -20, 2.0 ** -24, 2.0 ** 10)

# Two rays with ordinary directions whose nearer hit the product's walk lost (cornell_bunny("full_bsdf")): bit patterns of o, d
PINNED_A = (np.array([1063954181, 1059423177, 3211744549], np.uint32), np.array([3207771391, 3206515754, 1052016152], np.uint32))
PINNED_B = (np.array([1058765432, 1050963721, 3204798221], np.uint32), np.array([3208731264, 3204483550, 3201805114], np.uint32))


def pinned_rays():
    """Rays A and B -> (o (2, 3), d (2, 3)) float32."""
    o = np.stack([PINNED_A[0], PINNED_B[0]]).view(np.float32)
    d = np.stack([PINNED_A[1], PINNED_B[1]]).view(np.float32)
    return o, d


def _verts(tris):
    return np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)


def _unit32(v64):
    return (v64 / np.linalg.norm(v64, axis=1, keepdims=True)).astype(np.float32)


def _origins(rng, n, origin):
    if origin == "fixed":
        return np.tile(np.array(FIXED_ORIGIN, np.float32), (n, 1))
    assert origin == "box", origin
    o = rng.uniform(0.05, 0.95, (n, 3)).astype(np.float32)
    o[:, 2] = -o[:, 2]
    return o


def _random_vertices(rng, v, n):
    """A random vertex of a random triangle -> (points (n, 3) float32, triangle indices)."""
    t = rng.integers(0, len(v), n)
    return v[t, rng.integers(0, 3, n)], t


def _edge_points(rng, v, n, where):
    """Points on a random edge of a random triangle, float64: the midpoint, or a uniform point of the edge."""
    t = rng.integers(0, len(v), n)
    e = rng.integers(0, 3, n)
    a, b = v[t, e].astype(np.float64), v[t, (e + 1) % 3].astype(np.float64)
    s = np.full((n, 1), 0.5) if where == "midpoint" else rng.uniform(0.0, 1.0, (n, 1))
    assert where in ("midpoint", "random"), where
    return a + s * (b - a)


def _aim(o, p64):
    """Unit directions from the float32 origins o to the points p64; rays that would have no length get a fixed direction."""
    w = p64 - o.astype(np.float64)
    w[np.linalg.norm(w, axis=1) == 0] = (0.0, 0.0, -1.0)
    return _unit32(w)


def vertex_aimed(tris, n, seed, origin="box"):
    """d = unit(v - o) for a random vertex v of a random triangle.  origin: "box" -- uniform in (0.05, 0.95)^3 with z negated
    (inside the Cornell box) -- or "fixed", all rays from FIXED_ORIGIN."""
    rng = np.random.default_rng(seed)
    o = _origins(rng, n, origin)
    p, _ = _random_vertices(rng, _verts(tris), n)
    return o, _aim(o, p.astype(np.float64))


def edge_aimed(tris, n, seed, where="midpoint", origin="box"):
    """The same towards edge midpoints (where="midpoint") or uniform points on edges ("random")."""
    rng = np.random.default_rng(seed)
    o = _origins(rng, n, origin)
    return o, _aim(o, _edge_points(rng, _verts(tris), n, where))


def parallel_through(tris, n, seed, through="vertex", form="plus_zero"):
    """Parallel rays from the plane z = 1.5 down the z axis, one through each chosen point (a vertex, or an edge midpoint).
    form "plus_zero": d = (0, 0, -1) exactly; "minus_zero": the same with the zero components -0.0; "tilted": the control with no
    zero component, d = unit(1e-3, 2e-3, -1), the origin moved so that the ray still passes through the point."""
    rng = np.random.default_rng(seed)
    v = _verts(tris)
    if through == "vertex":
        p = _random_vertices(rng, v, n)[0].astype(np.float64)
    else:
        assert through == "edge", through
        p = _edge_points(rng, v, n, "midpoint")
    if form == "tilted":
        w = np.array([1e-3, 2e-3, -1.0])
        w /= np.linalg.norm(w)
        o = (p + ((1.5 - p[:, 2]) / w[2])[:, None] * w).astype(np.float32)
        o[:, 2] = np.float32(1.5)
        return o, np.tile(w.astype(np.float32), (n, 1))
    zero = {"plus_zero": np.float32(0.0), "minus_zero": np.float32(-0.0)}[form]
    o = np.stack([p[:, 0], p[:, 1], np.full(n, 1.5)], axis=1).astype(np.float32)
    d = np.tile(np.array([zero, zero, np.float32(-1.0)], np.float32), (n, 1))
    return o, d


def ends_on_vertex(tris, n, seed, exclude="none"):
    """Any-hit rays from random points towards vertices that END on the vertex -> (o, d, tmax, excluded).  tmax is the fp32
    distance to the vertex for a third of the rays, the float below it for a third, the float above for the rest.
    exclude: "none" (-1 everywhere) or "owner": the triangle the vertex was drawn from."""
    rng = np.random.default_rng(seed)
    o = _origins(rng, n, "box")
    p, t = _random_vertices(rng, _verts(tris), n)
    w = p.astype(np.float64) - o.astype(np.float64)
    dist = np.linalg.norm(w, axis=1).astype(np.float32)
    k = np.arange(n) % 3
    tmax = np.where(k == 0, dist, np.where(k == 1, np.nextafter(dist, np.float32(0)), np.nextafter(dist, FLT_MAX))).astype(np.float32)
    assert exclude in ("none", "owner"), exclude
    excluded = t.astype(np.int32) if exclude == "owner" else np.full(n, -1, np.int32)
    return o, _aim(o, p.astype(np.float64)), tmax, excluded


def scaled(d, s):
    """The directions times s (a power of two: exact unless it underflows): the same rays, with every t divided by s."""
    return (np.asarray(d, np.float32) * np.float32(s)).astype(np.float32)


def closest_families(tris, n, seed0=100):
    """name -> (o, d): every closest-hit family of this module, seeded from seed0 on."""
    return {
        "vertex_aimed-box": vertex_aimed(tris, n, seed0, "box"),
        "vertex_aimed-fixed": vertex_aimed(tris, n, seed0 + 1, "fixed"),
        "edge_aimed-midpoint": edge_aimed(tris, n, seed0 + 2, "midpoint", "box"),
        "edge_aimed-random": edge_aimed(tris, n, seed0 + 3, "random", "box"),
        "edge_aimed-midpoint-fixed": edge_aimed(tris, n, seed0 + 4, "midpoint", "fixed"),
        "edge_aimed-random-fixed": edge_aimed(tris, n, seed0 + 7, "random", "fixed"),
        "parallel-vertex": parallel_through(tris, n, seed0 + 5, "vertex", "plus_zero"),
        "parallel-vertex-minus_zero": parallel_through(tris, n, seed0 + 5, "vertex", "minus_zero"),
        "parallel-vertex-tilted": parallel_through(tris, n, seed0 + 5, "vertex", "tilted"),
        "parallel-edge": parallel_through(tris, n, seed0 + 6, "edge", "plus_zero"),
        "parallel-edge-minus_zero": parallel_through(tris, n, seed0 + 6, "edge", "minus_zero"),
        "parallel-edge-tilted": parallel_through(tris, n, seed0 + 6, "edge", "tilted"),
    }
