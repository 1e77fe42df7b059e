"""Small deterministic scenes and function-input tables for the reference pins.  TEST HELPER (a plain module).

Every scene of the parity suites lives in x, y in [0, 1], z in [-1, 0], has one glass index, and axis-aligned area lights
overhead.  The scenes here reach what those do not (see FRAMES): a box CENTRED ON THE ORIGIN, so hit points have both signs
in every coordinate and many lie within 1/32 of zero (both branches of offset_ray_origin, utility.cuh:40-46); glass of index
1.0, below 1 and above 2 with total internal reflection and near-grazing incidence; a mirror at grazing angles; slanted area
lights of very different areas; point lights only, mixed, none, seven; an emitter seen directly; max_bounces 0, 1 and above
RR_START; frames of more than 2^20 camera rays (several generations, slot reuse); two seeds.

tests/golden/make_ref_render_fixture.py renders FRAMES with the reference's own source compiled for the CPU
(oracle/ref_render_driver.cpp) and commits inputs and outputs as tests/golden/ref_render_fixture.npz;
make_ref_shade_fixture.py does the same for the function tables of shade_tables() (oracle/ref_shade_driver.cpp,
tests/golden/ref_shade_fixture.npz).  Everything here is a function of constants and of numpy's seeded PCG64 streams."""
from __future__ import annotations

import numpy as np

from rtcuda_amd import scenes

MATTE, MIRROR, GLASS = scenes.MATTE, scenes.MIRROR, scenes.GLASS
W = 1 << 20


# ------------------------------------------------------------------------------------------------ scene building
class _Builder:
    def __init__(self):
        self.tris, self.mat, self.light = [], [], []
        self.materials, self.lights = [], []

    def material(self, kind, albedo=(0, 0, 0), ior=0.0):
        self.materials.append((tuple(albedo), ior, kind))
        return len(self.materials) - 1

    def tri(self, a, b, c, m, L=None):
        self.tris.append(tuple(a) + tuple(b) + tuple(c))
        self.mat.append(m)
        if L is None:
            self.light.append(-1)
        else:
            self.lights.append((scenes.AREA_LIGHT, (0, 0, 0), len(self.tris) - 1, tuple(L)))
            self.light.append(len(self.lights) - 1)

    def quad(self, a, b, c, d, m, L=None):
        self.tri(a, b, c, m, L)
        self.tri(a, c, d, m, L)

    def point(self, pos, I):
        self.lights.append((scenes.POINT_LIGHT, tuple(pos), -1, tuple(I)))

    def box(self, lo, hi, mats):
        """Axis-aligned box; mats = one material or six (x-, x+, y-, y+, z-, z+)."""
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        m = [mats] * 6 if isinstance(mats, int) else list(mats)
        self.quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0), m[0])
        self.quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1), m[1])
        self.quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1), m[2])
        self.quad((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0), m[3])
        self.quad((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0), m[4])
        self.quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1), m[5])

    def wedge(self, base, size, m):
        """A prism with a slanted face: glass paths inside it meet faces well past the critical angle."""
        x, y, z = base
        sx, sy, sz = size
        a, b, c = (x, y, z), (x + sx, y, z), (x, y + sy, z)
        d, e, f = (x, y, z + sz), (x + sx, y, z + sz), (x, y + sy, z + sz)
        self.tri(a, c, b, m)
        self.tri(d, e, f, m)
        self.quad(a, b, e, d, m)
        self.quad(a, d, f, c, m)
        self.quad(b, c, f, e, m)

    def arrays(self, name):
        mats = np.zeros(len(self.materials), dtype=scenes.MATERIAL_DTYPE)
        for i, (a, ior, kind) in enumerate(self.materials):
            mats[i] = (a, ior, kind)
        lights = np.zeros(len(self.lights), dtype=scenes.LIGHT_DTYPE)
        for i, l in enumerate(self.lights):
            lights[i] = l
        return scenes.SceneArrays(tris=np.array(self.tris, np.float32).reshape(-1, 9), tri_material=np.array(self.mat, np.int32),
                                  tri_light=np.array(self.light, np.int32), materials=mats, lights=lights, name=name)


def _room(b, bright=False):
    """The box centred on the origin, [-1, 1]^3, walls of five colours -> the white material."""
    k = 0.95 if bright else 0.7
    red, green, white = b.material(MATTE, (k, 0.08, 0.06)), b.material(MATTE, (0.1, k, 0.15)), b.material(MATTE, (k, k, k))
    blue, sand = b.material(MATTE, (0.2, 0.25, k)), b.material(MATTE, (k, 0.8 * k, 0.6 * k))
    b.box((-1, -1, -1), (1, 1, 1), (red, green, sand, white, blue, white))
    return white


def _slanted_light(b, centre, u, v, L, m):
    """A slanted light of two triangles, each a light of its own, over the parallelogram centre +- u +- v -- with the fourth
    corner lifted off the plane.  The two must NOT be coplanar: shading a point of one while sampling the other would put wi
    in the sampled triangle's plane, where the reference's estimator divides inf by inf once the two normals round
    differently (light.cuh:45, utility.cuh:53-56; about one such shade in forty yields a NaN pixel)."""
    c, u, v = (np.asarray(x, np.float64) for x in (centre, u, v))
    n = np.cross(u, v)
    lift = 0.25 * np.linalg.norm(u) * n / np.linalg.norm(n)
    b.quad(c - u - v, c + u - v, c + u + v, c - u + v + lift, m, L)


def _furniture(b, white):
    """Matte things that cross the coordinate planes: a thin plate just above y = 0 and a slanted sheet through the origin."""
    grey = b.material(MATTE, (0.55, 0.5, 0.6))
    b.quad((-0.5, 0.01, -0.6), (0.45, 0.01, -0.6), (0.45, 0.02, 0.1), (-0.5, 0.02, 0.1), grey)
    b.quad((-0.3, -0.9, 0.02), (0.02, -0.9, -0.3), (0.02, -0.2, -0.3), (-0.3, -0.2, 0.02), white)


def scene_origin_box():
    b = _Builder()
    white = _room(b)
    _furniture(b, white)
    _slanted_light(b, (0.2, 0.93, -0.1), (0.3, 0.04, 0.0), (0.0, 0.03, 0.25), (9, 9, 8), white)
    return b.arrays("origin_box")


def scene_glass():
    """Glass of four indices (1.0, 0.8, 1.5, 2.4): a slab each, and wedges of 1.5 and 2.4 (total internal reflection)."""
    b = _Builder()
    white = _room(b)
    g = [b.material(GLASS, ior=i) for i in (1.0, 0.8, 1.5, 2.4)]
    for k, x in enumerate((-0.85, -0.4, 0.05, 0.5)):
        b.box((x, -0.6 + 0.1 * k, -0.35), (x + 0.33, 0.1 * k, -0.3 + 0.04 * k), g[k])
    b.wedge((-0.7, -0.95, -0.1), (0.6, 0.5, 0.45), g[2])
    b.wedge((0.1, -0.95, 0.0), (0.55, 0.6, 0.4), g[3])
    b.quad((-0.9, -0.999, 0.5), (0.9, -0.999, 0.5), (0.9, -0.99, 0.9), (-0.9, -0.99, 0.9), g[2])  # seen at grazing angles
    _slanted_light(b, (0.0, 0.9, 0.2), (0.45, 0.05, 0.0), (0.0, 0.0, 0.4), (6, 6, 6), white)
    b.point((-0.6, 0.5, 0.6), (0.5, 0.45, 0.4))
    return b.arrays("glass")


def scene_mirror():
    """A mirror floor under a low camera (grazing angles), a slanted mirror, a small bright light and a large dim one."""
    b = _Builder()
    white = _room(b)
    m1, m2 = b.material(MIRROR, (0.9, 0.9, 0.95)), b.material(MIRROR, (0.95, 0.7, 0.5))
    b.quad((-0.95, -0.97, -0.95), (0.95, -0.97, -0.95), (0.95, -0.97, 0.95), (-0.95, -0.97, 0.95), m1)
    b.quad((-0.8, -0.5, -0.9), (0.1, -0.5, -0.7), (0.1, 0.6, -0.75), (-0.8, 0.6, -0.95), m2)
    _furniture(b, white)
    _slanted_light(b, (0.5, 0.6, -0.5), (0.02, 0.01, 0.0), (0.0, 0.01, 0.02), (900, 850, 800), white)   # area 1.8e-3
    _slanted_light(b, (-0.3, 0.9, 0.3), (0.6, 0.08, 0.1), (-0.1, 0.0, 0.5), (1.2, 1.3, 1.5), white)     # area ~1.2
    return b.arrays("mirror")


def scene_lights(kind):
    """The furnished room under: "point" two point lights, "mixed" a point and an area light, "none" no light, "seven" five
    area lights (one triangle each) and two point lights."""
    b = _Builder()
    white = _room(b, bright=(kind == "bright"))
    _furniture(b, white)
    if kind in ("point", "mixed", "seven"):
        b.point((0.4, 0.6, 0.3), (1.1, 1.0, 0.9))
    if kind in ("point", "seven"):
        b.point((-0.7, -0.3, -0.6), (0.3, 0.5, 0.8))
    if kind in ("mixed", "bright"):
        _slanted_light(b, (-0.2, 0.92, -0.2), (0.3, 0.05, 0.0), (0.0, 0.0, 0.3), (7, 7, 7), white)
    if kind == "seven":
        for k in range(5):
            x = -0.8 + 0.38 * k
            b.tri((x, 0.95 - 0.02 * k, -0.5), (x + 0.1 + 0.05 * k, 0.9, -0.5), (x, 0.93, -0.2 + 0.1 * k), white,
                  (3 + 2 * k, 8 - k, 4 + k))
    return b.arrays("lights_" + kind)


def scene_emitter():
    """A large emitter facing the camera (bounce-0 emission on most pixels), glass and a mirror in front of it."""
    b = _Builder()
    white = _room(b)
    _slanted_light(b, (0.0, 0.0, -0.9), (0.7, 0.1, 0.0), (-0.1, 0.6, 0.05), (2.0, 1.5, 1.0), white)
    b.box((-0.3, -0.4, -0.2), (0.1, 0.0, 0.1), b.material(GLASS, ior=1.33))
    b.quad((0.3, -0.6, -0.5), (0.8, -0.6, -0.1), (0.8, 0.3, -0.1), (0.3, 0.3, -0.5), b.material(MIRROR, (0.8, 0.8, 0.8)))
    return b.arrays("emitter")


def scene_all():
    """Everything at once, for the frames of several generations."""
    b = _Builder()
    white = _room(b)
    _furniture(b, white)
    b.box((-0.8, -0.9, -0.7), (-0.35, -0.3, -0.3), b.material(GLASS, ior=1.5))
    b.wedge((0.3, -0.95, -0.2), (0.5, 0.6, 0.4), b.material(GLASS, ior=2.2))
    b.quad((0.2, -0.7, -0.95), (0.9, -0.7, -0.8), (0.9, 0.5, -0.8), (0.2, 0.5, -0.95), b.material(MIRROR, (0.9, 0.85, 0.8)))
    _slanted_light(b, (0.1, 0.9, 0.0), (0.35, 0.06, 0.0), (0.0, 0.02, 0.3), (8, 7.5, 7), white)
    b.point((-0.5, 0.3, 0.7), (0.4, 0.4, 0.5))
    return b.arrays("all")


_SCENES = {
    "origin_box": scene_origin_box, "glass": scene_glass, "mirror": scene_mirror, "emitter": scene_emitter, "all": scene_all,
    "lights_point": lambda: scene_lights("point"), "lights_mixed": lambda: scene_lights("mixed"),
    "lights_none": lambda: scene_lights("none"), "lights_seven": lambda: scene_lights("seven"),
    "lights_bright": lambda: scene_lights("bright"),
}

CAM_FRONT = ((0.05, 0.1, 0.92), (0.0, -0.05, -0.3), (0.0, 1.0, 0.0), 75.0)
CAM_LOW = ((0.1, -0.9, 0.9), (-0.1, -0.85, -0.9), (0.0, 1.0, 0.0), 60.0)      # 7 cm above the mirror floor
CAM_SIDE = ((-0.9, 0.5, 0.85), (0.3, -0.4, -0.4), (0.1, 1.0, 0.0), 65.0)

# name: (scene, camera, w, h, spp, max_bounces, seed)
FRAMES = {
    "origin_box": ("origin_box", CAM_FRONT, 48, 48, 8, 10, 1),
    "glass": ("glass", CAM_FRONT, 64, 48, 8, 10, 1),
    "glass_side_seed7": ("glass", CAM_SIDE, 48, 64, 6, 8, 7),
    "mirror_grazing": ("mirror", CAM_LOW, 64, 40, 8, 6, 1),
    "lights_point": ("lights_point", CAM_SIDE, 40, 40, 6, 5, 1),
    "lights_mixed": ("lights_mixed", CAM_FRONT, 40, 40, 6, 5, 1),
    "lights_none": ("lights_none", CAM_FRONT, 32, 32, 4, 5, 1),
    "lights_seven": ("lights_seven", CAM_SIDE, 48, 40, 8, 7, 7),
    "emitter": ("emitter", CAM_FRONT, 48, 48, 6, 6, 1),
    "roulette": ("lights_bright", CAM_FRONT, 40, 40, 8, 14, 1),     # max_bounces > RR_START = 4: long roulette chains
    "bounces_0": ("emitter", CAM_FRONT, 40, 40, 4, 0, 1),
    "bounces_1": ("emitter", CAM_FRONT, 40, 40, 4, 1, 1),
    "generations_a": ("all", CAM_FRONT, 64, 64, 300, 6, 1),         # 1.17 generations
    "generations_b": ("all", CAM_SIDE, 48, 40, 1200, 9, 7),         # 2.2 generations, spp does not divide 2^20
}


def frame(name):
    """-> (SceneArrays, camera (lookfrom, lookat, up, vfov, aspect), w, h, spp, max_bounces, seed)"""
    scene, (lookfrom, lookat, up, vfov), w, h, spp, max_bounces, seed = FRAMES[name]
    return _SCENES[scene](), (lookfrom, lookat, up, vfov, w / h), w, h, spp, max_bounces, seed


def frame_arrays(name):
    """The arrays a frame is stored as in the render fixture: key -> ndarray."""
    a, (lookfrom, lookat, up, vfov, aspect), w, h, spp, max_bounces, seed = frame(name)
    return {
        "tris": a.tris, "tri_material": a.tri_material, "tri_light": a.tri_light,
        "materials": a.materials.view(np.uint8).reshape(len(a.materials), -1) if len(a.materials) else np.zeros((0, 20), np.uint8),
        "lights": a.lights.view(np.uint8).reshape(len(a.lights), -1) if len(a.lights) else np.zeros((0, 32), np.uint8),
        "camera_params": np.array(list(lookfrom) + list(lookat) + list(up) + [vfov, aspect], np.float32),
        "params": np.array([w, h, spp, max_bounces, seed], np.int32),
    }


def scene_from_arrays(d, name=""):
    """SceneArrays of a stored frame (the inverse of frame_arrays)."""
    return scenes.SceneArrays(tris=np.ascontiguousarray(d["tris"], np.float32), tri_material=np.ascontiguousarray(d["tri_material"], np.int32),
                              tri_light=np.ascontiguousarray(d["tri_light"], np.int32),
                              materials=np.ascontiguousarray(d["materials"]).view(scenes.MATERIAL_DTYPE).reshape(-1),
                              lights=np.ascontiguousarray(d["lights"]).view(scenes.LIGHT_DTYPE).reshape(-1), name=name)


# ------------------------------------------------------------------------------------------------ replayed uniforms
_C = np.float32(2.3283064e-10)
_WEYL = 362437
_M32 = 0xFFFFFFFF


def uniform_of(raw):
    """curand_uniform of raw 32-bit draws, in float32: raw * 2^-32 + 2^-33 (raw 0 -> 2^-33, raw 2^32 - 1 -> 1.0)."""
    return (np.asarray(raw, np.uint32).astype(np.float32) * _C + (_C / np.float32(2.0))).astype(np.float32)


def _inv_g(a):
    """x with g(x) = a, where g(x) = t ^ (t << 1), t = x ^ (x >> 2): the way XORWOW's oldest word enters a draw."""
    t, s = a, 1
    while s < 32:           # invert t ^ (t << 1): prefix xor from the low bit
        t = (t ^ (t << s)) & _M32
        s <<= 1
    x, s = t, 2
    while s < 32:           # invert x ^ (x >> 2)
        x ^= x >> s
        s <<= 1
    return x & _M32


def xorwow_state_for(raws):
    """An XORWOW state {d, v0 .. v4} whose next len(raws) <= 5 draws are exactly `raws`: the oracle's generator replays a
    list of draws from it, as the shade driver's replaying curandState does.  (Draw k uses the k-th word as its oldest word
    and the previous draw's newest; d = 0, v4 = 0, so at most four.)"""
    assert len(raws) <= 4
    v = [0, 0, 0, 0, 0]
    newest, d = 0, 0
    for k, r in enumerate(raws):
        d = (d + _WEYL) & _M32
        want = (int(r) - d) & _M32                         # the newest word after this draw
        v[k] = _inv_g(want ^ (newest ^ (newest << 4)) & _M32)
        newest = want
    return np.array([0] + v, np.uint32)


def _inv_g_array(a):
    """_inv_g on a uint32 array."""
    t = np.asarray(a, np.uint64) & np.uint64(_M32)
    s = 1
    while s < 32:
        t = (t ^ (t << np.uint64(s))) & np.uint64(_M32)
        s <<= 1
    x, s = t, 2
    while s < 32:
        x = x ^ (x >> np.uint64(s))
        s <<= 1
    return x & np.uint64(_M32)


def xorwow_states_for2(raws2):
    """xorwow_state_for on every row of an (n, 2) table of raw draws at once -> (n, 6) uint32."""
    r = np.asarray(raws2, np.uint32).astype(np.uint64)
    m = np.uint64(_M32)
    out = np.zeros((len(r), 6), np.uint32)
    want0 = (r[:, 0] - np.uint64(_WEYL)) & m
    out[:, 1] = _inv_g_array(want0).astype(np.uint32)
    want1 = (r[:, 1] - np.uint64(2 * _WEYL)) & m
    out[:, 2] = _inv_g_array(want1 ^ ((want0 ^ (want0 << np.uint64(4))) & m)).astype(np.uint32)
    return out


# ------------------------------------------------------------------------------------------------ function tables
WORDS_IN = {1: 13, 2: 14, 3: 21, 4: 22, 5: 11, 6: 16, 7: 6, 8: 2, 9: 9, 10: 6, 11: 8, 12: 2, 13: 14}
WORDS_OUT = {1: 11, 2: 5, 3: 10, 4: 1, 5: 5, 6: 4, 7: 3, 8: 1, 9: 1, 10: 3, 11: 3, 12: 4, 13: 6}
FUNCTIONS = {1: "sample_f", 2: "get_f", 3: "sample_Li", 4: "pdf_Li", 5: "sample_p", 6: "intersect", 7: "offset_ray_origin",
             8: "power_heuristic", 9: "same_hemisphere", 10: "reflect", 11: "refract", 12: "uniform_sample_sphere", 13: "get_ray"}
RAW_EDGES = [0, 0xFFFFFFFF, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFF00, 0x3FFFFFFF]   # uniforms 2^-33 and 1.0 first


def _f(x):
    return np.asarray(x, np.float32)


def _bits(x):
    return _f(x).view(np.uint32)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _units(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _next(x, k=1):
    """The float32 k steps above (k < 0: below) x."""
    x = _f(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


def _raws(rng, n, cols=2):
    r = rng.integers(0, 1 << 32, size=(n, cols), dtype=np.uint64).astype(np.uint32)
    k = min(n, len(RAW_EDGES))
    for c in range(cols):
        r[:k, c] = np.roll(RAW_EDGES, c)[:k]
    return r


def _materials_rows(rng, n):
    """n material rows {albedo3, ior, type} as words; types cycle, glass indices include 1.0, below 1 and above 2."""
    iors = _f([1.0, 0.8, 1.5, 2.4, 1.33, 0.5, 3.0, 1.0000001])
    w = np.zeros((n, 5), np.uint32)
    w[:, 0:3] = _bits(rng.uniform(0.05, 0.95, (n, 3)))
    kind = np.arange(n) % 3
    w[:, 3] = _bits(np.where(kind == GLASS, iors[(np.arange(n) // 3) % len(iors)], 0.0))
    w[:, 4] = kind.astype(np.uint32)
    return w


def _critical_rows():
    """(wo, n, ior) with n = +z and sin(theta) within a few ulp of 1 / eta on either side: leaving glass of index ior."""
    rows = []
    for ior in (1.5, 2.4, 1.33, 1.0, 1.0000001):
        s0 = np.float32(1.0) / np.float32(ior)
        for k in (-3, -2, -1, 0, 1, 2, 3):
            s = min(float(_next(s0, k)), 1.0)
            c = np.sqrt(max(0.0, 1.0 - s * s))
            rows.append(((s, 0.0, c), (0.0, 0.0, 1.0), ior))       # dot(wo, n) > 0: inside, eta = ior
            rows.append(((s, 0.0, -c), (0.0, 0.0, 1.0), 1.0 / ior))  # entering a medium of index < 1
    return rows


def _tri_rows(rng, n):
    """n triangles p0 p1 p2 (9 floats): random, slanted, of areas from 1e-6 to 4; the first is degenerate (zero area)."""
    c = rng.uniform(-1, 1, (n, 1, 3))
    s = 10.0 ** rng.uniform(-3, 0.3, (n, 1, 1))
    t = (c + s * rng.normal(size=(n, 3, 3))).astype(np.float32)
    t[0, 2] = t[0, 0] + np.float32(2.0) * (t[0, 1] - t[0, 0])      # collinear: n = 0 or nearly, area ~ 0
    t[1, 1] = t[1, 0]                                               # two equal vertices: exactly zero area
    return t.reshape(n, 9)


def shade_tables(n_random=600):
    """function id -> (rows, WORDS_IN) uint32: the inputs of the shade fixture."""
    rng = np.random.default_rng(20260117)
    out = {}
    z, nz = np.float32(0.0), np.float32(-0.0)
    ax = _f([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]])

    # ---- 1 sample_f: random directions, then the edges: dot(wo, n) = 0 and +-1 exactly, the critical angle, ior 1
    n = n_random
    wo, nn = _units(rng, n), _units(rng, n)
    mats = _materials_rows(rng, n)
    raws = _raws(rng, n)
    edge = []
    for kind in (MATTE, MIRROR, GLASS):
        for ior in (1.5, 1.0, 0.8, 2.4):
            for a in ax:
                for b_ in ax:      # dot = 0 (perpendicular axes), +1 and -1 (equal / opposite axes)
                    edge.append((kind, ior, a, b_))
    crit = _critical_rows()
    for wo_c, n_c, ior in crit:
        edge.append((GLASS, ior, _f(wo_c), _f(n_c)))
    e = len(edge)
    em = np.zeros((e, 5), np.uint32)
    em[:, 0:3] = _bits(np.full((e, 3), 0.5))
    em[:, 3] = _bits([x[1] for x in edge])
    em[:, 4] = np.array([x[0] for x in edge], np.uint32)
    ewo, en = _f([x[2] for x in edge]), _f([x[3] for x in edge])
    er = _raws(rng, e)
    out[1] = np.concatenate([np.concatenate([mats, _bits(wo), _bits(nn), raws], axis=1),
                             np.concatenate([em, _bits(ewo), _bits(en), er], axis=1)])

    # ---- 2 get_f: random, wi and wo on either side, exact zeros of either dot
    wi = _units(rng, n)
    rows = np.concatenate([_materials_rows(rng, n), _bits(wo), _bits(wi), _bits(nn)], axis=1)
    e2 = [(a, b_, c) for a in ax for b_ in ax for c in ax[:3]]
    m2 = np.zeros((len(e2), 5), np.uint32)
    m2[:, 0:3] = _bits(np.full((len(e2), 3), 0.25))
    edge2 = np.concatenate([m2, _bits([x[0] for x in e2]), _bits([x[1] for x in e2]), _bits([x[2] for x in e2])], axis=1)
    out[2] = np.concatenate([rows, edge2])

    # ---- 3 sample_Li / 4 pdf_Li / 5 sample_p / 6 intersect share triangles
    tris = _tri_rows(rng, n)
    p = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32)
    ltype = (np.arange(n) % 4 != 0).astype(np.uint32)               # a quarter point lights
    ltype[0] = 1                                                    # (the degenerate triangles are area lights)
    pos = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    pos[4] = p[4]                                                   # the shading point ON a point light: t = 0
    pos[8] = p[8]
    L = rng.uniform(0.1, 20, (n, 3)).astype(np.float32)
    light = np.concatenate([ltype[:, None], _bits(pos), _bits(L), _bits(tris)], axis=1)
    raws = _raws(rng, n)
    # wi in the plane of the light triangle: the shading point on the triangle's plane (rows 12 .. 40: p = p0 + a e + b f)
    t3 = tris.reshape(n, 3, 3)
    for k in range(12, 40):
        a_, b_ = rng.uniform(-2, 3, 2)
        p[k] = (t3[k, 0] + np.float32(a_) * (t3[k, 1] - t3[k, 0]) + np.float32(b_) * (t3[k, 2] - t3[k, 0])).astype(np.float32)
    out[3] = np.concatenate([light, _bits(p), raws], axis=1)
    # pdf_Li: directions aimed at the triangle (so it is hit), random ones, and in-plane ones
    aim = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    target = np.einsum("nk,nkc->nc", aim, t3)
    wi4 = _unit(target.astype(np.float64) - p)
    wi4[1::5] = _units(rng, len(wi4[1::5]))
    for k in range(12, 40):
        wi4[k] = _unit(t3[k, 1].astype(np.float64) - p[k]) if np.any(t3[k, 1] != p[k]) else ax[0]
    out[4] = np.concatenate([light, _bits(p), _bits(wi4)], axis=1)
    out[5] = np.concatenate([_bits(tris), raws], axis=1)
    o6 = p.copy()
    d6 = wi4.copy()
    tmax = np.where(np.arange(n) % 3 == 0, np.float32(3.4028234663852886e38), rng.uniform(0.0, 3.0, n)).astype(np.float32)
    # a ray that ends exactly ON the triangle (t = tmax is accepted), one step short and one step past
    dist = np.linalg.norm(target.astype(np.float64) - p, axis=1).astype(np.float32)
    tmax[2::7] = dist[2::7]
    out[6] = np.concatenate([_bits(tris), _bits(o6), _bits(d6), _bits(tmax)[:, None]], axis=1)

    # ---- 7 offset_ray_origin: both signs of every coordinate, 0, -0, +-1/32 and their neighbours, tiny and large values
    o32 = np.float32(1.0 / 32.0)
    specials = _f([z, nz, o32, -o32, _next(o32), _next(o32, -1), _next(-o32), _next(-o32, -1), 1e-30, -1e-30, 1e-3, -1e-3,
                   0.03, -0.03, 0.5, -0.5, 1.0, -1.0, 100.0, -100.0, 1.1754944e-38, -1.1754944e-38, 0.99999994, -0.99999994])
    pp = np.concatenate([rng.uniform(-1.5, 1.5, (n, 3)), rng.uniform(-1 / 16, 1 / 16, (n, 3))]).astype(np.float32)
    nn7 = _units(rng, len(pp))
    sp = np.array([(a, b_, c) for a in specials for b_ in specials[:8] for c in specials[8:12]], np.float32)
    sn = np.concatenate([_units(rng, len(sp) - 12), ax, -ax])[:len(sp)]
    out[7] = np.concatenate([np.concatenate([_bits(pp), _bits(nn7)], axis=1), np.concatenate([_bits(sp), _bits(sn)], axis=1)])

    # ---- 8 power_heuristic: every class the int parameter distinguishes below 2^31: |g| < 1 (-> 0), 1 <= g < 46341 (g * g
    # exact), g >= 46341 (the int square wraps), negative g, and f of 0, tiny, huge and inf
    g = np.concatenate([rng.uniform(0, 1, 300), rng.uniform(1, 50, 300), rng.uniform(50, 46340, 300), rng.uniform(46341, 2.0e9, 300),
                        -rng.uniform(0, 2.0e9, 200), [0.0, -0.0, 0.99999994, 1.0, 1.9999999, 2.0, 46340.0, 46340.9, 46341.0, 65536.0,
                                                      92682.0, 2147483520.0, -2147483520.0, -1.0, -0.5, 3.0e-39]]).astype(np.float32)
    f = np.concatenate([10.0 ** rng.uniform(-6, 6, len(g) - 8), [0.0, 1e-30, 1e30, np.inf, 1.0, 0.5, 3.4e38, 1e-20]]).astype(np.float32)
    out[8] = np.stack([_bits(f), _bits(g)], axis=1)

    # ---- 9 same_hemisphere / 10 reflect / 11 refract / 12 uniform_sample_sphere
    e9 = [(a, b_, c) for a in ax for b_ in ax for c in ax]
    out[9] = np.concatenate([np.concatenate([_bits(wo), _bits(wi), _bits(nn)], axis=1),
                             np.concatenate([_bits([x[0] for x in e9]), _bits([x[1] for x in e9]), _bits([x[2] for x in e9])], axis=1)])
    e10 = [(a, b_) for a in ax for b_ in ax]
    out[10] = np.concatenate([np.concatenate([_bits(wo), _bits(nn)], axis=1),
                              np.concatenate([_bits([x[0] for x in e10]), _bits([x[1] for x in e10])], axis=1)])
    cos = np.abs(np.einsum("nk,nk->n", wo.astype(np.float64), nn.astype(np.float64))).astype(np.float32)
    eta = rng.choice(_f([1.0, 1 / 1.5, 1.5, 0.8, 1.25, 2.4, 1 / 2.4]), n)
    n11 = np.where((np.einsum("nk,nk->n", wo, nn) > 0)[:, None], -nn, nn)   # the caller's convention: n against wo
    rc = [(_f(w_), _f((0, 0, -1.0)) if w_[2] >= 0 else _f(n_), np.float32(i) if w_[2] >= 0 else np.float32(1.0) / np.float32(i),
           np.float32(abs(w_[2]))) for w_, n_, i in crit]   # as sample_f calls it: n against wo, eta, |cos|
    out[11] = np.concatenate([np.concatenate([_bits(wo), _bits(n11), _bits(eta)[:, None], _bits(cos)[:, None]], axis=1),
                              np.concatenate([_bits([x[0] for x in rc]), _bits([x[1] for x in rc]), _bits([x[2] for x in rc])[:, None],
                                              _bits([x[3] for x in rc])[:, None]], axis=1)])
    out[12] = _raws(rng, 2 * n)

    # ---- 13 get_ray: the frames' cameras with x, y over [0, 1] and the corners
    cams = []
    for lookfrom, lookat, up, vfov in (CAM_FRONT, CAM_LOW, CAM_SIDE, ((0.5, 0.5, 1.5), (0.5, 0.5, 0.0), (0, 1, 0), 37.8)):
        for half_w, half_h in ((0.7, 0.7), (1.1, 0.6), (0.35, 0.5)):   # (any twelve numbers make a Camera for get_ray)
            w_ = _unit(np.subtract(lookfrom, lookat))
            u_ = _unit(np.cross(up, w_))
            v_ = np.cross(w_, u_).astype(np.float32)
            hz, vt = np.float32(2 * half_w) * u_, np.float32(-2 * half_h) * v_
            ul = (_f(lookfrom) - w_ - np.float32(0.5) * hz - np.float32(0.5) * vt).astype(np.float32)
            cams.append(np.concatenate([_f(lookfrom), ul, hz, vt]).astype(np.float32))
    xy = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    xy[:4] = [[0, 0], [1, 1], [0, 1], [1, 0]]
    cam = np.stack([cams[k % len(cams)] for k in range(n)])
    out[13] = np.concatenate([_bits(cam), _bits(xy)], axis=1)

    for k, v in out.items():
        assert v.dtype == np.uint32 and v.shape[1] == WORDS_IN[k], (k, v.shape)
        out[k] = np.ascontiguousarray(v)
    return out


# ------------------------------------------------------------------------------------------------ fixture files
def save_npz(path, arrays):
    """An .npz whose bytes depend on the arrays alone (np.savez stamps each member with the time of day)."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def fixture_frame(npz, name):
    """The arrays of one frame of the render fixture: key -> ndarray."""
    pre = name + "__"
    return {k[len(pre):]: npz[k] for k in npz.files if k.startswith(pre)}
