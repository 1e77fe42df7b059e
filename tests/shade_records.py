"""Scenes and path states for whole shading steps: init() + mat() on the device against the oracle.  TEST HELPER (a plain module).

A record is one path state in the layout of the device's shading probe (22 words: bounces, hit_info, pixel, gen, XORWOW
state 6, beta 3, wo 3, isect_p 3, isect_n 3); rt_shade_records runs the kernels' advance_core on it, Oracle.mat_step the
oracle's mat_step.  Everything here is made of the committed function tables (tests/golden/ref_shade_fixture.npz): the
lights are the rows of the sample_Li table (its triangles are the scenes' triangles), isect_p is that table's p of the light
a record is meant to pick, (material, wo, n) are rows of the sample_f table.

Three scenes:
  small   rows 0 .. 47 of the sample_Li table as lights (the two degenerate triangles, the two shading points that sit ON a
          point light, the 28 rows with p in the triangle's plane) and 12 materials: one of each kind at iors 1.0, 0.8, 1.5
          and 2.4, albedo 0.5 -- the materials of the sample_f table's edge rows.  <= 64 of either: both table builds run.
  large   all 600 lights and 100 materials (those of the sample_f table's edge rows, then of its first random rows): past
          the LDS gate.
  dark    one triangle, no light.

Two ways to a record's XORWOW state:
  stream  a snapshot of a real stream (one long orc_xorwow_draw sequence) at a position whose draw after the record's
          sample_f draws picks the wanted light.  What follows is whatever the stream holds: the sample point on an area
          light, the Schlick draw, the burnt draws of the second sample_f call, the Russian-roulette rolls.
  replay  a state built to make five chosen draws next (replay_state): the sample_f table's two raws, a raw that picks the
          wanted light, the sample_Li table's two raws of that light's row.  A matte hit then computes exactly what the
          committed out_sample_f and out_sample_Li rows hold (its sixth and seventh draw, the burn, are what they are).

Records for init(): bounces 0 on a light-carrying triangle (emission), bounces kRrStart and kRrStart + 1, max3(beta) of
exactly 1.0 and one ulp below, beta small enough for the kill chain to run to max_bounces, bounces max_bounces - 1 and
max_bounces, misses.  Everything is a function of the fixture, constants and numpy's seeded PCG64 streams."""
from __future__ import annotations

import os

import numpy as np

import shade_scenes as ss
from rtcuda_amd import scenes

FIXTURE = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_shade_fixture.npz"))
T1_IN, T1_OUT = FIXTURE["in_sample_f"], FIXTURE["out_sample_f"]
T3_IN, T3_OUT = FIXTURE["in_sample_Li"], FIXTURE["out_sample_Li"]
MAX_BOUNCES = 10
RR_START = 4                        # constant.hpp:10
SMALL_LIGHTS = 48
SMALL_IORS = (1.0, 0.8, 1.5, 2.4)
LARGE_MATERIALS = 100
DEGENERATE_LIGHTS = (0, 1)          # zero-area light triangles
ON_LIGHT_POINTS = (4, 8)            # the shading point IS the point light: wi = 0 / 0, no shadow ray can exist
N_RANDOM_T1 = 600                   # the sample_f table: 600 random rows, then the edge rows
STREAM_SEED, STREAM_DRAWS = 20260118, 1 << 18
# how a record came about
STREAM, REPLAY, INIT = 0, 1, 2

_M32 = 0xFFFFFFFF
_WEYL = 362437


def _f32(words):
    return np.ascontiguousarray(words, np.uint32).view(np.float32)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def replay_state(raws):
    """An XORWOW state {d, v0 .. v4} whose next len(raws) <= 5 draws are exactly `raws`.  shade_scenes.xorwow_state_for fixes
    v4 = 0 and reaches four; the fifth draw's oldest word IS v4, so it is chosen first and the first draw built on it."""
    raws = [int(r) for r in raws]
    if len(raws) <= 4:
        return ss.xorwow_state_for(raws)
    assert len(raws) == 5
    h = lambda y: (y ^ (y << 4)) & _M32
    x = [(r - (k + 1) * _WEYL) & _M32 for k, r in enumerate(raws)]     # the newest word after each draw
    v4 = ss._inv_g(x[4] ^ h(x[3]))
    v = [ss._inv_g(x[0] ^ h(v4))] + [ss._inv_g(x[k] ^ h(x[k - 1])) for k in (1, 2, 3)] + [v4]
    return np.array([0] + v, np.uint32)


def pick_of(raw, num_lights):
    """render.cuh:178 in float32: the light a raw draw picks."""
    u = ss.uniform_of(raw)
    return np.minimum((u * np.float32(num_lights)).astype(np.int64), num_lights - 1)


def raw_picking(light, num_lights):
    """A raw draw that picks `light`: the middle of its interval."""
    raw = int((light + 0.5) / num_lights * (1 << 32))
    assert int(pick_of(raw, num_lights)) == light
    return raw


# ------------------------------------------------------------------------------------------------ scenes
def _materials(rows5):
    m = np.zeros(len(rows5), dtype=scenes.MATERIAL_DTYPE)
    m["albedo"], m["ior"], m["type"] = _f32(rows5[:, 0:3]), _f32(rows5[:, 3]), rows5[:, 4].astype(np.int32)
    return m


def small_material_rows():
    rows = np.zeros((3 * len(SMALL_IORS), 5), np.uint32)
    k = 0
    for kind in (ss.MATTE, ss.MIRROR, ss.GLASS):
        for ior in SMALL_IORS:
            rows[k, 0:3], rows[k, 3], rows[k, 4] = _bits([0.5, 0.5, 0.5]), _bits([ior])[0], kind
            k += 1
    return rows


def large_material_rows():
    """The distinct materials of the sample_f table's edge rows, then of its random rows, up to LARGE_MATERIALS."""
    seen, rows = set(), []
    for k in list(range(N_RANDOM_T1, len(T1_IN))) + list(range(N_RANDOM_T1)):
        key = tuple(T1_IN[k, 0:5].tolist())
        if key not in seen:
            seen.add(key)
            rows.append(T1_IN[k, 0:5])
        if len(rows) == LARGE_MATERIALS:
            break
    return np.array(rows, np.uint32)


def _scene(n_lights, material_rows, name):
    rows = T3_IN[:n_lights]
    ltype = rows[:, 0].astype(np.int32)
    idx = np.arange(n_lights, dtype=np.int32)
    lights = np.zeros(n_lights, dtype=scenes.LIGHT_DTYPE)
    lights["type"], lights["pos"], lights["L"] = ltype, _f32(rows[:, 1:4]), _f32(rows[:, 4:7])
    lights["tri"] = np.where(ltype == scenes.AREA_LIGHT, idx, -1)
    return scenes.SceneArrays(tris=_f32(rows[:, 7:16]).reshape(-1, 9), tri_material=idx % len(material_rows),
                              tri_light=np.where(ltype == scenes.AREA_LIGHT, idx, -1).astype(np.int32),
                              materials=_materials(material_rows), lights=lights, name=name)


def dark_scene():
    return scenes.SceneArrays(tris=_f32(T3_IN[5:6, 7:16]).reshape(-1, 9), tri_material=np.zeros(1, np.int32),
                              tri_light=np.full(1, -1, np.int32), materials=_materials(small_material_rows()),
                              lights=np.zeros(0, dtype=scenes.LIGHT_DTYPE), name="shade_dark")


# ------------------------------------------------------------------------------------------------ records
class _Stream:
    """One long XORWOW sequence and the state at any position of it (the state after s draws is the last five xorshift words:
    raw[k - 1] - d_k for k = s - 4 .. s)."""

    def __init__(self, oracle):
        st = oracle.xorwow_init(STREAM_SEED, 0)
        self.d0 = int(st[0])
        self.raw, _ = oracle.xorwow_draw(st, STREAM_DRAWS)
        k = np.arange(1, STREAM_DRAWS + 1, dtype=np.uint64)
        self.x = ((self.raw.astype(np.uint64) - (np.uint64(self.d0) + k * np.uint64(_WEYL))) & np.uint64(_M32)).astype(np.uint32)
        self._picks = {}
        self._next = {}

    def state(self, s):
        assert 5 <= s < STREAM_DRAWS - 16
        return np.concatenate([[np.uint32((self.d0 + s * _WEYL) & _M32)], self.x[s - 5:s]]).astype(np.uint32)

    def position(self, light, num_lights, draws_before, skip=0):
        """The next unused position s whose draw number draws_before + 1 picks `light` (light < 0: any position)."""
        if light < 0:
            s = self._next.get(None, 5)
            self._next[None] = s + 7
            return s
        if num_lights not in self._picks:
            self._picks[num_lights] = pick_of(self.raw, num_lights)
        key = (num_lights, light, draws_before)
        if key not in self._next:
            p = np.flatnonzero(self._picks[num_lights] == light) - draws_before
            self._next[key] = [p[(p >= 5) & (p < STREAM_DRAWS - 16)], 0]
        cand, used = self._next[key]
        assert used + skip < len(cand), ("the stream never picks light", light, num_lights)
        self._next[key][1] = used + skip + 1
        return int(cand[used + skip])


class Records:
    def __init__(self, name, arrays, max_bounces=MAX_BOUNCES):
        self.name, self.arrays, self.max_bounces = name, arrays, max_bounces
        self.rows, self.meta = [], []

    def add(self, how, bounces, hit_info, state, beta, wo, p, n, light=-1, t1_row=-1, purpose=""):
        row = np.zeros(22, np.uint32)
        row[0], row[1], row[2], row[3] = np.uint32(bounces), np.uint32(hit_info & _M32), len(self.rows), 0
        row[4:10] = state
        row[10:13], row[13:16], row[16:19], row[19:22] = _bits(beta), _bits(wo), _bits(p), _bits(n)
        self.rows.append(row)
        self.meta.append((how, light, t1_row, purpose))

    def finish(self):
        self.records = np.array(self.rows, np.uint32).reshape(-1, 22)
        self.how = np.array([m[0] for m in self.meta], np.int32)
        self.light = np.array([m[1] for m in self.meta], np.int32)       # the light the record is meant to pick, or -1
        self.t1_row = np.array([m[2] for m in self.meta], np.int32)      # its row of the sample_f table, or -1
        self.purpose = np.array([m[3] for m in self.meta])
        assert len(self.records) <= 4096
        return self


def _material_index(material_rows):
    """sample_f-table row -> index of ITS material in the scene's table, or -1."""
    table = {tuple(r.tolist()): k for k, r in enumerate(material_rows)}
    return np.array([table.get(tuple(T1_IN[k, 0:5].tolist()), -1) for k in range(len(T1_IN))], np.int32)


def _same_kind_index(material_rows):
    """sample_f-table row -> a material of the row's kind (iors in rotation) where the row's own is not in the table."""
    own = _material_index(material_rows)
    kinds = material_rows[:, 4]
    out = own.copy()
    for k in np.flatnonzero(own < 0):
        pool = np.flatnonzero(kinds == T1_IN[k, 4])
        out[k] = pool[k % len(pool)]
    return out


def _accepting_rows(wi, rows):
    """The matte rows of `rows` (sample_f table) whose (wo, n) make get_f accept wi: wo and wi on opposite sides of n."""
    wo, n = _f32(T1_IN[rows, 5:8]).astype(np.float64), _f32(T1_IN[rows, 8:11]).astype(np.float64)
    prod = np.einsum("nk,nk->n", wo, n) * (n @ np.asarray(wi, np.float64))
    return rows[(T1_IN[rows, 4] == ss.MATTE) & (prod < -1e-3)]


def build(oracle):
    """-> {"small": Records, "large": Records, "dark": Records}"""
    rng = np.random.default_rng(20260118)
    stream = _Stream(oracle)
    out = {}
    for name, n_lights, material_rows in (("small", SMALL_LIGHTS, small_material_rows()), ("large", len(T3_IN), large_material_rows())):
        R = Records(name, _scene(n_lights, material_rows, "shade_" + name))
        own = _material_index(material_rows)
        mat_of = _same_kind_index(material_rows) if name == "small" else own
        usable = np.flatnonzero(mat_of >= 0)
        matte = usable[T1_IN[usable, 4] == ss.MATTE]
        exact_matte = matte[own[matte] >= 0]
        other = usable[T1_IN[usable, 4] != ss.MATTE]
        centre = _f32(T3_IN[:, 7:16]).reshape(-1, 3, 3).astype(np.float64).mean(axis=1)

        def beta():
            return rng.uniform(0.05, 1.0, 3).astype(np.float32)

        def row_fields(k, R=R, mat_of=mat_of, own=own):
            """material index, wo, n and the draws sample_f consumes there (the table's own count where the material is the
            row's own; otherwise -- glass of another index may or may not refract -- the oracle's sample_f says)."""
            m, wo, n = int(mat_of[k]), _f32(T1_IN[k, 5:8]), _f32(T1_IN[k, 8:11])
            if own[k] >= 0:
                return m, wo, n, int(T1_OUT[k, 10])
            st = np.zeros(6, np.uint32)
            oracle.sample_f(R.arrays.materials[m:m + 1], wo, n, st)
            return m, wo, n, int((int(st[0]) * pow(_WEYL, -1, 1 << 32)) & _M32)

        for L in range(n_lights):
            p = _f32(T3_IN[L, 16:19])
            area = T3_IN[L, 0] == scenes.AREA_LIGHT
            wi_ref = _f32(T3_OUT[L, 1:4]).astype(np.float64)
            # ---- replay: a matte hit that computes the committed sample_f and sample_Li rows (the shadow ray exists
            # wherever one can: never at an on-light point, whose wi is NaN)
            acc = _accepting_rows(wi_ref, exact_matte) if np.isfinite(wi_ref).all() else exact_matte[:0]
            k = int(acc[L % len(acc)]) if len(acc) else int(exact_matte[L % len(exact_matte)])
            m, wo, n, _ = row_fields(k)
            st = replay_state([T1_IN[k, 11], T1_IN[k, 12], raw_picking(L, n_lights), T3_IN[L, 19], T3_IN[L, 20]])
            R.add(REPLAY, 1 + L % 3, m, st, beta(), wo, p, n, light=L, t1_row=k, purpose="replay")
            # ---- stream: a matte hit aimed so that the shadow ray exists for a sample point near the triangle's centre
            # (a point light: for its position), and a mirror or glass hit
            aim = (centre[L] if area else _f32(T3_IN[L, 1:4]).astype(np.float64)) - p.astype(np.float64)
            acc = _accepting_rows(aim, matte) if np.isfinite(aim).all() and np.any(aim != 0) else matte[:0]
            for j in range(3 if name == "small" else 1):
                k = int(acc[(L + 7 * j) % len(acc)]) if len(acc) else int(matte[(L + 7 * j) % len(matte)])
                m, wo, n, draws = row_fields(k)
                R.add(STREAM, 1 + (L + j) % 3, m, stream.state(stream.position(L, n_lights, draws)), beta(), wo, p, n, light=L,
                      t1_row=k, purpose="stream_matte")
            for j in range(2 if name == "small" else 1):
                k = int(other[(5 * L + j) % len(other)])
                m, wo, n, draws = row_fields(k)
                R.add(STREAM, 1 + (L + j) % 3, m, stream.state(stream.position(L, n_lights, draws)), beta(), wo, p, n, light=L,
                      t1_row=k, purpose="stream_specular")
        # ---- every usable edge row of the sample_f table (dot(wo, n) of 0 and +-1, the critical angle, ior 1), lights in rotation
        edge = usable[usable >= N_RANDOM_T1]
        for j, k in enumerate(edge):
            L = j % n_lights
            m, wo, n, draws = row_fields(int(k))
            R.add(STREAM, 1 + j % 4, m, stream.state(stream.position(L, n_lights, draws)), beta(), wo, _f32(T3_IN[L, 16:19]), n,
                  light=L, t1_row=int(k), purpose="edge_row")
        # ---- init()
        lit = np.flatnonzero(T3_IN[:n_lights, 0] == scenes.AREA_LIGHT)
        one, below = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(0.0))

        def init_record(purpose, bounces, b3, j, light_of_hit=-1, miss=False):
            k = int(usable[(11 * j + 3) % len(usable)])
            L = (5 * j + 1) % n_lights
            m, wo, n, _ = row_fields(k)
            hit_info = -1 if miss else (m | ((light_of_hit + 1) << 16))
            R.add(INIT, bounces, hit_info, stream.state(stream.position(-1, n_lights, 0)), np.asarray(b3, np.float32), wo,
                  _f32(T3_IN[L, 16:19]), n, t1_row=k, purpose=purpose)

        for j in range(24):
            init_record("emission", 0, [1, 1, 1], j, light_of_hit=int(lit[j % len(lit)]))
            init_record("no_emission_bounce_1", 1, beta(), j, light_of_hit=int(lit[j % len(lit)]))
            init_record("rr_start", RR_START, [0.3, 0.2, 0.1], j)                  # bounces > kRrStart is false: no roulette
            init_record("rr_start_plus_1", RR_START + 1, [0.3, 0.2, 0.1], j)
            init_record("beta_one", RR_START + 1 + j % 4, [0.5, one, 0.25], j)     # max3(beta) < 1 is false: no roulette
            init_record("beta_below_one", RR_START + 1 + j % 4, [0.5, below, 0.25], j)   # pt = max(0.05, 2^-24) = 0.05
            init_record("last_bounce", MAX_BOUNCES - 1, [1, 1, 1], j)
            init_record("last_bounce_rr", MAX_BOUNCES - 1, [0.5, 0.4, 0.3], j)
            init_record("no_bounce_left", MAX_BOUNCES, beta(), j, light_of_hit=int(lit[j % len(lit)]))
            init_record("miss", j % MAX_BOUNCES, beta(), j, miss=True)
        for j in range(96):   # kill chains of every length: pt 0.5, 0.7, 0.9 and 0.999 from every bounce count past kRrStart
            b = [0.5, 0.3, 0.1, 0.001][j % 4]
            init_record("rr_chain", RR_START + 1 + (j // 4) % (MAX_BOUNCES - RR_START - 1), [b, 0.5 * b, 0.25 * b], j)
        out[name] = R.finish()
    # ---- no light at all: mat() ends after the beta update
    R = Records("dark", dark_scene())
    rows = np.concatenate([np.arange(0, 60), np.arange(N_RANDOM_T1, len(T1_IN), 7)])
    mat_of = _same_kind_index(small_material_rows())
    for j, k in enumerate(rows):
        R.add(STREAM, j % 6, int(mat_of[k]), stream.state(stream.position(-1, 0, 0)), rng.uniform(0.05, 1.0, 3).astype(np.float32),
              _f32(T1_IN[k, 5:8]), _f32(T3_IN[j % len(T3_IN), 16:19]), _f32(T1_IN[k, 8:11]), t1_row=int(k), purpose="dark")
    out["dark"] = R.finish()
    return out
