"""What a followed AOV frame must hold (rt_render_aov_follow_fixed / rt_render_aov_follow_rays_fixed_device, DESIGN.md section
2.11), from numpy and the oracle alone.  Rays and streams: raytable_keyed (held to the oracle by
tests/test_render_rays_keyed_host.py).  Hits: OracleScene.trace_closest in the hit mode wanted.  The step at a specular vertex:
Oracle.mat_step -- the code the oracle's per-sample frame runs between two traversals -- on a record laid out as
tests/shade_records.py lays them out: it returns the next ray, beta and the stream behind every draw mat() makes there, so the
draw skipping is not restated here at all.  The hit point p(u, v) = (p0 - e1 * u) + e2 * v is restated in float32 on
Oracle.triangle's record.  to_fixed, deposit and shading_normals are aov_expected's.  tests/test_aov_follow_host.py holds this
file to the oracle's own per-sample frame, ray for ray, before any GPU test leans on it."""
import dataclasses

import numpy as np

import aov_expected as ae
import raytable
import raytable_keyed as rk
from rtcuda_amd import scenes

F32 = np.float32
FOLLOW_MAX = 5
DIFFUSE, CAP, MISS, NOTHING = 0, 1, 2, 3          # how a chain ended (NOTHING: the first ray missed)
REFLECT, REFRACT, CANNOT_REFRACT = 0, 1, 2        # what a glass step did
_WEYL_INV = pow(362437, -1, 1 << 32)

_tri_cache = {}


def _tri_records(oracle, arrays, tri_ids):
    """Oracle.triangle's {p0, e1, e2, n} of the triangles `tri_ids` -> (k, 12) float32."""
    cache = _tri_cache.setdefault(id(arrays), {})
    tris = np.asarray(arrays.tris, np.float32).reshape(-1, 9)
    out = np.zeros((len(tri_ids), 12), np.float32)
    for k, t in enumerate(np.asarray(tri_ids).tolist()):
        if t not in cache:
            cache[t] = oracle.triangle(tris[t])[0].astype(np.float32)
        out[k] = cache[t]
    return out


def _dot(a, b):
    return ((a[:, 0] * b[:, 0]).astype(F32) + (a[:, 1] * b[:, 1]).astype(F32) + (a[:, 2] * b[:, 2]).astype(F32)).astype(F32)


def sample_streams(oracle, seed, keys):
    """The streams of the samples `keys` behind their two jitter draws -> (n, 6) uint32."""
    with np.errstate(over="ignore"):
        st = rk.stream_states(oracle, seed, keys)
        raytable._xorwow_next(st)
        raytable._xorwow_next(st)
    return st


def follow(oracle, osc, o, d, states, max_specular, census=True):
    """The chains of the samples whose first rays are (o, d) and whose streams stand at `states` -> a dict of per-sample arrays:
    tri0, mat0 (first hit, caller's order; -1), vals (n, 10) float32 to deposit, dep (bool: deposits at all), hit (0 / 1: what
    it adds to the hit count), length (specular steps taken), ending, and `rays`: per sample the list of (o, d, tri, t) of every
    ray traced, `steps`: per sample the list of glass branches / -1 for a mirror step, and end_words / end_flags: Oracle.mat_step's
    output on the vertex a chain ends on, run with max_bounces = that vertex's bounce count + 1.  census=False (large frames):
    `rays`, `steps` and the end words are left empty."""
    assert 0 <= max_specular <= FOLLOW_MAX
    arrays = osc.arrays
    n = len(o)
    o, d = np.array(o, np.float32), np.array(d, np.float32)
    st = np.array(states, np.uint32)
    beta = np.ones((n, 3), np.float32)
    path = np.zeros(n, np.float32)
    tri0, mat0 = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    light0 = np.full(n, -1, np.int32)
    vals = np.zeros((n, 10), np.float32)
    hit = np.zeros(n, np.int32)
    length = np.zeros(n, np.int32)
    ending = np.full(n, NOTHING, np.int32)
    rays, steps = [[] for _ in range(n)], [[] for _ in range(n)]
    end_words, end_flags = np.zeros((n, 27), np.uint32), np.zeros(n, np.uint32)
    tri_material, tri_light = np.asarray(arrays.tri_material, np.int32), np.asarray(arrays.tri_light, np.int32)
    live = np.arange(n)
    for j in range(max_specular + 1):
        if live.size == 0:
            break
        tri, t, u, v = osc.trace_closest(o[live], d[live], np.full(live.size, ae.FLT_MAX, np.float32))
        for a, s in enumerate(live.tolist() if census else ()):
            rays[s].append((o[s].copy(), d[s].copy(), int(tri[a]), F32(t[a])))
        missed = tri < 0
        if j > 0:
            ending[live[missed]] = MISS
        live, tri, t, u, v = live[~missed], tri[~missed], t[~missed], u[~missed], v[~missed]
        mat = tri_material[tri]
        if j == 0:
            tri0[live], mat0[live], light0[live] = tri, mat, tri_light[tri]
        path[live] = (path[live] + t).astype(F32)
        nn = ae.shading_normals(oracle, arrays, tri)
        go = (arrays.materials["type"][mat] != scenes.MATTE) & (j < max_specular)
        # ---- the chains that end on this vertex
        e = live[~go]
        m_e, n_e, d_e = mat[~go], nn[~go], d[e]
        vals[e, ae.ALBEDO:ae.ALBEDO + 3] = (beta[e] * arrays.materials["albedo"][m_e]).astype(F32)
        vals[e, ae.NORMAL:ae.NORMAL + 3] = np.where((_dot(n_e, d_e) > 0)[:, None], -n_e, n_e)
        vals[e, ae.DEPTH] = path[e]
        hit[e] = 1
        ending[e] = np.where(arrays.materials["type"][m_e] == scenes.MATTE, DIFFUSE, CAP)
        # ---- mat() at the others
        def records(sel):
            rec = _tri_records(oracle, arrays, tri[sel])
            uu, vv = u[sel][:, None], v[sel][:, None]
            p = ((rec[:, 0:3] - (rec[:, 3:6] * uu).astype(F32)).astype(F32) + (rec[:, 6:9] * vv).astype(F32)).astype(F32)
            rows = np.zeros((int(sel.sum()), 22), np.uint32)
            rows[:, 0] = j
            rows[:, 1] = (mat[sel] | ((tri_light[tri[sel]] + 1) << 16)).astype(np.uint32)
            rows[:, 4:10] = st[live[sel]]
            rows[:, 10:13], rows[:, 13:16] = beta[live[sel]].view(np.uint32), d[live[sel]].view(np.uint32)
            rows[:, 16:19], rows[:, 19:22] = p.view(np.uint32), np.ascontiguousarray(nn[sel]).view(np.uint32)
            return rows

        if e.size and census:  # (what the estimator would do on the vertex the chain ends on: test_aov_follow_host.py's tie to the beauty frame)
            end_words[e], _, end_flags[e] = oracle.mat_step(osc, records(~go), j + 1)
        g = live[go]
        if g.size:
            words, _, flags = oracle.mat_step(osc, records(go), 10)
            assert (flags & 1).all()  # (no Russian roulette below bounce 5: every step shades)
            assert (words[:, 26] == j + 1).all()
            wi = words[:, 3:6].copy().view(np.float32)
            for a, s in enumerate(g.tolist() if census else ()):
                m = int(mat[go][a])
                if arrays.materials["type"][m] == scenes.GLASS:
                    probe = np.zeros(6, np.uint32)
                    oracle.sample_f(arrays.materials[m:m + 1], d[s], nn[go][a], probe)
                    draws = (int(probe[0]) * _WEYL_INV) & 0xFFFFFFFF
                    back = float(np.dot(wi[a].astype(np.float64), nn[go][a])) * float(np.dot(d[s].astype(np.float64), nn[go][a])) < 0
                    steps[s].append(CANNOT_REFRACT if draws == 0 else REFLECT if back else REFRACT)
                else:
                    steps[s].append(-1)
            o[g], d[g] = words[:, 0:3].copy().view(np.float32), wi
            beta[g] = words[:, 17:20].copy().view(np.float32)
            st[g] = words[:, 20:26]
            length[g] = j + 1
        live = g
    lit = light0 >= 0
    if len(arrays.lights):
        vals[lit, ae.EMISSION:ae.EMISSION + 3] = arrays.lights["L"][light0[lit]]
    dep = (hit == 1) | ((ending == MISS) & lit)
    return dict(tri0=tri0, mat0=mat0, vals=vals, dep=dep, hit=hit, length=length, ending=ending, rays=rays, steps=steps,
                end_words=end_words, end_flags=end_flags)


def deposit(chains, pixel, n_pixels):
    """The int64 sums (n_pixels, 11): aov_expected.deposit on the samples that deposit, the hit count from `hit`."""
    dep = chains["dep"]
    sums = ae.deposit(np.where(dep, 0, -1), chains["vals"], pixel, n_pixels)
    sums[:, ae.HITS] = np.bincount(np.asarray(pixel)[chains["hit"] == 1], minlength=n_pixels)
    return sums


def table_expected(oracle, osc, o, d, pixel, n_pixels, keys, max_specular, seed=1, first=None, census=True):
    """(sums, ids, chains) of a table whose row c has the key keys[c] and lands on pixel[c]; `first` as aov_expected's."""
    chains = follow(oracle, osc, o, d, sample_streams(oracle, seed, keys), max_specular, census)
    ids = np.full((n_pixels, 2), -7, np.int32)
    if first is not None:
        f = np.asarray(first, bool)
        ids[np.asarray(pixel)[f], 0] = chains["tri0"][f]
        ids[np.asarray(pixel)[f], 1] = chains["mat0"][f]
    return deposit(chains, pixel, n_pixels), ids, chains


def frame_expected(oracle, osc, cam12, w, h, spp, max_specular, seed=1, shard=(0, 1), census=True):
    """(sums, ids, chains, (pixel, keys)) of shard (r, R) of the camera's followed frame."""
    r, R = shard
    keys = np.arange(r, w * h * spp, R, dtype=np.int64)
    o, d, pixel = rk.keyed_pinhole_table(oracle, cam12, w, h, spp, seed, keys.tolist())
    sums, ids, chains = table_expected(oracle, osc, o, d, pixel, w * h, keys.tolist(), max_specular, seed, first=keys % spp == 0, census=census)
    return sums, ids, chains, (pixel, keys)


def chain_census(chains, pixel=None):
    """Counts over the samples: specular first hits, chains per length and per ending, glass steps per branch, and (with
    `pixel`) the pixels whose depositing samples end with different chain lengths."""
    steps = [b for s in chains["steps"] for b in s if b >= 0]
    out = dict(samples=len(chains["length"]), specular_first=int((chains["length"] > 0).sum()),
               glass_samples=sum(1 for s in chains["steps"] if any(b >= 0 for b in s)),
               lengths={k: int((chains["length"] == k).sum()) for k in range(FOLLOW_MAX + 1)},
               endings={k: int((chains["ending"] == k).sum()) for k in (DIFFUSE, CAP, MISS, NOTHING)},
               branches={k: steps.count(k) for k in (REFLECT, REFRACT, CANNOT_REFRACT)})
    if pixel is not None:
        lo, hi = {}, {}
        for p, k, e in zip(np.asarray(pixel).tolist(), chains["length"].tolist(), chains["ending"].tolist()):
            if e != NOTHING:
                lo[p], hi[p] = min(lo.get(p, k), k), max(hi.get(p, k), k)
        out["mixed_pixels"] = sum(1 for p in lo if lo[p] != hi[p])
    return out


# ---- the frames the CPU test and the GPU tests share
# A close view of the glass bunny in front of the mirror wall: nearly every sample re-arms, most of them more than once.
CLOSE_VIEW = dict(lookfrom=(0.5, 0.45, 0.9), lookat=(0.5, 0.3, 0.0), up=(0.0, 1.0, 0.0), vfov=25.0)
SMALL_FRAMES = ((1, 1, 3), (3, 2, 65), (4, 3, 64))


def close_camera(make_camera, aspect):
    v = CLOSE_VIEW
    return make_camera(v["lookfrom"], v["lookat"], v["up"], v["vfov"], aspect)


# The light-dependent skip: the bare box of full_bsdf (its back wall a mirror) with the two triangles of the left wall made glass, under
# three light sets.  BOX_VIEW looks from inside the box into the corner of the glass wall and the mirror: half of the samples take a
# glass step, one in eight takes it BEHIND the mirror -- where the branch it takes depends on what the mirror vertex drew.
BOX_VIEW = dict(lookfrom=(0.9, 0.5, -0.3), lookat=(0.0, 0.45, -1.0), up=(0.0, 1.0, 0.0), vfov=70.0)
BOX_FRAME = (16, 12, 8)  # (at 2 spp the three light sets give one and the same frame: too few Schlick draws sit behind a skip)
BOX_LIGHTS = ("none", "point", "mixed")


def box_camera(make_camera, aspect):
    v = BOX_VIEW
    return make_camera(v["lookfrom"], v["lookat"], v["up"], v["vfov"], aspect)


def box_scene(which):
    """(arrays of the box as created, the material table and (lights, tri_light) of light set `which`): the GPU test creates the
    scene from the first and edits it with set_materials / set_lights; the helper's arrays are box_arrays(which).  The red
    material becomes glass: the two triangles of the left wall."""
    base = scenes.cornell_bunny("full_bsdf", bunny=False)
    materials = base.materials.copy()
    materials[0] = materials[np.flatnonzero(base.materials["type"] == scenes.GLASS)[0]]
    assert int((np.asarray(base.tri_material) == 0).sum()) == 2
    point = np.zeros(1, dtype=scenes.LIGHT_DTYPE)
    point["type"], point["pos"], point["tri"], point["L"] = scenes.POINT_LIGHT, (0.5, 0.8, 0.5), -1, (0.3, 0.3, 0.3)
    dark = np.full(len(base.tri_material), -1, np.int32)
    lights, tri_light = {"none": (base.lights[:0].copy(), dark), "point": (point, dark),
                         "mixed": (np.concatenate([base.lights, point]), np.array(base.tri_light, np.int32))}[which]
    return base, materials, lights, tri_light


def box_arrays(which):
    base, materials, lights, tri_light = box_scene(which)
    return dataclasses.replace(base, materials=materials, tri_light=tri_light, lights=lights)
