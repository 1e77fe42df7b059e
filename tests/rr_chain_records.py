"""Path states for the Russian-roulette chain of init(): every chain length at every limit.  TEST HELPER (a plain module).

A record is a path state in the layout of tests/shade_records.py (22 words), on that module's `small` scene.  init() rolls
a path with bounces > kRrStart and max3(beta) < 1 once per call until it survives or bounces reaches max_bounces; the device
runs the whole chain inside one ADV block, as one loop whose limit L = max_bounces - bounces is known before it.

For max_bounces 10, 7 and 6 (a Records each: max_bounces is a property of the call), every entry `bounces` from kRrStart + 1
to max_bounces - 1, so L = 1 .. 5; for every L and every k = 1 .. L a record with k - 1 kills and then a survivor, and one
with L kills.  The rolls are the record's next draws (shade_records.replay_state: up to five chosen raws); what a survivor's
mat() draws behind them is whatever the state holds then.

pt = max(0.05, 1 - max3(beta)) at the floor (max3(beta) 0.95 and 0.999), mid-range (0.5) and high (max3(beta) 1e-3).  The
draws sit at the comparison's edge -- a kill is the largest raw whose uniform is below pt, a survivor the smallest raw whose
uniform is not below pt (`at`: where a raw's uniform EQUALS pt, this is one; it survives) or the smallest whose uniform is
above pt (`above`) -- or anywhere on their side (`far`: numpy's seeded stream).

Fillers, for which no chain runs: max3(beta) exactly 1.0, bounces == kRrStart, bounces == max_bounces, misses.

Every Records is laid out in waves of 64 consecutive records (the shading probe runs record i on lane i % 64): the chains
and fillers shuffled together, matte and specular hits alternating, so that a wave holds every chain length side by side;
then, for max_bounces 10, a wave in which all 64 lanes make five rolls and one in which exactly one lane does.

`expect` of a Records: (rolls, shaded) per record, as the builder means them; tests/test_rr_chain_records_host.py holds them
to Oracle.mat_step."""
from __future__ import annotations

import numpy as np

import shade_records as sr
import shade_scenes as ss

MAX_BOUNCES = (10, 7, 6)
BETA_MAX = (0.95, 0.999, 0.5, 1e-3)
WAVE = 64


def pt_of(beta3):
    """render.cuh:113 in float32."""
    return max(np.float32(0.05), np.float32(1.0) - np.float32(max(beta3)))


def _first_raw(pred):
    """The smallest raw draw whose uniform satisfies `pred` (monotone: false below, true from some raw on)."""
    lo, hi = 0, 0xFFFFFFFF
    assert pred(ss.uniform_of(hi)) and not pred(ss.uniform_of(lo))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(ss.uniform_of(mid)):
            hi = mid
        else:
            lo = mid
    return hi


_edges = {}


def edge_raws(pt):
    """(below, at, above): the largest raw that is killed, the smallest that survives, the smallest whose uniform is past pt."""
    if float(pt) not in _edges:
        _edges[float(pt)] = _edge_raws(pt)
    return _edges[float(pt)]


def _edge_raws(pt):
    at = _first_raw(lambda u: u >= pt)
    above = _first_raw(lambda u: u > pt)
    assert ss.uniform_of(at - 1) < pt <= ss.uniform_of(at) and ss.uniform_of(above) > pt
    return at - 1, at, above


def build():
    """-> {max_bounces: Records with .expect (n, 2) int32 = (rolls, shaded) and .batch (n,) names of the special waves}"""
    arrays = sr._scene(sr.SMALL_LIGHTS, sr.small_material_rows(), "shade_small")
    mat_of = sr._same_kind_index(sr.small_material_rows())
    usable = np.flatnonzero(mat_of >= 0)
    matte = usable[sr.T1_IN[usable, 4] == ss.MATTE]
    specular = usable[sr.T1_IN[usable, 4] != ss.MATTE]
    out = {}
    for M in MAX_BOUNCES:
        rng = np.random.default_rng(20261021 + M)
        counter = [0]

        def hit(miss=False):
            """(hit_info, wo, p, n) of the next record: matte and specular rows of the sample_f table alternating."""
            j = counter[0]
            counter[0] += 1
            pool = matte if j % 2 == 0 else specular
            k = int(pool[(7 * j + 3) % len(pool)])
            L = (5 * j + 1) % sr.SMALL_LIGHTS
            return (-1 if miss else int(mat_of[k])), sr._f32(sr.T1_IN[k, 5:8]), sr._f32(sr.T3_IN[L, 16:19]), sr._f32(sr.T1_IN[k, 8:11])

        def beta3(bmax, j):
            b = [np.float32(bmax), np.float32(0.5 * bmax), np.float32(0.25 * bmax)]
            return b[j % 3:] + b[:j % 3]          # the largest component in every place

        def chain(bounces, k_survive, bmax, where, j):
            """k_survive - 1 kills and a survivor, or (k_survive None) kills to the end."""
            L = M - bounces
            beta = beta3(bmax, j)
            pt = pt_of(beta)
            below, at, above = edge_raws(pt)
            if where == "far":
                kill = lambda: int(rng.integers(0, below + 1))
                live = int(rng.integers(above, 1 << 32))
            else:
                kill = lambda: below
                live = at if where == "at" else above
            raws = [kill() for _ in range(L)] if k_survive is None else [kill() for _ in range(k_survive - 1)] + [live]
            raws += [int(r) for r in rng.integers(0, 1 << 32, 5 - len(raws))]     # what mat() draws first
            expect = (L, 0) if k_survive is None else (k_survive, 1)
            return ("chain", bounces, beta, sr.replay_state(raws), expect, False)

        def filler(kind, j):
            st = sr.replay_state([int(r) for r in rng.integers(0, 1 << 32, 5)])
            if kind == "beta_one":          # max3(beta) < 1 is false: one init(), a shade
                return (kind, sr.RR_START + 1 + j % max(M - sr.RR_START - 1, 1), beta3(1.0, j), st, (1, 1), False)
            if kind == "rr_start":          # bounces > kRrStart is false
                return (kind, sr.RR_START, beta3(0.3, j), st, (1, 1), False)
            if kind == "no_bounce_left":
                return (kind, M, beta3(0.3, j), st, (0, 0), False)
            return (kind, j % M, beta3(0.3, j), st, (0, 0), True)       # a miss

        pool, j = [], 0
        for bounces in range(sr.RR_START + 1, M):
            L = M - bounces
            for bmax in BETA_MAX:
                for k in range(1, L + 1):
                    for where in ("at", "above", "far"):
                        for _ in range(4):      # (the largest component of beta in every place; matte and specular hits)
                            pool.append(chain(bounces, k, bmax, where, j))
                            j += 1
                for where in ("edge", "far"):
                    for _ in range(4):
                        pool.append(chain(bounces, None, bmax, where, j))
                        j += 1
        n_chain = len(pool)
        for j in range(max(n_chain // 3, 32)):
            pool.append(filler(("beta_one", "rr_start", "no_bounce_left", "miss")[j % 4], j))
        order = rng.permutation(len(pool))
        rows = [pool[i] + ("mixed",) for i in order]
        while len(rows) % WAVE:
            rows.append(filler(("miss", "no_bounce_left")[len(rows) % 2], len(rows)) + ("mixed",))
        if M == 10:
            b5 = sr.RR_START + 1
            # all 64 lanes roll five times: survivors of the fifth roll and paths killed to the end, side by side
            for j in range(WAVE):
                rows.append(chain(b5, 5 if j % 3 else None, BETA_MAX[j % 4], ("at", "above", "far", "at")[j % 4] if j % 3 else ("edge", "far")[j % 2], j)
                            + ("all_five",))
            # exactly one lane rolls five times; no other lane rolls at all
            for j in range(WAVE):
                if j == 37:
                    rows.append(chain(b5, None, 0.5, "edge", j) + ("one_five",))
                else:
                    rows.append(filler(("beta_one", "rr_start", "no_bounce_left", "miss")[j % 4], j) + ("one_five",))
        R = sr.Records(f"rr_chain_{M}", arrays, max_bounces=M)
        for kind, bounces, beta, st, expect, miss, batch in rows:
            hit_info, wo, p, n = hit(miss)
            R.add(sr.INIT, bounces, hit_info, st, beta, wo, p, n, purpose=kind)
        R.finish()
        R.expect = np.array([r[4] for r in rows], np.int32)
        R.batch = np.array([r[6] for r in rows])
        assert len(R.records) % WAVE == 0
        out[M] = R
    return out
