"""The shading records reach what they are there for -- asserted from the oracle alone.  CPU only.

tests/shade_records.py builds the path states that tests/test_gpu_shade_records.py runs through the kernels' advance_core.
A record that does not pick the light it is meant to pick, or a roulette chain that never runs to max_bounces, would leave
the GPU comparison green and empty; this file holds the records to their purposes with Oracle.mat_step, the oracle's
generator and the oracle's sample_f.

One thing the records cannot reach, by arithmetic and not for want of searching: a shadow ray towards a point light the
shading point sits ON (rows 4 and 8 of the sample_Li table).  There wi = 0 * (1 / 0) is NaN, same_hemisphere compares a NaN
and get_f rejects.  Those two lights are picked, and the test asserts that no record picking them has a shadow ray; every
other light of the small scene is picked by a record that has one."""
import numpy as np
import pytest

import shade_records as sr
import shade_scenes as ss

WEYL_INV = pow(362437, -1, 1 << 32)


@pytest.fixture(scope="module")
def built(oracle):
    recs = sr.build(oracle)
    out = {}
    for name, R in recs.items():
        sc = oracle.scene(R.arrays)
        words, emission, flags = oracle.mat_step(sc, R.records, R.max_bounces)
        out[name] = (R, words, emission, flags)
    return out


def _draws(d_in, d_out):
    return ((d_out.astype(np.uint64) - d_in.astype(np.uint64)) * np.uint64(WEYL_INV)) & np.uint64(0xFFFFFFFF)


def test_replay_state_replays_five_draws_and_agrees_with_the_four_draw_form(oracle):
    rng = np.random.default_rng(5)
    for raws in [[0, 0xFFFFFFFF, 1, 0x80000000, 0x7FFFFFFF]] + rng.integers(0, 1 << 32, (20, 5)).tolist():
        got, _ = oracle.xorwow_draw(sr.replay_state(raws).copy(), 5)
        assert got.tolist() == raws
    assert sr.replay_state([7, 8]).tolist() == ss.xorwow_state_for([7, 8]).tolist()
    r2 = rng.integers(0, 1 << 32, (50, 2), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(ss.xorwow_states_for2(r2), np.stack([ss.xorwow_state_for(x) for x in r2]))


def test_stream_snapshots_are_states_of_the_stream(oracle):
    s = sr._Stream(oracle)
    for pos in (5, 6, 1000, 77777):
        got, _ = oracle.xorwow_draw(s.state(pos).copy(), 8)
        assert np.array_equal(got, s.raw[pos:pos + 8])


def test_scene_sizes(built):
    small, large, dark = (built[k][0].arrays for k in ("small", "large", "dark"))
    assert len(small.lights) == 48 and len(small.materials) == 12 and len(small.tris) == 48
    assert len(large.lights) == 600 and len(large.materials) == 100
    assert len(dark.lights) == 0 and len(dark.tris) == 1
    for name in built:
        assert 50 <= len(built[name][0].records) <= 4096
        assert np.array_equal(built[name][0].records[:, 2], np.arange(len(built[name][0].records)))   # a pixel each


@pytest.mark.parametrize("name", ["small", "large"])
def test_records_pick_the_light_they_are_meant_to(oracle, built, name):
    """The pick draw, made by the oracle's generator from the record's state after the draws the oracle's sample_f consumes."""
    R, words, _, flags = built[name]
    n_lights = len(R.arrays.lights)
    aimed = np.flatnonzero(R.light >= 0)
    assert len(aimed) > 5 * 48
    for i in aimed:
        st = R.records[i, 4:10].copy()
        m = R.arrays.materials[int(R.records[i, 1]) & 0xFFFF:][:1]
        oracle.sample_f(m, sr._f32(R.records[i, 13:16]), sr._f32(R.records[i, 19:22]), st)
        raw, _ = oracle.xorwow_draw(st, 1)
        assert int(sr.pick_of(raw[0], n_lights)) == R.light[i], (i, R.purpose[i])
    shadow = (flags & 2) != 0
    with_shadow = set(R.light[aimed][shadow[aimed]].tolist())
    picked = set(R.light[aimed].tolist())
    assert picked == set(range(n_lights))
    for L in sr.DEGENERATE_LIGHTS:
        assert L in with_shadow
    on_light = np.isin(R.light, sr.ON_LIGHT_POINTS)
    assert on_light.sum() >= 2 * len(sr.ON_LIGHT_POINTS) and not shadow[on_light].any()
    if name == "small":
        assert with_shadow == set(range(n_lights)) - set(sr.ON_LIGHT_POINTS)
    else:
        assert len(with_shadow) >= 0.9 * n_lights
    # the excluded triangle of a shadow ray is the picked area light's, and a replayed matte hit on a light has a shadow ray
    area = R.arrays.lights["type"][np.maximum(R.light, 0)] == 1
    sel = aimed[shadow[aimed]]
    assert np.array_equal(words[sel, 16].view(np.int32), np.where(area[sel], R.light[sel], -1))
    replay = (R.how == sr.REPLAY) & ~on_light
    assert shadow[replay].mean() > 0.95


@pytest.mark.parametrize("name", ["small", "large", "dark"])
def test_every_material_kind_draws_what_it_can(oracle, built, name):
    R = built[name][0]
    seen = {0: set(), 1: set(), 2: set()}
    for i in np.flatnonzero(R.how != sr.INIT):
        st = R.records[i, 4:10].copy()
        m = R.arrays.materials[int(R.records[i, 1]) & 0xFFFF:][:1]
        oracle.sample_f(m, sr._f32(R.records[i, 13:16]), sr._f32(R.records[i, 19:22]), st)
        seen[int(m["type"][0])].add(int(_draws(R.records[i, 4:5], st[0:1])[0]))
    assert seen == {0: {2}, 1: {0}, 2: {0, 1}}      # matte 2, a mirror 0, glass 1 or -- total internal reflection -- 0


@pytest.mark.parametrize("name", ["small", "large"])
def test_init_records(oracle, built, name):
    R, words, emission, flags = built[name]
    rec = R.records
    b_in, b_out = rec[:, 0].view(np.int32), words[:, 26].view(np.int32)
    alive = (flags & 1) != 0
    rolls = b_out - b_in

    def of(purpose):
        sel = np.flatnonzero(R.purpose == purpose)
        assert len(sel) >= 20, purpose
        return sel

    # emission: at bounce 0 on a light-carrying triangle, the light's L; nowhere else
    e = of("emission")
    lights = R.arrays.lights["L"][((rec[e, 1] >> 16) & 0xFFFF).astype(np.int64) - 1]
    assert ((flags[e] & 4) != 0).all() and np.array_equal(emission[e].view(np.float32), lights) and alive[e].all()
    rest = np.setdiff1d(np.arange(len(rec)), e)
    assert ((flags[rest] & 4) == 0).all() and (emission[rest] == 0).all()
    # no bounce left, and a miss: nothing moves
    for purpose in ("no_bounce_left", "miss"):
        s = of(purpose)
        assert (flags[s] == 0).all() and (rolls[s] == 0).all()
        assert np.array_equal(words[s, 17:26], rec[s][:, [10, 11, 12, 4, 5, 6, 7, 8, 9]])
    # no roulette at bounces == kRrStart or with max3(beta) == 1: one init(), always a shade
    for purpose in ("rr_start", "beta_one", "last_bounce"):
        s = of(purpose)
        assert alive[s].all() and (rolls[s] == 1).all()
    assert (b_out[of("last_bounce")] == R.max_bounces).all()
    # one ulp below 1: the roulette runs with pt = max(0.05, 2^-24) = 0.05.  A survivor of the first roll equals, word for
    # word, the state one draw further on with beta / (1 - pt) -- whose max3 is past 1, so that it does not roll
    s = of("beta_below_one")
    first = alive[s] & (rolls[s] == 1)
    assert first.sum() >= 15
    twin = rec[s].copy()
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(0.05))
    twin[:, 10:13] = (twin[:, 10:13].view(np.float32) * inv).view(np.uint32)
    for k in range(len(twin)):
        st = twin[k, 4:10].copy()
        oracle.xorwow_draw(st, 1)
        twin[k, 4:10] = st
    tw, _, tf = oracle.mat_step(oracle.scene(R.arrays), twin, R.max_bounces)
    assert np.array_equal(tw[first], words[s][first]) and np.array_equal(tf[first], flags[s][first])
    # the roulette chain: 1, 2 and >= 3 draws, killed and surviving; a state that reaches max_bounces inside the chain
    chain = np.concatenate([of("rr_chain"), of("rr_start_plus_1"), of("last_bounce_rr")])
    assert (rolls[chain] >= 1).all()
    for survived in (True, False):
        got = set(np.minimum(rolls[chain][alive[chain] == survived], 3).tolist())
        assert got == {1, 2, 3}, (survived, got)
    killed = chain[~alive[chain]]
    assert (b_out[killed] == R.max_bounces).all()                      # a killed path is rolled again until the last bounce
    assert ((rolls[killed] >= 3) & (b_in[killed] < R.max_bounces - 2)).any()
    assert np.array_equal(words[killed, 17:20], rec[killed, 10:13])    # beta does not change along a chain of kills
    assert (_draws(rec[killed, 4], words[killed, 20]) == rolls[killed]).all()


def test_dark_scene_has_no_shadow_rays(built):
    R, words, emission, flags = built["dark"]
    assert ((flags & 2) == 0).all() and ((flags & 1) != 0).sum() > 50 and (emission == 0).all()


def test_batched_uniform_sample_sphere_equals_the_reference_table(oracle):
    """orc_uniform_sample_sphere_raws (the expected values of the GPU sweep) on the committed table: the reference's own words."""
    rows, want = sr.FIXTURE["in_uniform_sample_sphere"], sr.FIXTURE["out_uniform_sample_sphere"]
    got = oracle.uniform_sample_sphere_raws(rows)
    assert len(rows) == 1200 and np.array_equal(got, want)
