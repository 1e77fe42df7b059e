"""The Russian-roulette chain records do what their builder means them to -- asserted from the oracle alone.  CPU only.

tests/rr_chain_records.py builds the path states that tests/test_gpu_rr_chain.py runs through the kernels' advance_core.
A raw draw placed on the wrong side of pt, or a chain one roll short, would leave the GPU comparison green and testing
something else; here Oracle.mat_step says how often each record rolled and whether it ended in a shade."""
import numpy as np
import pytest

import rr_chain_records as rc
import shade_records as sr
import shade_scenes as ss

WEYL_INV = pow(362437, -1, 1 << 32)


@pytest.fixture(scope="module")
def built(oracle):
    out = {}
    for M, R in rc.build().items():
        out[M] = (R,) + oracle.mat_step(oracle.scene(R.arrays), R.records, R.max_bounces)
    return out


def test_edge_raws_sit_at_the_comparison(oracle):
    exact = 0
    for bmax in rc.BETA_MAX:
        pt = rc.pt_of([np.float32(bmax), np.float32(0.5 * bmax), np.float32(0.25 * bmax)])
        below, at, above = rc.edge_raws(pt)
        # the oracle's own uniforms of the three raws, and of their neighbours
        _, u = oracle.xorwow_draw(sr.replay_state([below, at, above - 1, above]).copy(), 4)
        assert u[0] < pt and u[1] >= pt and u[2] <= pt and u[3] > pt and at == below + 1
        assert np.array_equal(u, ss.uniform_of([below, at, above - 1, above]))
        exact += int(u[1] == pt)
    assert exact >= 1       # a draw EQUAL to pt exists for at least one pt (0.5), and it survives


@pytest.mark.parametrize("M", rc.MAX_BOUNCES)
def test_records_roll_and_end_as_meant(built, M):
    R, words, _, flags = built[M]
    rec = R.records
    b_in, b_out = rec[:, 0].view(np.int32), words[:, 26].view(np.int32)
    shaded = ((flags & 1) != 0).astype(np.int32)
    assert np.array_equal(b_out - b_in, R.expect[:, 0])
    assert np.array_equal(shaded, R.expect[:, 1])
    chain = R.purpose == "chain"
    killed = chain & (shaded == 0)
    assert (b_out[killed] == M).all() and np.array_equal(words[killed, 17:20], rec[killed, 10:13])
    draws = ((words[:, 20].astype(np.uint64) - rec[:, 4].astype(np.uint64)) * np.uint64(WEYL_INV)) & np.uint64(0xFFFFFFFF)
    assert (draws[killed] == R.expect[killed, 0]).all()                    # a roll is a draw; a killed path draws nothing else
    assert (draws[chain & (shaded == 1)] >= R.expect[chain & (shaded == 1), 0]).all()
    assert (draws[np.isin(R.purpose, ["miss", "no_bounce_left"])] == 0).all()
    # every limit, and at every limit every length, killed and surviving
    limit = M - b_in
    for L in range(1, M - sr.RR_START):
        at_L = chain & (limit == L)
        assert set(R.expect[at_L & (shaded == 1), 0].tolist()) == set(range(1, L + 1)), L
        assert (R.expect[at_L & (shaded == 0), 0] == L).all() and (at_L & (shaded == 0)).sum() >= 8, L
    assert set((limit[chain]).tolist()) == set(range(1, M - sr.RR_START))
    for purpose in ("beta_one", "rr_start", "no_bounce_left", "miss"):
        assert (R.purpose == purpose).sum() >= 8, purpose
    kinds = R.arrays.materials["type"][np.maximum(rec[:, 1].view(np.int32), 0) & 0xFFFF]
    assert (kinds[chain] == ss.MATTE).sum() > 0.3 * chain.sum() and (kinds[chain] != ss.MATTE).sum() > 0.3 * chain.sum()


def test_waves_are_mixed(built):
    R = built[10][0]
    n = len(R.records)
    assert n % rc.WAVE == 0 and 2000 <= sum(2 * len(built[M][0].records) for M in rc.MAX_BOUNCES) <= 8192
    rolls = np.where(R.purpose == "chain", R.expect[:, 0], 0).reshape(-1, rc.WAVE)
    batch = R.batch.reshape(-1, rc.WAVE)[:, 0]
    assert (R.batch.reshape(-1, rc.WAVE) == batch[:, None]).all()
    mixed = rolls[batch == "mixed"]
    assert len(mixed) >= 16
    assert (np.array([len(set(w.tolist())) for w in mixed]) >= 5).mean() > 0.9      # chains of most lengths side by side
    purposes = R.purpose.reshape(-1, rc.WAVE)[batch == "mixed"]
    assert np.mean([("miss" in w) and ("no_bounce_left" in w) for w in purposes.tolist()]) > 0.9
    assert (rolls[batch == "all_five"] == 5).all() and (batch == "all_five").sum() == 1
    ends = R.expect[:, 1].reshape(-1, rc.WAVE)[batch == "all_five"][0]
    assert 0 < ends.sum() < rc.WAVE                                        # survivors of the fifth roll beside paths killed by it
    one = rolls[batch == "one_five"]
    assert one.shape == (1, rc.WAVE) and (one == 5).sum() == 1 and (one == 0).sum() == rc.WAVE - 1
