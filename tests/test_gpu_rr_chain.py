"""init()'s Russian-roulette chain on the device -- advance_core's loop of draws -- against the oracle.  Run with -m gpu.

advance_core runs a killed path's re-rolls as one loop inside the ADV block: the number of rolls a lane may make is fixed
before the loop, a turn holds the draw and one stop test, and bounces, the survivor's beta and the routing follow from the
number of rolls behind it.  rt_shade_records (the lab library) runs that code on the path states of
tests/rr_chain_records.py -- every limit 1 .. 5 (max_bounces 10, 7 and 6), every chain length at each, killed to the end
and surviving, draws one step below pt, at pt and one step above, pt at its floor, mid-range and high, and the states for
which no chain runs -- 64 consecutive records to a wave, so that lanes with chains of every length, misses, paths without
a bounce left and matte and specular hits sit side by side; one wave rolls five times on all 64 lanes, one on exactly one.

Oracle.mat_step runs the oracle's init() + mat() on the same states.  All 27 output words and the three emission words are
compared as integers (a NaN must be a NaN), in both table placements; where the kernel writes nothing (no new ray, no
shadow ray) the flags are compared and nothing else.  tests/test_rr_chain_records_host.py holds the records to what they are
meant to be on the CPU."""
import numpy as np
import pytest

import rr_chain_records as rc

pytestmark = pytest.mark.gpu

NO_SHADOW = 0xBF800000     # word 12 (s_tmax) without a shadow ray: -1.0f


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.tools_lib()
    return _api


@pytest.fixture(scope="module")
def built(oracle):
    """max_bounces -> (Records, the oracle's words, emission, flags): computed once, shared, never changed."""
    out = {}
    for M, R in rc.build().items():
        out[M] = (R,) + oracle.mat_step(oracle.scene(R.arrays), R.records, R.max_bounces)
    return out


def _canon(words):
    w = np.array(words, np.uint32)
    w[np.isnan(w.view(np.float32))] = 0x7FC00000
    return w


@pytest.mark.parametrize("lds", [0, 1])
@pytest.mark.parametrize("M", rc.MAX_BOUNCES)
def test_chain_equals_the_oracle(api, built, M, lds):
    R, want, emission, flags = built[M]
    scene = api.Scene(R.arrays, library=api.tools_lib())
    got = api.shade_records(scene, R.records, R.max_bounces, bool(lds))
    scene.close()
    assert got.shape == (len(R.records), api.SHADE_RECORD_OUT)
    new_ray = ~(got[:, 0:6] == api.SHADE_UNWRITTEN).all(axis=1)
    shadow = got[:, 12] != NO_SHADOW
    rolls = got[:, 26].view(np.int32) - R.records[:, 0].view(np.int32)
    print(f"max_bounces {M} lds={lds}: {len(got)} records, {int(new_ray.sum())} shade, {int(shadow.sum())} shadow rays, "
          f"rolls {np.bincount(np.clip(rolls, 0, 6)).tolist()}")
    bad_flags = np.flatnonzero((new_ray != ((flags & 1) != 0)) | (shadow != ((flags & 2) != 0)))
    assert len(bad_flags) == 0, (len(bad_flags), [(int(i), str(R.purpose[i]), str(R.batch[i]), R.expect[i].tolist()) for i in bad_flags[:5]])
    assert not (got[:, 17:27] == api.SHADE_UNWRITTEN).all(axis=1).any()      # the kernel ran: beta, rng and bounces are always written
    compare = np.ones((len(got), 27), bool)
    compare[~new_ray, 0:6] = False
    compare[~shadow, 6:12] = False
    compare[~shadow, 13:17] = False
    g, w = _canon(got[:, :27]), _canon(want)
    bad = np.flatnonzero(((g != w) & compare).any(axis=1))
    assert len(bad) == 0, (len(bad), [(int(i), str(R.purpose[i]), str(R.batch[i]), R.expect[i].tolist(),
                                       np.flatnonzero((g[i] != w[i]) & compare[i]).tolist(), R.records[i].tolist(), g[i].tolist(),
                                       w[i].tolist()) for i in bad[:3]])
    assert np.array_equal(_canon(got[:, 27:30]), _canon(emission)), "bounce-0 emission"
    # and, from the device's words alone, what the builder meant: the rolls made and how the record ended
    assert np.array_equal(rolls, R.expect[:, 0]) and np.array_equal(new_ray.astype(np.int32), R.expect[:, 1])
