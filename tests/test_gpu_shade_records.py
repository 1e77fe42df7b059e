"""Whole shading steps on the device -- init() + mat() as k_paths compiles them -- against the oracle.  Run with -m gpu.

sample_Li and sample_p have no device function of their own: their code lives inside mat(), with the light pick, the
1 / area and unit-normal tables k_build_tables precomputes per scene, the beta update, the Russian-roulette chain of init()
and the burn of the second sample_f call's draws.  rt_shade_records (the lab library) runs the product's advance_core --
the instantiation the persistent kernel uses, through the shading probe -- on the path states of tests/shade_records.py,
one lane each; Oracle.mat_step runs the function the oracle's per-sample renderer is made of on the same states.  All 27
output words and the emission must be equal as integers (a NaN must be a NaN).  Where the kernel writes nothing (no new
ray, no shadow ray) the flags are compared and nothing else.

tests/test_shade_records_host.py asserts that the records reach what they are there for: every light picked, the zero-area
light triangles, the shading points that sit on a point light, dot(wo, n) of 0 and +-1, the critical angle, every length of
roulette chain, killed and surviving.

Tied to the reference directly, without the oracle: where a shadow ray exists and the light sample is the one the committed
sample_Li table holds -- always for a point light, whose sample depends on (light, p) alone, and for the REPLAY records,
whose state replays the table's own two uniforms on an area light -- s_d and s_tmax equal the wi and t words of the
committed out_sample_Li row; a REPLAY record's new ray direction equals the committed out_sample_f row's wi.  (A STREAM
record that picks an area light samples the triangle with whatever its stream holds: it is held to the oracle only.)

Light::pdf_Li (table 4 of the fixture) has no device counterpart: its only caller is the BSDF-sampled MIS ray, which the
device does not make (it cannot contribute; its draws are burnt).  It stays CPU-only (tests/test_ref_shade_pins.py).
"""
import numpy as np
import pytest

import shade_records as sr

pytestmark = pytest.mark.gpu

NO_SHADOW = 0xBF800000     # word 12 (s_tmax) without a shadow ray: -1.0f
CASES = [("small", 0), ("small", 1), ("large", 0), ("dark", 0), ("dark", 1)]


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.tools_lib()
    return _api


@pytest.fixture(scope="module")
def built(oracle):
    """name -> (Records, the oracle's words, emission, flags): computed once, shared, never changed."""
    out = {}
    for name, R in sr.build(oracle).items():
        out[name] = (R,) + oracle.mat_step(oracle.scene(R.arrays), R.records, R.max_bounces)
    return out


_gpu_cache = {}


def _device(api, built, name, lds):
    if (name, lds) not in _gpu_cache:
        R = built[name][0]
        scene = api.Scene(R.arrays, library=api.tools_lib())
        _gpu_cache[(name, lds)] = api.shade_records(scene, R.records, R.max_bounces, bool(lds))
        scene.close()
    return _gpu_cache[(name, lds)]


def _canon(words):
    w = np.array(words, np.uint32)
    w[np.isnan(w.view(np.float32))] = 0x7FC00000
    return w


@pytest.mark.parametrize("name,lds", CASES)
def test_shading_step_equals_the_oracle(api, built, name, lds):
    R, want, emission, flags = built[name]
    got = _device(api, built, name, lds)
    assert got.shape == (len(R.records), api.SHADE_RECORD_OUT)
    new_ray = ~(got[:, 0:6] == api.SHADE_UNWRITTEN).all(axis=1)
    shadow = got[:, 12] != NO_SHADOW
    bad_flags = np.flatnonzero((new_ray != ((flags & 1) != 0)) | (shadow != ((flags & 2) != 0)))
    assert len(bad_flags) == 0, (len(bad_flags), [(int(i), str(R.purpose[i])) for i in bad_flags[:5]])
    assert not (got[:, 17:27] == api.SHADE_UNWRITTEN).all(axis=1).any()      # the kernel ran: beta, rng and bounces are always written
    compare = np.ones((len(got), 27), bool)
    compare[~new_ray, 0:6] = False
    compare[~shadow, 6:12] = False
    compare[~shadow, 13:17] = False
    g, w = _canon(got[:, :27]), _canon(want)
    bad = np.flatnonzero(((g != w) & compare).any(axis=1))
    print(f"{name} lds={lds}: {len(bad)} of {len(got)} records differ; {int(new_ray.sum())} shade, {int(shadow.sum())} shadow rays")
    assert len(bad) == 0, (len(bad), [(int(i), str(R.purpose[i]), np.flatnonzero((g[i] != w[i]) & compare[i]).tolist(),
                                      R.records[i].tolist(), g[i].tolist(), w[i].tolist()) for i in bad[:3]])
    assert np.array_equal(_canon(got[:, 27:30]), _canon(emission)), "bounce-0 emission"


def test_both_table_builds_agree(api, built):
    for name in ("small", "dark"):
        assert np.array_equal(_device(api, built, name, 0), _device(api, built, name, 1)), name


def test_lds_tables_past_the_gate_is_an_error(api, built):
    R = built["large"][0]
    scene = api.Scene(R.arrays, library=api.tools_lib())
    with pytest.raises(api.RtError, match="lds_tables"):
        api.shade_records(scene, R.records[:4], R.max_bounces, True)
    bad = R.records[:4].copy()
    bad[2, 2] = 4                                                      # a pixel outside the call's framebuffer
    with pytest.raises(api.RtError, match="pixel"):
        api.shade_records(scene, bad, R.max_bounces, False)
    bad = R.records[:4].copy()
    bad[1, 1] = 100                                                    # material 100 of 100
    with pytest.raises(api.RtError, match="out of range"):
        api.shade_records(scene, bad, R.max_bounces, False)
    assert api.shade_records(scene, R.records[:0], R.max_bounces, False).shape == (0, api.SHADE_RECORD_OUT)
    scene.close()


@pytest.mark.parametrize("name,lds", [("small", 1), ("large", 0)])
def test_shadow_rays_equal_the_committed_sample_Li_rows(api, built, name, lds):
    R = built[name][0]
    got = _canon(_device(api, built, name, lds))
    shadow = got[:, 12] != NO_SHADOW
    point = R.arrays.lights["type"][np.maximum(R.light, 0)] == 0
    tied = np.flatnonzero(shadow & (R.light >= 0) & (point | (R.how == sr.REPLAY)))
    area_tied = int((~point[tied]).sum())
    print(f"{name}: {len(tied)} shadow rays tied to the fixture, {area_tied} of them on area lights")
    assert area_tied >= 0.6 * (R.arrays.lights["type"] == 1).sum() and (point[tied]).sum() >= 10
    ref = _canon(sr.T3_OUT[R.light[tied]])
    assert np.array_equal(got[tied, 9:12], ref[:, 1:4]), "s_d != the reference's wi"
    assert np.array_equal(got[tied, 12], ref[:, 7]), "s_tmax != the reference's t"
    replay = np.flatnonzero((R.how == sr.REPLAY) & ~(got[:, 0:6] == api.SHADE_UNWRITTEN).all(axis=1))
    assert len(replay) >= 40
    assert np.array_equal(got[replay, 3:6], _canon(sr.T1_OUT[R.t1_row[replay], 3:6])), "ray_d != the reference's sample_f wi"
