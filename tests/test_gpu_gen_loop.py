"""GPU tests of the GEN block's run over background pixels in k_paths<PathsBg> / k_paths<PathsChunkedBg>: a lane's run
ends at a pixel inside the rectangle or at ONE limit fixed before the run (rtchunks::run_limit: the end of the slot's chain, a
dealt lane's next chunk's end, one turn where the pixel cannot be stepped).  The frames here put the three limits where a run
meets them; RT_FLAG_DETERMINISTIC's int64 sums and every event total must EQUAL the CPU oracle's and those of the same frame
with RT_BG_SKIP=0.  Run with -m gpu."""
import numpy as np
import pytest

from conftest import default_camera, oracle_scene, usable_cpus
from test_gpu_background_skip import _expect_skip, _knobs, _on_off, _same, _sums
from test_gpu_slot_chunks import EVENTS, _check, _oracle_sums

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()  # raises if the HIP library is missing: there is no fallback
    return _api


@pytest.fixture(scope="module")
def gpu(api):
    from rtcuda_amd import scenes
    sc = api.Scene(scenes.cornell_bunny("full_bsdf"))
    yield sc
    sc.close()


def _skipping(api, gpu, monkeypatch, w, h, spp, chunk, head, **kw):
    """The frame with the skip on and with RT_BG_SKIP=0 under the same deal; both must report the deal, the first the skip.
    chunk None: no RT_SLOT_CHUNK, the launch plan's own deal, whatever it is -- the same in both frames."""
    _knobs(monkeypatch, chunk=chunk, head=head)
    got, st = _sums(api, gpu, w, h, spp, **kw)
    assert _expect_skip(api, w, h, kw.get("cam"))
    assert st["background_skip"] == 1, "the frame did not run a skipping kernel"
    dealt = st["slot_chunk"] if chunk is None else chunk
    assert st["slot_chunk"] == dealt, (st["slot_chunk"], chunk)
    _knobs(monkeypatch, skip=False, chunk=chunk, head=head)
    off, st_off = _sums(api, gpu, w, h, spp, **kw)
    assert st_off["background_skip"] == 0 and st_off["slot_chunk"] == dealt
    _knobs(monkeypatch)
    _same(got, st, off, st_off, ("skip on / off", chunk, head))
    return got, st


# 320 x 180 x 256: 14.06 generations, so chains of 14 camera rays in k_paths<PathsChunkedBg>.  G = 1: every turn of a run ends a
# chunk; 4 and 5 do not divide the chain; 13: a chunk's end one turn before the chain's.  RT_SLOT_HEAD unset: the plan's static
# head (lanes inside it run to g_stop, lanes past it to the chunk's end, in one wave); 0: every set dealt.
@pytest.mark.parametrize("head", [None, 0])
@pytest.mark.parametrize("chunk", [1, 4, 5, 13])
def test_runs_end_at_chunk_ends(api, gpu, oracle, monkeypatch, chunk, head):
    w, h, spp = 320, 180, 256
    want, st_c = _oracle_sums(oracle, w, h, spp)
    got, st = _skipping(api, gpu, monkeypatch, w, h, spp, chunk, head)
    _check(got, st, want, st_c, f"RT_SLOT_CHUNK={chunk} RT_SLOT_HEAD={head}")
    assert st["camera_rays"] == w * h * spp


def test_every_run_ends_at_a_limit(api, gpu, monkeypatch):
    """The camera turned away from the scene: no run ever ends at a ray, every one at a chunk's end or at the chain's.  The image
    is all zero and every camera ray is counted."""
    w, h, spp = 320, 180, 256
    cam = api.make_camera(lookfrom=(0.5, 0.5, 1.5), lookat=(0.5, 0.5, 3.0), aspect=w / h)
    got, st = _skipping(api, gpu, monkeypatch, w, h, spp, 4, None, cam=cam)
    assert not got.any()
    assert st["camera_rays"] == st["closest_rays"] == w * h * spp
    for kg, _ in EVENTS:
        assert st[kg] == 0, (kg, st[kg])


def test_odd_spp_takes_one_turn_per_visit(api, gpu, oracle, monkeypatch):
    """96 x 54 x 509: the pixel cannot be stepped (dpy < 0), so the limit is one turn and the pixel comes from the divisions."""
    w, h, spp = 96, 54, 509
    want, st_c = _oracle_sums(oracle, w, h, spp)
    got, st = _skipping(api, gpu, monkeypatch, w, h, spp, 2, None)
    _check(got, st, want, st_c, "odd spp, RT_SLOT_CHUNK=2")
    assert st["camera_rays"] == w * h * spp


def test_per_sample_streams(api, gpu, oracle, monkeypatch):
    """RT_FLAG_RNG_PER_SAMPLE: the build without a loop -- one turn per drawn id, no stream for a background id."""
    w, h, spp = 160, 90, 256
    want = np.zeros((h, w, 3), np.int64)
    _, _, st_c = oracle_scene(oracle, "full_bsdf", True).render(default_camera(oracle, w / h), w, h, spp, threads=usable_cpus(),
                                                                fixed_out=want, rng_mode="per_sample")
    got, st = _on_off(api, gpu, monkeypatch, w, h, spp, want, st_c, flags=api.FLAG_RNG_PER_SAMPLE)
    assert st["camera_rays"] == st_c["sum_gen"] == w * h * spp


def test_long_chains_dealt_64_at_a_time(api, gpu, monkeypatch):
    """1024 x 770 x 512 (chains of 384 camera rays), every set dealt 64 rays at a time: against the plan's own deal (G = 48 with
    its static head) and, each, against RT_BG_SKIP=0.  No oracle at this size."""
    w, h, spp = 1024, 770, 512
    _knobs(monkeypatch)
    ref, st_ref = _sums(api, gpu, w, h, spp)
    assert st_ref["slot_chunk"] == 48 and st_ref["background_skip"] == 1
    got, st = _skipping(api, gpu, monkeypatch, w, h, spp, 64, 0)
    assert st["camera_rays"] == w * h * spp
    _same(got, st, ref, st_ref, "G = 64 head 0 / the default deal")
