"""GPU tests of the background skip of k_paths / k_paths<PathsChunked> (rt_background.h): a camera ray whose pixel
lies outside the rectangle the scene's bounds project to is counted, its two jitter draws are made, and no ray is made or
walked.  Nothing else may change: RT_FLAG_DETERMINISTIC's int64 sums and every event total must EQUAL the CPU oracle's, those of
the same frame with RT_BG_SKIP=0 (the rectangle is the whole frame: every ray is walked, as before).  Run with -m gpu.  Those
comparisons are exact.

The round pipeline (RT_PERSISTENT=0) keeps tracing every ray.  Its event totals must equal the persistent frame's exactly.  Its
sums equal the persistent frame's bit for bit where a camera ray has at most one contribution (max_bounces = 0; a camera turned
away).  With several contributions per ray the two pipelines round differently whatever this change does -- k_paths adds a
camera ray's contributions in fp32 and deposits the sum once, k_advance / k_trace deposit each contribution, and both convert
to 2^-30 fixed point per deposit (160 x 90 x 256: 16 202 of 43 200 sums differ, with RT_BG_SKIP=0 as well) -- so there the
sums are held to the bound of exactly that: see _same_as_rounds."""
import numpy as np
import pytest

from conftest import default_camera, oracle_scene, usable_cpus
from test_gpu_slot_chunks import EVENTS, _check, _oracle_sums

pytestmark = pytest.mark.gpu

W = 1 << 20
TOTALS = ("camera_rays", "closest_rays") + tuple(kg for kg, _ in EVENTS)


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


def _knobs(monkeypatch, skip=True, persistent=True, chunk=None, head=None):
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "1")
    for name, value in (("RT_BG_SKIP", None if skip else 0), ("RT_PERSISTENT", None if persistent else 0), ("RT_SLOT_CHUNK", chunk),
                        ("RT_SLOT_HEAD", head)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


def _sums(api, gpu, w, h, spp, flags=0, shard=(0, 1), max_bounces=10, cam=None):
    import torch
    buf = torch.zeros(h * w * 3, dtype=torch.int64, device="cuda")
    cam = api.make_camera(aspect=w / h) if cam is None else cam
    st = gpu.render_shard_fixed(cam, w, h, spp, shard[0], shard[1], buf.data_ptr(), max_bounces=max_bounces, flags=flags)
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(h, w, 3), st


def _same(got, st, ref, st_ref, what):
    assert np.array_equal(got, ref), (what, int((got != ref).sum()))
    for k in TOTALS:
        assert st[k] == st_ref[k], (what, k, st[k], st_ref[k])


def _same_as_rounds(got, st, rnd, st_rnd, spp, max_bounces, what):
    """The persistent frame against the round pipeline's: every event total, exactly; the sums exactly where a camera ray has one
    contribution, else within what the two summation orders can differ by.  A camera ray has at most n = max_bounces + 1
    contributions c_k >= 0 (bounce-0 emission or the shadow rays of its bounces).  Rounds: each c_k is converted on its own, half
    a unit of 2^-30 each.  Persistent: fl(c_1 + ... + c_n) with at most (n - 1) roundings of 2^-24 relative to the partial sums,
    each no larger than the ray's total, then one conversion.  Over the spp camera rays of a pixel:
        |persistent - rounds| <= (n - 1) 2^-24 (1 + 2^-24)^(n - 1) total + (n + 1) spp / 2      (units of 2^-30)."""
    for k in TOTALS:
        assert st[k] == st_rnd[k], (what, k, st[k], st_rnd[k])
    if max_bounces == 0:
        assert np.array_equal(got, rnd), (what, int((got != rnd).sum()))
        return
    n = max_bounces + 1
    total = np.maximum(np.abs(got), np.abs(rnd)).astype(np.float64)
    bound = (n - 1) * 2.0 ** -24 * (1 + 2.0 ** -24) ** (n - 1) * total + (n + 1) * spp / 2
    diff = np.abs(got - rnd).astype(np.float64)
    print(what, "sums that differ from the rounds':", int((diff > 0).sum()), "largest difference / bound", float((diff / bound).max()))
    assert (diff <= bound).all(), (what, float((diff / bound).max()))
    assert not rnd[got == 0].any() and not got[rnd == 0].any(), what  # (a pixel nothing reaches is exactly zero in both)


def _expect_skip(api, w, h, cam=None, arrays=None):
    """Whether the frame's persistent launch must be a skipping build: the rectangle rt_background_rect gives for the camera and
    the scene's bounds (the library computes it from the root's child boxes, 2 ulps wider: the same pixels in these frames) is
    smaller than the frame.  Every frame of this file has background, so every one must take the skipping kernel.  `arrays`: the
    scene's, where it is not the full-BSDF bunny."""
    from test_background_rect_host import bounds, rect
    cam = api.make_camera(aspect=w / h) if cam is None else cam
    x0, y0, x1, y1 = rect(cam, w, h, *bounds(_arrays() if arrays is None else arrays))
    return (x1 - x0) * (y1 - y0) < w * h


_arrays_cache = []


def _arrays():
    if not _arrays_cache:
        from rtcuda_amd import scenes
        _arrays_cache.append(scenes.cornell_bunny("full_bsdf"))
    return _arrays_cache[0]


def _on_off(api, gpu, monkeypatch, w, h, spp, want=None, st_c=None, rounds=False, arrays=None, **kw):
    """The frame with the skip on (the default), held to the oracle's frame if given, and to RT_BG_SKIP=0; `rounds`: and to the
    round pipeline.  The skipping frame's persistent launch must have been k_paths<PathsBg> / k_paths<PathsChunkedBg>
    (st["background_skip"]; without that the comparisons below would hold trivially), the RT_BG_SKIP=0 frame's and the rounds' not.
    `arrays`: what `gpu` holds, where it is not the full-BSDF bunny.  Returns the frame."""
    what = (w, h, spp, tuple(sorted(kw.items(), key=lambda t: t[0])) if "cam" not in kw else "cam")
    _knobs(monkeypatch)
    got, st = _sums(api, gpu, w, h, spp, **kw)
    assert _expect_skip(api, w, h, kw.get("cam"), arrays), what
    assert st["background_skip"] == 1, (what, "the frame did not run a skipping kernel")
    if want is not None:
        _check(got, st, want, st_c, f"skip on {what}")
    _knobs(monkeypatch, skip=False)
    off, st_off = _sums(api, gpu, w, h, spp, **kw)
    assert st_off["background_skip"] == 0, what
    if want is not None:
        _check(off, st_off, want, st_c, f"RT_BG_SKIP=0 {what}")
    _same(got, st, off, st_off, ("skip on / off", what))
    if rounds:
        _knobs(monkeypatch, persistent=False)
        rnd, st_rnd = _sums(api, gpu, w, h, spp, **kw)
        assert st_rnd["background_skip"] == 0, what
        _same_as_rounds(got, st, rnd, st_rnd, spp, kw.get("max_bounces", 10), ("persistent / RT_PERSISTENT=0", what))
    _knobs(monkeypatch)
    return got, st


# 160 x 90 x 256: 3.5 generations; the rectangle is columns 35 .. 124 of every row, (35, 0, 125, 90): its left and right edges lie
# inside the frame, its top and bottom edges are the frame's (at no size of this file is a row skipped: the views that cut rows off,
# start at column 0 or end at the last row are in test_gpu_background_views.py).  96 x 54 x 509: an odd spp (no pixel stepping:
# the division path).  200 x 120 x 16 and 640 x 360 x 16 (3.5 generations): a wave's 64 slots span four pixels, so lanes of one
# wave stand on both sides of an edge.
@pytest.mark.parametrize("w,h,spp", [(160, 90, 256), (96, 54, 509), (200, 120, 16), (640, 360, 16)])
def test_frames_equal_the_oracle_the_unskipped_frame_and_the_rounds(api, gpu, oracle, monkeypatch, w, h, spp):
    want, st_c = _oracle_sums(oracle, w, h, spp)
    _, st = _on_off(api, gpu, monkeypatch, w, h, spp, want, st_c, rounds=True)
    assert st["camera_rays"] == w * h * spp


@pytest.mark.parametrize("max_bounces", [0, 10])
def test_max_bounces(api, gpu, oracle, monkeypatch, max_bounces):
    w, h, spp = 160, 90, 256
    if max_bounces == 10:
        want, st_c = _oracle_sums(oracle, w, h, spp)
    else:
        want = np.zeros((h, w, 3), np.int64)
        _, _, st_c = oracle_scene(oracle, "full_bsdf", False).render(default_camera(oracle, w / h), w, h, spp, max_bounces=max_bounces,
                                                                     threads=usable_cpus(), fixed_out=want)
    _on_off(api, gpu, monkeypatch, w, h, spp, want, st_c, rounds=True, max_bounces=max_bounces)


# shard 1 of 4: one slot per lane at 4 waves per SIMD; shard 0 of 8: the 2-waves-per-SIMD build, whose gen() is advance_core's own
@pytest.mark.parametrize("shard", [(1, 4), (0, 8)])
def test_slot_range_shards(api, gpu, oracle, monkeypatch, shard):
    w, h, spp = 160, 90, 256
    want, st_c = _oracle_sums(oracle, w, h, spp, shard=shard)
    _on_off(api, gpu, monkeypatch, w, h, spp, want, st_c, shard=shard)


@pytest.mark.parametrize("mode", ["watertight", "reference_walk"])
def test_the_other_reference_mode_builds(api, gpu, oracle, monkeypatch, mode):
    w, h, spp = 160, 90, 256
    flags = {"watertight": api.FLAG_WATERTIGHT, "reference_walk": api.FLAG_REFERENCE_WALK}[mode]
    want, st_c = _oracle_sums(oracle, w, h, spp, watertight=mode == "watertight")
    _on_off(api, gpu, monkeypatch, w, h, spp, want, st_c, flags=flags)


def test_per_sample_streams_equal_render_per_sample(api, gpu, oracle, monkeypatch):
    """RT_FLAG_RNG_PER_SAMPLE: a drawn id whose pixel is background is counted and dropped without starting its stream."""
    w, h, spp = 160, 90, 256
    want = np.zeros((h, w, 3), np.int64)
    _, _, st_c = oracle_scene(oracle, "full_bsdf", True).render(default_camera(oracle, w / h), w, h, spp, threads=usable_cpus(),
                                                                fixed_out=want, rng_mode="per_sample")
    got, st = _on_off(api, gpu, monkeypatch, w, h, spp, want, st_c, flags=api.FLAG_RNG_PER_SAMPLE)
    assert st["camera_rays"] == st_c["sum_gen"] == w * h * spp


def test_camera_turned_away_from_the_scene(api, gpu, monkeypatch):
    """Every camera ray is skipped: the image is all zero and every ray is still counted."""
    w, h, spp = 160, 90, 256
    cam = api.make_camera(lookfrom=(0.5, 0.5, 1.5), lookat=(0.5, 0.5, 3.0), aspect=w / h)
    got, st = _on_off(api, gpu, monkeypatch, w, h, spp, rounds=True, cam=cam)
    assert not got.any()
    assert st["camera_rays"] == st["closest_rays"] == w * h * spp
    for kg, _ in EVENTS:
        assert st[kg] == 0, (kg, st[kg])


def test_background_runs_across_chunk_ends(api, gpu, monkeypatch):
    """1024 x 770 x 512: 385 generations, so chains of 384 rays in k_paths<PathsChunked> -- the shortest the launch plan deals -- and
    G = 48.  (1024 x 768 x 512 is exactly 384 generations: its chains are 383 rays, the last generation runs in lockstep, and the
    plan keeps the static deal.)  A run of background generations crosses chunk ends and reaches the end of a slot's chain.
    Skip on against RT_BG_SKIP=0 (no oracle at this size), then the same with every set dealt 64 rays at a time."""
    w, h, spp = 1024, 770, 512
    ref = None
    for chunk, head, g in ((None, None, 48), (64, 0, 64)):
        _knobs(monkeypatch, chunk=chunk, head=head)
        got, st = _sums(api, gpu, w, h, spp)
        assert st["slot_chunk"] == g, st["slot_chunk"]
        assert st["background_skip"] == 1 and _expect_skip(api, w, h)  # (k_paths<PathsChunkedBg>)
        assert st["camera_rays"] == w * h * spp
        _knobs(monkeypatch, skip=False, chunk=chunk, head=head)
        off, st_off = _sums(api, gpu, w, h, spp)
        assert st_off["slot_chunk"] == g and st_off["background_skip"] == 0  # (k_paths<PathsChunked>)
        _same(got, st, off, st_off, ("skip on / off", chunk, head))
        if ref is not None:
            _same(got, st, ref[0], ref[1], "G = 48 / G = 64 head 0")
        ref = (got, st)
    _knobs(monkeypatch)
