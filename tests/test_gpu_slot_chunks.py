"""GPU tests of k_paths' chunked deal (rt_slot_chunks.h): a workgroup's lanes take its slots G camera rays
at a time, so a slot's chain of camera rays moves from lane to lane between two rays.  Nothing a ray does may change: with
RT_SLOT_CHUNK = 1, 2, 3 (3 divides neither chain length) the event totals and RT_FLAG_DETERMINISTIC's int64 sums must EQUAL
the CPU oracle's and those of RT_SLOT_CHUNK=0, the static deal -- every path, every random number, every contribution.
Run with -m gpu.  All comparisons are exact."""
import numpy as np
import pytest

from conftest import default_camera, oracle_scene, usable_cpus

pytestmark = pytest.mark.gpu

W = 1 << 20
EVENTS = (("shade_events", "sum_mat"), ("any_rays", "sum_ah"), ("emission_adds", "emission_adds"), ("shadow_adds", "ah_adds"),
          ("rr_draws", "rr_draws"))


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


_oracle_cache = {}


def _oracle_sums(oracle, w, h, spp, watertight=False, shard=(0, 1)):
    """The oracle's fixed-point sums and event totals of (a slot-range shard of) the frame, computed once."""
    key = (w, h, spp, watertight, shard)
    if key not in _oracle_cache:
        r, R = shard
        n = W // R
        want = np.zeros((h, w, 3), np.int64)
        osc = oracle_scene(oracle, "full_bsdf", watertight)
        _, _, st = osc.render(default_camera(oracle, w / h), w, h, spp, threads=usable_cpus(), fixed_out=want,
                              slot_lo=r * n, slot_hi=(r + 1) * n)
        want.setflags(write=False)
        _oracle_cache[key] = (want, st)
    return _oracle_cache[key]


def _gpu_sums(api, gpu, w, h, spp, flags=0, shard=(0, 1), chunk=0):
    """The frame's int64 sums and stats; `chunk`: the G the launch must report having run with (0 = the static deal, k_paths)."""
    import torch
    buf = torch.zeros(h * w * 3, dtype=torch.int64, device="cuda")
    st = gpu.render_shard_fixed(api.make_camera(aspect=w / h), w, h, spp, shard[0], shard[1], buf.data_ptr(), flags=flags)
    torch.cuda.synchronize()
    assert st["slot_chunk"] == chunk, (st["slot_chunk"], chunk)
    return buf.cpu().numpy().reshape(h, w, 3), st


def _chunk(monkeypatch, g):
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "1")
    monkeypatch.setenv("RT_SLOT_CHUNK", str(g))


def _check(got, st_g, want, st_c, what):
    for kg, kc in EVENTS:
        print(what, kg, st_g[kg], st_c[kc])
        assert st_g[kg] == st_c[kc], (what, kg, st_g[kg], st_c[kc])
    bad = int((got != want).sum())
    print(what, "sums that differ from the oracle's:", bad)
    assert bad == 0, (what, bad, np.argwhere(got != want)[:4])


# 480 x 270 x 32: 3.96 generations, spp | W.  300 x 200 x 48: spp does not divide W, and slots differ in their number of rays.
FRAMES = [(480, 270, 32), (300, 200, 48)]


@pytest.mark.parametrize("w,h,spp", FRAMES)
def test_chunked_deal_equals_the_oracle_and_the_static_deal(api, gpu, oracle, monkeypatch, w, h, spp):
    want, st_c = _oracle_sums(oracle, w, h, spp)
    _chunk(monkeypatch, 0)
    static, st_0 = _gpu_sums(api, gpu, w, h, spp)
    assert st_0["camera_rays"] == w * h * spp
    _check(static, st_0, want, st_c, "static deal")
    for g in (1, 2, 3):
        _chunk(monkeypatch, g)
        got, st_g = _gpu_sums(api, gpu, w, h, spp, chunk=g)
        assert st_g["camera_rays"] == w * h * spp
        _check(got, st_g, want, st_c, f"RT_SLOT_CHUNK={g}")
        assert np.array_equal(got, static)
        for k in ("camera_rays", "closest_rays") + tuple(kg for kg, _ in EVENTS):
            assert st_g[k] == st_0[k], (g, k)


@pytest.mark.parametrize("shard", [(1, 2), (3, 4)])
def test_chunked_deal_on_slot_range_shards(api, gpu, oracle, monkeypatch, shard):
    """Shard 1 of 2: two slots per lane.  Shard 3 of 4: ONE slot per lane -- a level is 256 tasks for 256 lanes, so every lane
    that runs ahead leaves a claim and the runner of that slot goes on with the next chunk itself."""
    w, h, spp = 480, 270, 32
    want, st_c = _oracle_sums(oracle, w, h, spp, shard=shard)
    _chunk(monkeypatch, 0)
    static, st_0 = _gpu_sums(api, gpu, w, h, spp, shard=shard)
    _check(static, st_0, want, st_c, f"static deal, shard {shard}")
    _chunk(monkeypatch, 1)
    got, st_g = _gpu_sums(api, gpu, w, h, spp, shard=shard, chunk=1)
    _check(got, st_g, want, st_c, f"RT_SLOT_CHUNK=1, shard {shard}")
    assert np.array_equal(got, static) and st_g["camera_rays"] == st_0["camera_rays"]


@pytest.mark.parametrize("mode", ["watertight", "reference_walk"])
def test_chunked_deal_in_the_other_reference_mode_builds(api, gpu, oracle, monkeypatch, mode):
    w, h, spp = 480, 270, 32
    flags = {"watertight": api.FLAG_WATERTIGHT, "reference_walk": api.FLAG_REFERENCE_WALK}[mode]
    want, st_c = _oracle_sums(oracle, w, h, spp, watertight=mode == "watertight")
    _chunk(monkeypatch, 0)
    static, st_0 = _gpu_sums(api, gpu, w, h, spp, flags=flags)
    _check(static, st_0, want, st_c, f"static deal, {mode}")
    _chunk(monkeypatch, 3)
    got, st_g = _gpu_sums(api, gpu, w, h, spp, flags=flags, chunk=3)
    _check(got, st_g, want, st_c, f"RT_SLOT_CHUNK=3, {mode}")
    assert np.array_equal(got, static)


def test_knob_without_the_gate_changes_nothing(api, gpu, oracle, monkeypatch):
    """RT_SLOT_CHUNK=1 without RTCUDA_EXPERIMENTAL=1: the launch reports the static deal (the library's default for a frame
    whose chains are 3 rays long), as it does with no knob at all, and the frame is the oracle's."""
    w, h, spp = 480, 270, 32
    want, st_c = _oracle_sums(oracle, w, h, spp)
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "0")
    monkeypatch.delenv("RT_SLOT_CHUNK", raising=False)
    got, st_g = _gpu_sums(api, gpu, w, h, spp, chunk=0)
    _check(got, st_g, want, st_c, "default")
    monkeypatch.setenv("RT_SLOT_CHUNK", "1")
    got_1, st_1 = _gpu_sums(api, gpu, w, h, spp, chunk=0)
    _check(got_1, st_1, want, st_c, "RT_SLOT_CHUNK=1 without the gate")
    assert np.array_equal(got_1, got)
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "1")
    _gpu_sums(api, gpu, w, h, spp, chunk=1)  # (and with the gate the same knob is honoured)


def test_default_deal_on_the_headline_frame(api, gpu, monkeypatch):
    """C2 (1920 x 1080 x 256, chains of 506 rays) with no knob: the launch plan picks the chunked deal, G = ceil(506 / 8) = 64,
    k_paths<PathsChunked> runs it, and the frame's event totals are the committed oracle totals.  One frame, 0.1 s of GPU."""
    import json
    import os
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "0")
    monkeypatch.delenv("RT_SLOT_CHUNK", raising=False)
    w, h, spp = 1920, 1080, 256
    here = os.path.dirname(os.path.abspath(__file__))
    frame = [f for f in json.load(open(os.path.join(here, "golden", "full_size_event_totals.json")))["frames"]
             if (f["scene"], f["spp"]) == ("full_bsdf", spp)][0]
    _, st = _gpu_sums(api, gpu, w, h, spp, chunk=64)
    assert st["camera_rays"] == w * h * spp
    for k, v in frame["oracle_literal"].items():
        assert st[k] == v, (k, st[k], v)
