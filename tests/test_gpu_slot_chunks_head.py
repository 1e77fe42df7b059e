"""GPU tests of k_paths<PathsChunked>'s static head and LDS semaphores (rt_slot_chunks.h): a lane runs its first
`head` slot sets as the static deal does, and only the remaining sets are dealt G camera rays at a time, handed over through
16-bit semaphore fields in the workgroup's LDS.  Nothing a ray does may change: for every head the event totals and
RT_FLAG_DETERMINISTIC's int64 sums must EQUAL the CPU oracle's and those of RT_SLOT_CHUNK=0, the static deal -- every path,
every random number, every contribution.  (tests/test_gpu_slot_chunks.py runs the same kernel at the default head.)
Run with -m gpu.  All comparisons are exact."""
import numpy as np
import pytest

# (the oracle's frames are shared with the older file: a frame both need is computed once per session)
from test_gpu_slot_chunks import EVENTS, _check, _gpu_sums, _oracle_sums

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


def _deal(monkeypatch, g, head=None):
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "1")
    monkeypatch.setenv("RT_SLOT_CHUNK", str(g))
    if head is None:
        monkeypatch.delenv("RT_SLOT_HEAD", raising=False)
    else:
        monkeypatch.setenv("RT_SLOT_HEAD", str(head))


_static_cache = {}


def _static(api, gpu, monkeypatch, w, h, spp, flags=0, shard=(0, 1)):
    """The static deal's sums and stats of a frame (k_paths, RT_SLOT_CHUNK=0), rendered once."""
    key = (w, h, spp, flags, shard)
    if key not in _static_cache:
        _deal(monkeypatch, 0)
        got, st = _gpu_sums(api, gpu, w, h, spp, flags=flags, shard=shard)
        got.setflags(write=False)
        _static_cache[key] = (got, st)
    return _static_cache[key]


def _same_as_static(got, st_g, static, st_0, what):
    assert np.array_equal(got, static), what
    for k in ("camera_rays", "closest_rays") + tuple(kg for kg, _ in EVENTS):
        assert st_g[k] == st_0[k], (what, k, st_g[k], st_0[k])


@pytest.mark.parametrize("g", [1, 3])
def test_every_head_equals_the_oracle_and_the_static_deal(api, gpu, oracle, monkeypatch, g):
    """480 x 270 x 32 on the full pool: four slots per lane, chains of 3 rays.  Head 0 deals every set, head 3 leaves one dealt
    slot per lane-entry (every task finds its slot running or banked by its own lane's neighbours: claims)."""
    w, h, spp = 480, 270, 32
    want, st_c = _oracle_sums(oracle, w, h, spp)
    static, st_0 = _static(api, gpu, monkeypatch, w, h, spp)
    _check(static, st_0, want, st_c, "static deal")
    for head in (0, 1, 2, 3):
        _deal(monkeypatch, g, head)
        got, st_g = _gpu_sums(api, gpu, w, h, spp, chunk=g)
        assert st_g["slot_head"] == head
        assert st_g["camera_rays"] == w * h * spp
        _check(got, st_g, want, st_c, f"RT_SLOT_CHUNK={g} RT_SLOT_HEAD={head}")
        _same_as_static(got, st_g, static, st_0, (g, head))


def test_ragged_chains_behind_a_static_head(api, gpu, oracle, monkeypatch):
    """300 x 200 x 48: spp does not divide W, and slots differ in their number of rays."""
    w, h, spp = 300, 200, 48
    want, st_c = _oracle_sums(oracle, w, h, spp)
    static, st_0 = _static(api, gpu, monkeypatch, w, h, spp)
    _deal(monkeypatch, 2, 2)
    got, st_g = _gpu_sums(api, gpu, w, h, spp, chunk=2)
    assert st_g["slot_head"] == 2
    _check(got, st_g, want, st_c, "RT_SLOT_CHUNK=2 RT_SLOT_HEAD=2")
    _same_as_static(got, st_g, static, st_0, "ragged")


@pytest.mark.parametrize("shard,head", [((0, 1), 2), ((3, 4), 0)])
def test_long_chains_at_the_default_head(api, gpu, oracle, monkeypatch, shard, head):
    """256 x 128 x 256: 8 generations, so chains of 7 rays inside k_paths<PathsChunked> (the eighth generation runs in lockstep) and 6
    hand-overs per dealt slot at G = 1.  The whole frame has four
    slots per lane (default head 2); shard 3 of 4 has ONE slot per lane (head 0): every lane that runs ahead leaves a claim, and
    the claims pile up in neighbouring 16-bit fields."""
    w, h, spp = 256, 128, 256
    want, st_c = _oracle_sums(oracle, w, h, spp, shard=shard)
    static, st_0 = _static(api, gpu, monkeypatch, w, h, spp, shard=shard)
    _check(static, st_0, want, st_c, f"static deal, shard {shard}")
    _deal(monkeypatch, 1)
    got, st_g = _gpu_sums(api, gpu, w, h, spp, shard=shard, chunk=1)
    assert st_g["slot_head"] == head
    _check(got, st_g, want, st_c, f"RT_SLOT_CHUNK=1, shard {shard}")
    _same_as_static(got, st_g, static, st_0, shard)


@pytest.mark.parametrize("mode", ["watertight", "reference_walk"])
def test_static_head_in_the_other_reference_mode_builds(api, gpu, oracle, monkeypatch, mode):
    w, h, spp = 480, 270, 32
    flags = {"watertight": api.FLAG_WATERTIGHT, "reference_walk": api.FLAG_REFERENCE_WALK}[mode]
    want, st_c = _oracle_sums(oracle, w, h, spp, watertight=mode == "watertight")
    static, st_0 = _static(api, gpu, monkeypatch, w, h, spp, flags=flags)
    _check(static, st_0, want, st_c, f"static deal, {mode}")
    _deal(monkeypatch, 1, 1)
    got, st_g = _gpu_sums(api, gpu, w, h, spp, flags=flags, chunk=1)
    assert st_g["slot_head"] == 1
    _check(got, st_g, want, st_c, f"RT_SLOT_CHUNK=1 RT_SLOT_HEAD=1, {mode}")
    _same_as_static(got, st_g, static, st_0, mode)
