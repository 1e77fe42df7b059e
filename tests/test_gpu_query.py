"""Ray queries on device buffers (rt_query_closest_device / rt_query_any_device) against the CPU oracle.  Run with -m gpu.

The bar is the project's usual one: equal bits, every ray.  Rays are made with tests/raygen.py, uploaded with torch, traced
from the tensors' device pointers and compared with OracleScene.trace_closest / trace_any -- the literal oracle for flags 0
and RT_FLAG_REFERENCE_WALK, a set_watertight(True) oracle scene for RT_FLAG_WATERTIGHT.  A miss must read t = u = v = 0.
No ray is left out of any comparison, and nothing here provokes a device fault: the validation cases are error returns."""
import dataclasses

import numpy as np
import pytest

from conftest import default_camera, oracle_scene
import raygen
from test_scene_update_host import deform
from test_gpu_parity import KNOWN_MISS_O, KNOWN_MISS_D, _oracle_ray_log
from test_gpu_scene_update import _rays as far_origin_rays

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028234663852886e38)
SENTINEL = -12345


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _flag_modes(api):
    return [(0, False), (api.FLAG_REFERENCE_WALK, False), (api.FLAG_WATERTIGHT, True)]


def _check_closest(gpu, cpu, o, d, tmax=None, flags=0, what=""):
    """Every ray: the oracle's triangle; t, u, v bit-equal where it hits, all zero where it misses.  Returns the oracle's
    answer."""
    n = len(o)
    want = cpu.trace_closest(o, d, np.full(n, FLT_MAX, np.float32) if tmax is None else tmax)
    hit, t, u, v = (x.cpu().numpy() for x in gpu.query_closest(_dev(o), _dev(d), None if tmax is None else _dev(tmax), flags=flags))
    assert hit.shape == (n,) and t.shape == (n,)
    bad = np.where(hit != want[0])[0]
    assert len(bad) == 0, f"{what} flags {flags}: {len(bad)} of {n} rays disagree on the triangle, first {bad[:8]}"
    h = want[0] >= 0
    for name, got, ref in (("t", t, want[1]), ("u", u, want[2]), ("v", v, want[3])):
        assert np.array_equal(_bits(got[h]), _bits(ref[h])), f"{what} flags {flags}: {name} differs on a hit"
        assert not _bits(got[~h]).any(), f"{what} flags {flags}: {name} is not zero on a miss"
    return want


def _check_any(gpu, cpu, o, d, tmax, excluded, flags=0, tmax_null=False, excluded_null=False):
    occ = gpu.query_any(_dev(o), _dev(d), None if tmax_null else _dev(tmax), None if excluded_null else _dev(excluded), flags=flags)
    want = cpu.trace_any(o, d, tmax, excluded)
    assert np.array_equal(occ.cpu().numpy(), want), (flags, tmax_null, excluded_null)
    return want


def _any_batch(cpu, arrays, o, d, seed):
    """The recipe of test_trace_any_matches_oracle: bounce rays, tmax uniform in (0.05, 1.2), the excluded triangle drawn from
    the light triangles and -1."""
    c = cpu.trace_closest(o, d, np.full(len(o), FLT_MAX, np.float32))
    o2, d2 = raygen.bounce_rays(o, d, c[1], c[0] >= 0, seed=seed)
    rng = np.random.default_rng(seed + 1)
    tm = rng.uniform(0.05, 1.2, len(o2)).astype(np.float32)
    light_tris = np.where(arrays.tri_light >= 0)[0]
    excl = rng.choice(np.concatenate([light_tris, [-1]]), len(o2)).astype(np.int32)
    return o2, d2, tm, excl


# ---- 1, 2, 3: batches x scenes x builders x flags
@pytest.mark.parametrize("device_bvh", [False, True], ids=["host-sah", "device-ploc"])
@pytest.mark.parametrize("variant", ["matte", "full_bsdf"])
def test_closest_and_any_match_the_oracle(api, oracle, variant, device_bvh):
    from rtcuda_amd import scenes
    arrays = scenes.cornell_bunny(variant)
    gpu = api.Scene(arrays, device_bvh=device_bvh)
    cam = default_camera(oracle, 16 / 9)
    o, d = raygen.camera_rays(cam, 1920, 1080, 200_000, seed=11)
    o3, d3 = raygen.axis_aligned_rays(50_000, seed=13)
    of, df = far_origin_rays(api, (1.0, np.zeros(3)))
    of, df = of[-20_000:], df[-20_000:]  # the aimed rays from 30 - 60 scene sizes away
    for flags, watertight in _flag_modes(api):
        cpu = oracle_scene(oracle, variant, watertight)
        c = _check_closest(gpu, cpu, o, d, flags=flags, what="camera")
        assert 0.2 < (c[0] >= 0).mean() < 0.8
        o2, d2 = raygen.bounce_rays(o, d, c[1], c[0] >= 0, seed=12)
        c2 = _check_closest(gpu, cpu, o2, d2, flags=flags, what="bounce")
        assert 0.2 < (c2[0] >= 0).mean() < 0.8
        tm = np.random.default_rng(5).uniform(0.05, 1.5, len(o2)).astype(np.float32)
        _check_closest(gpu, cpu, o2, d2, tmax=tm, flags=flags, what="bounce, finite tmax")
        _check_closest(gpu, cpu, o3, d3, flags=flags, what="axis-aligned")
        cf = _check_closest(gpu, cpu, of, df, flags=flags, what="far origins")  # (re-pads through the device-reduced radius)
        assert (cf[0] >= 0).mean() > 0.5
        # any hit
        cam1 = default_camera(oracle, 1.0)
        oa, da = raygen.camera_rays(cam1, 512, 512, 100_000, seed=21)
        o4, d4, tm4, excl = _any_batch(cpu, arrays, oa, da, seed=22)
        occ = _check_any(gpu, cpu, o4, d4, tm4, excl, flags)
        assert 0.05 < occ.mean() < 0.95
        _check_any(gpu, cpu, o4, d4, tm4, np.full(len(o4), -1, np.int32), flags, excluded_null=True)
        _check_any(gpu, cpu, o4, d4, np.full(len(o4), FLT_MAX, np.float32), excl, flags, tmax_null=True)
        _check_any(gpu, cpu, of, df, np.full(len(of), FLT_MAX, np.float32), np.full(len(of), -1, np.int32), flags)
    gpu.close()


def test_after_update_device_and_after_rebuild(api, oracle, bunny_matte):
    """Moved vertices: refit (rt_scene_update_device, from a torch tensor), then a new tree (rt_scene_rebuild: the leaf order
    changes, and with it the device copy of the inverse order the excluded triangle goes through) -- the answers are those of
    an oracle scene made from the same vertices."""
    moved = deform(bunny_matte.tris)
    arrays = dataclasses.replace(bunny_matte, tris=moved)
    gpu = api.Scene(bunny_matte)
    cam = default_camera(oracle, 16 / 9)
    o, d = raygen.camera_rays(cam, 1920, 1080, 100_000, seed=31)
    cpu0 = oracle.scene(bunny_matte)
    o4, d4, tm4, excl = _any_batch(cpu0, bunny_matte, o, d, seed=32)
    _check_any(gpu, cpu0, o4, d4, tm4, excl)  # (makes the inverse order of the FIRST tree)
    verts = _dev(moved)
    gpu.update_device(verts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    for step in ("refit", "rebuild"):
        if step == "rebuild":
            gpu.rebuild()
        for flags, watertight in _flag_modes(api):
            cpu = oracle.scene(arrays).set_watertight(watertight)
            c = _check_closest(gpu, cpu, o, d, flags=flags, what=step)
            assert 0.2 < (c[0] >= 0).mean() < 0.8
            o5, d5, tm5, excl5 = _any_batch(cpu, arrays, o, d, seed=33)
            occ = _check_any(gpu, cpu, o5, d5, tm5, excl5, flags)
            assert 0.05 < occ.mean() < 0.95
            # shadow-ray style: the ray starts ON its excluded triangle, so a wrong remap flips the answer
            h = c[0] >= 0
            o6, d6 = raygen.bounce_rays(o, d, c[1], h, seed=34, eps=0.0)
            occ6 = _check_any(gpu, cpu, o6, d6, np.full(len(o6), FLT_MAX, np.float32), c[0][h].astype(np.int32), flags)
            assert 0.05 < occ6.mean() < 0.95
    gpu.close()


# ---- 4, 8: the oracle's ray log, the experiment knobs, the rare path
@pytest.mark.parametrize("watertight", [False, True], ids=["default-vs-literal", "watertight-flag-vs-watertight"])
@pytest.mark.parametrize("env", [{}, {"RT_BVH_WIDE": "0"}, {"RT_STACK_CAP": "2"}], ids=["wide", "pairs", "wide-overflow"])
def test_oracle_ray_log_through_the_device_queries(api, oracle, bunny_matte, monkeypatch, env, watertight):
    log = _oracle_ray_log(oracle, bunny_matte, watertight)
    flags = api.FLAG_WATERTIGHT if watertight else 0
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gpu = api.Scene(bunny_matte)
    o = np.concatenate([log["closest_o"], KNOWN_MISS_O])
    d = np.concatenate([log["closest_d"], KNOWN_MISS_D])
    want_tri = np.concatenate([log["closest_tri"], [log["miss_tri"]]]).astype(np.int32)
    want_t = np.concatenate([log["closest_t"], [log["miss_t"]]]).astype(np.float32)
    hit, t, u, v = (x.cpu().numpy() for x in gpu.query_closest(_dev(o), _dev(d), flags=flags))
    assert np.array_equal(hit, want_tri)
    h = want_tri >= 0
    assert np.array_equal(_bits(t[h]), _bits(want_t[h]))
    assert not _bits(t[~h]).any() and not _bits(u[~h]).any() and not _bits(v[~h]).any()
    counters = gpu.query_counters()
    if watertight:
        assert counters == {"retraced": 0, "lost": 0, "tied": 0}
    else:
        assert counters["retraced"] >= 1 and counters["lost"] >= 1
    occ = gpu.query_any(_dev(log["any_o"]), _dev(log["any_d"]), _dev(log["any_tmax"]), _dev(log["any_excluded"].astype(np.int32)), flags=flags)
    assert np.array_equal(occ.cpu().numpy(), log["any_occluded"])
    assert len(o) > 500_000 and len(log["any_o"]) > 200_000
    gpu.close()


def test_rare_path_counters_on_the_known_miss_ray(api, oracle, bunny_matte):
    """The one ray of the log whose nearest accepted hit the reference's box test loses: the default query re-traces it
    literally (and says so), RT_FLAG_WATERTIGHT has no rare path; each answers what its oracle mode answers."""
    gpu = api.Scene(bunny_matte)
    o, d = _dev(KNOWN_MISS_O), _dev(KNOWN_MISS_D)
    for watertight in (False, True):
        log = _oracle_ray_log(oracle, bunny_matte, watertight)
        hit, t, _, _ = gpu.query_closest(o, d, flags=api.FLAG_WATERTIGHT if watertight else 0)
        assert int(hit[0]) == log["miss_tri"] == (69462 if watertight else 69458)
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(np.array([log["miss_t"]], np.float32)))
        c = gpu.query_counters()
        if watertight:
            assert c == {"retraced": 0, "lost": 0, "tied": 0}
        else:
            assert c["retraced"] == 1 and c["lost"] >= 1
    gpu.close()


# ---- 5: size
def test_four_million_rays_in_one_call(api, oracle, bunny_matte):
    """Several chunks per wave and a ragged tail: the ray log tiled to 4 194 304 + 37 rays, the oracle run once on the log."""
    log = _oracle_ray_log(oracle, bunny_matte, False)
    gpu = api.Scene(bunny_matte)
    n = (1 << 22) + 37
    m = len(log["closest_o"])
    idx = torch.arange(n, device="cuda") % m
    o, d = _dev(log["closest_o"])[idx].contiguous(), _dev(log["closest_d"])[idx].contiguous()
    hit, t, u, v = gpu.query_closest(o, d)
    want_tri, want_t = _dev(log["closest_tri"].astype(np.int32))[idx], _dev(log["closest_t"].astype(np.float32))[idx]
    assert torch.equal(hit, want_tri)
    h = want_tri >= 0
    assert torch.equal(t[h].view(torch.int32), want_t[h].view(torch.int32))
    assert not t[~h].view(torch.int32).any() and not u[~h].view(torch.int32).any() and not v[~h].view(torch.int32).any()
    ma = len(log["any_o"])
    ia = torch.arange(n, device="cuda") % ma
    occ = gpu.query_any(_dev(log["any_o"])[ia].contiguous(), _dev(log["any_d"])[ia].contiguous(), _dev(log["any_tmax"])[ia].contiguous(),
                        _dev(log["any_excluded"].astype(np.int32))[ia].contiguous())
    assert torch.equal(occ, _dev(log["any_occluded"].astype(np.int32))[ia])
    gpu.close()


class _GuardedOutputs:
    """query_closest / query_any of a scene through the device entry points, into buffers of the caller's that are 64
    elements longer than the batch and pre-filled with SENTINEL: what lies past the batch must come back untouched."""

    def __init__(self, gpu):
        self.gpu = gpu

    @staticmethod
    def _buffers(n, dtypes):
        return [torch.full((n + 64,), SENTINEL, dtype=dt, device="cuda") for dt in dtypes]

    @staticmethod
    def _cut(n, bufs):
        torch.cuda.synchronize()
        for b in bufs:
            assert bool((b[n:] == SENTINEL).all()), f"{n} rays: an output was written past the batch"
        return [b[:n] for b in bufs]

    def query_closest(self, o, d, tmax=None, flags=0):
        n = len(o)
        bufs = self._buffers(n, [torch.int32, torch.float32, torch.float32, torch.float32])
        self.gpu.query_closest_device(o.data_ptr(), d.data_ptr(), 0 if tmax is None else tmax.data_ptr(), n,
                                      *(b.data_ptr() for b in bufs), flags)
        return tuple(self._cut(n, bufs))

    def query_any(self, o, d, tmax=None, excluded=None, flags=0):
        n = len(o)
        bufs = self._buffers(n, [torch.int32])
        self.gpu.query_any_device(o.data_ptr(), d.data_ptr(), 0 if tmax is None else tmax.data_ptr(),
                                  0 if excluded is None else excluded.data_ptr(), n, bufs[0].data_ptr(), flags)
        return self._cut(n, bufs)[0]


def test_batches_around_one_chunk_and_one_wave(api, oracle, bunny_matte):
    """The hand-out of chunks at its edges: one lane, one short of a chunk of 64, exactly one, one over, two chunks and a bit,
    and a count that gives most waves of the grid nothing and a few of them one chunk.  Closest hit under the three flag
    modes, any hit with and without the excluded triangles; every answer the oracle's, nothing written past the batch."""
    gpu = api.Scene(bunny_matte)
    guarded = _GuardedOutputs(gpu)
    o_all, d_all = raygen.camera_rays(default_camera(oracle, 16 / 9), 1920, 1080, 4097, seed=71)
    for n in (1, 63, 64, 65, 129, 4097):
        o, d = o_all[:n], d_all[:n]
        for flags, watertight in _flag_modes(api):
            cpu = oracle_scene(oracle, "matte", watertight)
            _check_closest(guarded, cpu, o, d, flags=flags, what=f"{n} rays")
        cpu = oracle_scene(oracle, "matte", False)
        # (bounce rays leave the hits only -- the first ray of this seed hits --: tiled to the count under test)
        o2, d2, tm, excl = (np.ascontiguousarray(x[np.arange(n) % len(x)]) for x in _any_batch(cpu, bunny_matte, o, d, seed=72))
        _check_any(guarded, cpu, o2, d2, tm, excl)
        _check_any(guarded, cpu, o2, d2, tm, np.full(n, -1, np.int32), excluded_null=True)
    gpu.close()


# ---- 6: stream order
def test_query_is_ordered_on_the_callers_stream(api, oracle, bunny_matte):
    """On a non-default stream: a torch kernel writes the rays, the query runs on that stream, a torch kernel consumes hit_tri;
    no synchronise in between."""
    gpu = api.Scene(bunny_matte)
    cpu = oracle.scene(bunny_matte)
    o, d = raygen.camera_rays(default_camera(oracle, 16 / 9), 1920, 1080, 300_000, seed=41)
    want = cpu.trace_closest(o, d, np.full(len(o), FLT_MAX, np.float32))
    o_src, d_src = _dev(o), _dev(d)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        o_dev = torch.zeros_like(o_src)
        d_dev = torch.zeros_like(d_src)
        for _ in range(20):  # (work queued ahead of the rays' producer)
            o_dev = o_dev * 0.5
        o_dev = o_dev + o_src
        d_dev = d_dev + d_src
        hit, t, _, _ = gpu.query_closest(o_dev, d_dev)
        n_hit = (hit >= 0).sum()
        plus_one = hit + 1
    s.synchronize()
    assert np.array_equal(hit.cpu().numpy(), want[0])
    assert int(n_hit) == int((want[0] >= 0).sum())
    assert np.array_equal(plus_one.cpu().numpy(), want[0] + 1)
    gpu.close()


# ---- 7: validation
def test_bad_arguments_are_errors_and_write_nothing(api, oracle, bunny_matte):
    gpu = api.Scene(bunny_matte)
    cpu = oracle.scene(bunny_matte)
    o, d = raygen.camera_rays(default_camera(oracle, 16 / 9), 1920, 1080, 10_000, seed=51)
    n = len(o)
    o_dev = _dev(o)
    hit = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    t = torch.full((n,), float(SENTINEL), dtype=torch.float32, device="cuda")
    occ = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((hit == SENTINEL).all()) and bool((t == float(SENTINEL)).all()) and bool((occ == SENTINEL).all())

    def closest(d_dev, flags=0, count=n, hit_ptr=None):
        gpu.query_closest_device(o_dev.data_ptr(), d_dev.data_ptr(), 0, count, hit.data_ptr() if hit_ptr is None else hit_ptr,
                                 t.data_ptr(), 0, 0, flags)

    for bad, k in ((np.nan, 1), (np.float32(2.0 ** 126), 1), (-np.float32(2.0 ** 126), 2), (np.inf, 1), (-np.inf, 3)):
        db = d.copy()
        rows = np.random.default_rng(int(k)).choice(n, k, replace=False)
        db[rows, rows % 3] = bad
        d_dev = _dev(db)
        with pytest.raises(api.RtError, match=f"rt_query_closest_device: {k} of {n} directions are not finite or reach 2\\^126"):
            closest(d_dev)
        with pytest.raises(api.RtError, match=f"rt_query_any_device: {k} of {n} directions"):
            gpu.query_any_device(o_dev.data_ptr(), d_dev.data_ptr(), 0, 0, n, occ.data_ptr())
        assert untouched()
    d_dev = _dev(d)
    with pytest.raises(api.RtError, match="exclude each other"):
        closest(d_dev, flags=api.FLAG_REFERENCE_WALK | api.FLAG_WATERTIGHT)
    with pytest.raises(api.RtError, match="outside 0 .. 2\\^30"):
        closest(d_dev, count=-1)
    with pytest.raises(api.RtError, match="outside 0 .. 2\\^30"):
        closest(d_dev, count=(1 << 30) + 1)
    L = api.lib()
    assert L.rt_query_closest_device(gpu.h, 0, n, o_dev.data_ptr(), d_dev.data_ptr(), None, None, t.data_ptr(), None, None, None) != 0
    assert "null d_hit_tri" in L.rt_last_error().decode()
    assert L.rt_query_any_device(gpu.h, 0, n, o_dev.data_ptr(), d_dev.data_ptr(), None, None, None, None) != 0
    assert "null d_occluded" in L.rt_last_error().decode()
    assert untouched()
    # the largest legal component, and a non-finite ORIGIN: legal, the ray misses
    ob = o.copy()
    ob[0, 0], ob[1, 1], ob[2, 2] = np.nan, np.inf, -np.inf
    got = gpu.query_closest(_dev(ob), d_dev)
    want = cpu.trace_closest(o, d, np.full(n, FLT_MAX, np.float32))
    got_hit = got[0].cpu().numpy()
    assert (got_hit[:3] == -1).all() and not got[1][:3].view(torch.int32).any()
    assert np.array_equal(got_hit[3:], want[0][3:])
    gpu.close()


# ---- 9: n = 0 and optional outputs
def test_empty_batch_and_optional_outputs(api, oracle, bunny_matte):
    gpu = api.Scene(bunny_matte)
    cpu = oracle.scene(bunny_matte)
    gpu.query_closest_device(0, 0, 0, 0, 0)
    gpu.query_any_device(0, 0, 0, 0, 0, 0)
    e3, e1 = torch.zeros((0, 3), device="cuda"), torch.zeros(0, device="cuda")
    assert all(len(x) == 0 for x in gpu.query_closest(e3, e3, e1))
    assert len(gpu.query_any(e3, e3)) == 0
    o, d = raygen.camera_rays(default_camera(oracle, 16 / 9), 1920, 1080, 5_000, seed=61)
    n = len(o)
    want = cpu.trace_closest(o, d, np.full(n, FLT_MAX, np.float32))
    o_dev, d_dev = _dev(o), _dev(d)
    hit = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    t, u, v = (torch.full((n,), float(SENTINEL), dtype=torch.float32, device="cuda") for _ in range(3))
    gpu.query_closest_device(o_dev.data_ptr(), d_dev.data_ptr(), 0, n, hit.data_ptr(), t.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    assert np.array_equal(hit.cpu().numpy(), want[0])
    h = want[0] >= 0
    assert np.array_equal(_bits(t.cpu().numpy()[h]), _bits(want[1][h]))
    assert bool((u == float(SENTINEL)).all()) and bool((v == float(SENTINEL)).all())  # not wanted: not written
    gpu.query_closest_device(o_dev.data_ptr(), d_dev.data_ptr(), 0, n, hit.data_ptr())  # only the triangle
    assert np.array_equal(hit.cpu().numpy(), want[0])
    gpu.close()


# ---- 10: the host-pointer form (rt_trace_closest / rt_trace_any) is the device query's kernel behind copies
HOOK_SIZES = (1, 63, 64, 65, 4099)  # one lane; one short of a chunk, one chunk, one over; several chunks and a ragged tail


_hook_cases = {}


def _hook_case(oracle, bunny_matte, name):
    """(arrays, literal oracle scene, closest-hit rays, any-hit batch) of the bare Cornell box / the box with the bunny.  The
    4099 camera rays of this seed hold a hit and a miss among the first 63 on both scenes in all three hit modes, and the
    any-hit batch made from them an occluded and a free ray (checked on the CPU oracle when the seeds were chosen; asserted
    again by the test that relies on it)."""
    if name not in _hook_cases:
        from rtcuda_amd import scenes
        arrays = scenes.cornell_bunny("matte", bunny=False) if name == "box" else bunny_matte
        cpu = oracle.scene(arrays) if name == "box" else oracle_scene(oracle, "matte", False)
        o, d = raygen.camera_rays(default_camera(oracle, 16 / 9), 1920, 1080, HOOK_SIZES[-1], seed=81)
        batch = tuple(np.ascontiguousarray(x[np.arange(len(o)) % len(x)]) for x in _any_batch(cpu, arrays, o, d, seed=82))
        _hook_cases[name] = arrays, cpu, (o, d), batch
    return _hook_cases[name]


both_scenes = pytest.mark.parametrize("name", ["box", "bunny"])


@both_scenes
def test_hooks_give_the_device_queries_answers(api, oracle, bunny_matte, name):
    arrays, _, (o_all, d_all), (o2_all, d2_all, tm_all, excl_all) = _hook_case(oracle, bunny_matte, name)
    gpu = api.Scene(arrays)
    for flags, _ in _flag_modes(api):
        for n in HOOK_SIZES:
            o, d = o_all[:n], d_all[:n]
            tm = np.full(n, FLT_MAX, np.float32)
            q_hit, q_t, q_u, q_v = (x.cpu().numpy() for x in gpu.query_closest(_dev(o), _dev(d), _dev(tm), flags=flags))
            h_hit, h_t, h_u, h_v = gpu.trace_closest(o, d, tm, flags=flags)
            assert np.array_equal(h_hit, q_hit), (flags, n)
            h = q_hit >= 0
            for what, got, ref in (("t", h_t, q_t), ("u", h_u, q_u), ("v", h_v, q_v)):
                assert np.array_equal(_bits(got[h]), _bits(ref[h])), f"flags {flags}, {n} rays: {what} differs on a hit"
                assert not _bits(got[~h]).any(), f"flags {flags}, {n} rays: the hook's {what} is not zero on a miss"
            o2, d2, tm2, excl = o2_all[:n], d2_all[:n], tm_all[:n], excl_all[:n]
            q_occ = gpu.query_any(_dev(o2), _dev(d2), _dev(tm2), _dev(excl), flags=flags).cpu().numpy()
            h_occ = gpu.trace_any(o2, d2, tm2, excl, flags=flags)
            assert np.array_equal(h_occ, q_occ), (flags, n)
            if n >= 63:
                assert h.any() and not h.all(), (flags, n)
                assert q_occ.any() and not q_occ.all(), (flags, n)
    gpu.close()


@both_scenes
def test_hook_exclusions_out_of_range_exclude_nothing(api, oracle, bunny_matte, name):
    """Shadow-ray style rays, each starting ON the triangle it names, so that whether the exclusion is honoured decides the answer."""
    arrays, cpu, (o, d), _ = _hook_case(oracle, bunny_matte, name)
    gpu = api.Scene(arrays)
    c = cpu.trace_closest(o, d, np.full(len(o), FLT_MAX, np.float32))
    h = c[0] >= 0
    o6, d6 = raygen.bounce_rays(o, d, c[1], h, seed=83, eps=0.0)
    own = c[0][h].astype(np.int32)
    n = len(o6)
    tm = np.full(n, FLT_MAX, np.float32)
    n_tris = len(arrays.tris)
    free = gpu.query_any(_dev(o6), _dev(d6), _dev(tm), None).cpu().numpy()
    for value in (-1, n_tris, np.iinfo(np.int32).min, np.iinfo(np.int32).max):
        assert np.array_equal(gpu.trace_any(o6, d6, tm, np.full(n, value, np.int32)), free), value
    in_range = gpu.query_any(_dev(o6), _dev(d6), _dev(tm), _dev(own)).cpu().numpy()
    assert np.array_equal(gpu.trace_any(o6, d6, tm, own), in_range)
    assert np.array_equal(in_range, cpu.trace_any(o6, d6, tm, own))
    assert (in_range != free).any()  # (the exclusion matters on these rays)
    mixed = own.copy()
    mixed[1::4], mixed[2::4], mixed[3::4] = n_tris, np.iinfo(np.int32).min, np.iinfo(np.int32).max
    assert np.array_equal(gpu.trace_any(o6, d6, tm, mixed), np.where(np.arange(n) % 4 == 0, in_range, free))
    gpu.close()


def test_hooks_leave_the_last_querys_counters(api, oracle, bunny_matte):
    """rt_query_last_counters speaks of the last QUERY: the known-miss ray leaves a re-trace there, a hook call on other rays
    (which re-traces nothing) does not take it away."""
    _, _, (o, d), (o2, d2, tm, excl) = _hook_case(oracle, bunny_matte, "bunny")
    gpu = api.Scene(bunny_matte)
    gpu.query_closest(_dev(KNOWN_MISS_O), _dev(KNOWN_MISS_D))
    before = gpu.query_counters()
    assert before["retraced"] == 1 and before["lost"] >= 1
    gpu.trace_closest(o, d, np.full(len(o), FLT_MAX, np.float32))
    assert gpu.query_counters() == before
    gpu.trace_any(o2, d2, tm, excl)
    assert gpu.query_counters() == before
    gpu.close()


@both_scenes
def test_hook_query_hook_share_the_scenes_scratch(api, oracle, bunny_matte, name):
    """The inverse leaf order, the overflow stacks and the scratch words are the scene's, made by whichever call comes first:
    a hook, a device query, a hook again on a fresh scene, each the oracle's."""
    arrays, cpu, (o, d), (o2, d2, tm, excl) = _hook_case(oracle, bunny_matte, name)
    gpu = api.Scene(arrays)
    want_occ = cpu.trace_any(o2, d2, tm, excl)
    assert np.array_equal(gpu.trace_any(o2, d2, tm, excl), want_occ)
    _check_any(gpu, cpu, o2, d2, tm, excl)
    full = np.full(len(o), FLT_MAX, np.float32)
    want = cpu.trace_closest(o, d, full)
    hit, t, u, v = gpu.trace_closest(o, d, full)
    assert np.array_equal(hit, want[0])
    h = want[0] >= 0
    for got, ref in ((t, want[1]), (u, want[2]), (v, want[3])):
        assert np.array_equal(_bits(got[h]), _bits(ref[h]))
    assert np.array_equal(gpu.trace_any(o2, d2, tm, excl), want_occ)
    gpu.close()


def test_hook_through_the_overflow_stack(api, oracle, bunny_matte, monkeypatch):
    """RT_STACK_CAP=2 sends every traversal of the bunny's tree through the overflow columns of the scene's query state."""
    _, _, (o, d), (o2, d2, tm, excl) = _hook_case(oracle, bunny_matte, "bunny")
    full = np.full(len(o), FLT_MAX, np.float32)
    gpu = api.Scene(bunny_matte)
    plain = gpu.trace_closest(o, d, full), gpu.trace_any(o2, d2, tm, excl)
    gpu.close()
    monkeypatch.setenv("RT_STACK_CAP", "2")
    small = api.Scene(bunny_matte)
    got = small.trace_closest(o, d, full), small.trace_any(o2, d2, tm, excl)
    small.close()
    assert np.array_equal(got[0][0], plain[0][0])
    for a, b in zip(got[0][1:], plain[0][1:]):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(got[1], plain[1])
