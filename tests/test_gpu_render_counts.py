"""GPU tests of the counted frames (rt_render_counts_fixed) and what they are used with (rt_normalize_counts_fixed,
rt_post_process_counts_fixed, rt_sample_allocate).  Run with -m gpu.

Pixel p renders the samples first[p] .. first[p] + count[p] - 1 of the w x h x S per-sample frame, so every expected value comes
from the oracle (tests/render_counts_expected.py, held to it by tests/test_render_counts_host.py): the sums are the masked sum of
the oracle's sample frames, or of its keyed tables run by run, which also give the six event totals.  ALL int64 sums EQUAL and
the event totals EQUAL: no tolerance, no masked pixel."""
import numpy as np
import pytest

from conftest import default_camera, oracle_scene, usable_cpus
import render_counts_expected as rc

pytestmark = pytest.mark.gpu

KEYS = rc.KEYS
MAIN = (160, 90, 16)  # whole: 230 400 rays, 450 chunks of 512 ids
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()  # raises if the HIP library is missing: there is no fallback
    return _api


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    return _torch


_gpu_cache = {}


def _gpu(api, variant):
    if variant not in _gpu_cache:
        from rtcuda_amd import scenes
        _gpu_cache[variant] = api.Scene(scenes.cornell_bunny(variant))
    return _gpu_cache[variant]


def _osc(oracle, variant="full_bsdf"):
    return oracle_scene(oracle, variant, True)


def _dev(torch, a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _ev(st):
    return {k: st[k] for k in KEYS}


def _add(evs):
    return {k: sum(e[k] for e in evs) for k in KEYS}


def _render(api, torch, gpu, w, h, S, count, first=None, **kw):
    return gpu.render_counts(api.make_camera(aspect=w / h), w, h, S, _dev(torch, count), first=None if first is None else _dev(torch, first), **kw)


def _assert_sums(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    bad = got != want
    print(what, "sums that differ:", int(bad.sum()), "of", bad.size)
    assert not bad.any(), (what, "sums that differ: %d of %d" % (int(bad.sum()), bad.size), "first (pixel, channel):",
                           np.argwhere(bad)[:6].tolist(), "got", got[bad][:6].tolist(), "want", want[bad][:6].tolist())


_whole = {}


def _oracle_whole(oracle, w, h, S, max_bounces=10, seed=1, variant="full_bsdf"):
    """(sums (w * h, 3) int64, the six event totals) of the oracle's whole per-sample frame; computed once, read-only."""
    key = (variant, w, h, S, max_bounces, seed)
    if key not in _whole:
        want = np.zeros((h, w, 3), np.int64)
        _, _, st = _osc(oracle, variant).render(default_camera(oracle, w / h), w, h, S, max_bounces=max_bounces, seed=seed, threads=usable_cpus(),
                                                fixed_out=want, rng_mode="per_sample")
        want = want.reshape(-1, 3)
        want.setflags(write=False)
        _whole[key] = (want, rc.events_of(st))
    return _whole[key]


def _random_map(w, h, S, seed=3):
    rng = np.random.default_rng(seed)
    count = rng.integers(0, S + 1, w * h)
    first = (rng.random(w * h) * (S - count + 1)).astype(np.int64)
    return first, count


# ---- 1. a whole frame of counts
@pytest.mark.parametrize("w,h,S", [(1, 1, 1), (1, 513, 1), (19, 27, 3), MAIN], ids=lambda v: str(v))
def test_whole_frame_is_the_oracles_per_sample_frame(api, torch, oracle, w, h, S):
    want, ev_c = _oracle_whole(oracle, w, h, S)
    gpu = _gpu(api, "full_bsdf")
    out, st = _render(api, torch, gpu, w, h, S, np.full(w * h, S))
    _assert_sums(out, want, ("whole frame", w, h, S))
    assert _ev(st) == ev_c and st["camera_rays"] == w * h * S
    cam = torch.zeros((w * h, 3), dtype=torch.int64, device="cuda")
    st_c = gpu.render_shard_fixed(api.make_camera(aspect=w / h), w, h, S, 0, 1, cam.data_ptr(), flags=api.FLAG_RNG_PER_SAMPLE)
    torch.cuda.synchronize()
    assert torch.equal(out, cam) and _ev(st_c) == _ev(st)


# ---- 2. varied maps, sums and events
def _small_maps(oracle):
    w, h, S = 9, 7, 8
    first, count = _random_map(w, h, S)
    one = np.zeros(w * h, np.int64)
    one[int(np.argmax(_oracle_whole(oracle, w, h, S)[0].sum(axis=1)))] = S  # (the frame's brightest pixel holds all samples)
    return {"random": (first, count), "one-pixel": (None, one)}


@pytest.mark.parametrize("which", ["random", "one-pixel"])
def test_varied_maps_sums_and_events(api, torch, oracle, which):
    w, h, S = 9, 7, 8
    first, count = _small_maps(oracle)[which]
    want, ev_c = rc.expected_by_tables(oracle, _osc(oracle), w, h, S, first, count)
    assert want.any()
    out, st = _render(api, torch, _gpu(api, "full_bsdf"), w, h, S, count, first)
    _assert_sums(out, want, which)
    assert _ev(st) == ev_c and st["camera_rays"] == int(count.sum())


def test_a_call_equals_the_keyed_table_of_the_same_keys(api, torch, oracle):
    """The third promise, on the device: the random map's keys p * S + k as ONE keyed table with an explicit pixel array is not
    affine in the row, so it goes through rt_render_rays_keyed_fixed_device run by run into one buffer."""
    import raytable_keyed as rk
    w, h, S = 9, 7, 8
    first, count = _random_map(w, h, S)
    gpu = _gpu(api, "full_bsdf")
    out, st = _render(api, torch, gpu, w, h, S, count, first)
    acc = torch.zeros((w * h, 3), dtype=torch.int64, device="cuda")
    evs = []
    for p in np.flatnonzero(count > 0):
        key_first = int(p) * S + int(first[p])
        o, d, pixel = rk.keyed_pinhole_table(oracle, default_camera(oracle, w / h), w, h, S, 1, range(key_first, key_first + int(count[p])))
        _, s = gpu.render_rays_keyed(_dev(torch, o, np.float32), _dev(torch, d, np.float32), w * h, pixel=_dev(torch, pixel), key_first=key_first,
                                     fixed=True, out=acc)
        evs.append(_ev(s))
    assert torch.equal(out, acc) and _add(evs) == _ev(st)


def test_all_zero_counts_render_nothing(api, torch):
    w, h, S = 9, 7, 8
    buf = torch.full((w * h, 3), SENTINEL, dtype=torch.int64, device="cuda")
    samples = torch.full((w * h,), 5, dtype=torch.int32, device="cuda")
    out, st = _render(api, torch, _gpu(api, "full_bsdf"), w, h, S, np.zeros(w * h), samples=samples, out=buf)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and bool((samples == 5).all())
    assert all(st[k] == 0 for k in KEYS) and st["closest_rays"] == 0


# ---- 3. chunk and search edges
def _edge_map():
    count = np.zeros(1300, np.int64)
    count[1100] = 600  # behind a run of pixels without samples longer than a chunk; spans two chunks of 512 ids
    count[1101::2] = 1
    return count


@pytest.mark.parametrize("reverse", [False, True], ids=["as-is", "reversed"])
def test_chunk_and_search_edges(api, torch, oracle, reverse):
    w, h, S = 1, 1300, 600
    count = _edge_map()[::-1].copy() if reverse else _edge_map()
    assert int(count.sum()) == 700 and count[-1 if not reverse else 0] == 1
    want, ev_c = rc.expected_by_tables(oracle, _osc(oracle), w, h, S, None, count)
    out, st = _render(api, torch, _gpu(api, "full_bsdf"), w, h, S, count)
    _assert_sums(out, want, ("edges", reverse))
    assert _ev(st) == ev_c


# ---- 4. a structured map
def _structured_map():
    w, h, S = MAIN
    count = np.full((h, w), 2, np.int64)
    count[30:80, 50:110] = 16  # around the bunny
    count[37, :] = 0
    return count.reshape(-1)


def test_structured_map(api, torch, oracle):
    w, h, S = MAIN
    count = _structured_map()
    want = rc.expected_by_frames(oracle, _osc(oracle), "full_bsdf", w, h, S, None, count)
    assert want[count == 16].any() and not want[count == 0].any()
    out, st = _render(api, torch, _gpu(api, "full_bsdf"), w, h, S, count)
    _assert_sums(out, want, "structured")
    assert st["camera_rays"] == int(count.sum())


# ---- 5. tiling
def test_passes_that_tile_the_samples_add_up_in_any_order(api, torch, oracle):
    w, h, S = MAIN
    want, ev_c = _oracle_whole(oracle, w, h, S)
    n = np.random.default_rng(8).integers(0, 13, w * h)
    assert (n == 0).any() and (n == 12).any()
    passes = [(np.zeros(w * h, np.int64), np.full(w * h, 4)), (np.full(w * h, 4), n), (4 + n, 12 - n)]
    gpu = _gpu(api, "full_bsdf")
    results = []
    for order in (passes, passes[::-1]):
        acc = torch.zeros((w * h, 3), dtype=torch.int64, device="cuda")
        samples = torch.zeros((w * h,), dtype=torch.int32, device="cuda")
        evs = []
        for first, count in order:
            _, st = _render(api, torch, gpu, w, h, S, count, first, samples=samples, out=acc)
            assert st["camera_rays"] == int(count.sum())
            evs.append(_ev(st))
        _assert_sums(acc, want, "tiling")
        assert _add(evs) == ev_c and bool((samples == S).all())
        results.append(acc)
    assert torch.equal(results[0], results[1])


# ---- 6. keys beyond 32 bits
def test_keys_beyond_32_bits(api, torch, oracle):
    w, h, S = 9, 7, 2 ** 31 - 1
    first, count = np.full(w * h, S - 3), np.full(w * h, 3)
    want, ev_c = rc.expected_by_tables(oracle, _osc(oracle), w, h, S, first, count)
    out, st = _render(api, torch, _gpu(api, "full_bsdf"), w, h, S, count, first)
    _assert_sums(out, want, "S = 2^31 - 1")
    assert _ev(st) == ev_c and want.any()


# ---- 7. parameters, builds, trees, scenes
@pytest.mark.parametrize("seed", [0, 2 ** 32, 0xFFFFFFFF00000007], ids=hex)
def test_seeds_whose_high_word_matters(api, torch, oracle, seed):
    w, h, S = 9, 7, 8
    first, count = _random_map(w, h, S)
    want, ev_c = rc.expected_by_tables(oracle, _osc(oracle), w, h, S, first, count, seed=seed)
    out, st = _render(api, torch, _gpu(api, "full_bsdf"), w, h, S, count, first, seed=seed)
    _assert_sums(out, want, ("seed", seed))
    assert _ev(st) == ev_c


@pytest.mark.parametrize("max_bounces", [0, 1, 10])
def test_max_bounces(api, torch, oracle, max_bounces):
    w, h, S = 9, 7, 8
    first, count = _random_map(w, h, S)
    want, ev_c = rc.expected_by_tables(oracle, _osc(oracle), w, h, S, first, count, max_bounces=max_bounces)
    out, st = _render(api, torch, _gpu(api, "full_bsdf"), w, h, S, count, first, max_bounces=max_bounces)
    _assert_sums(out, want, ("max_bounces", max_bounces))
    assert _ev(st) == ev_c and (st["shade_events"] == 0) == (max_bounces == 0)


@pytest.mark.parametrize("blocks", ["512", "64"])
def test_the_few_blocks_build(api, torch, oracle, monkeypatch, blocks):
    """A grid of at most two workgroups per CU launches the MIN_WAVES = 2 build: gen() inside the ADV block, ids tied to slots
    (id = generation * W + slot), each found in the prefix sum over the whole image."""
    monkeypatch.setenv("RT_PATHS_BLOCKS", blocks)
    gpu = _gpu(api, "full_bsdf")
    w, h, S = MAIN
    count = _structured_map()
    out, st = _render(api, torch, gpu, w, h, S, count)
    _assert_sums(out, rc.expected_by_frames(oracle, _osc(oracle), "full_bsdf", w, h, S, None, count), ("RT_PATHS_BLOCKS", blocks))
    assert st["camera_rays"] == int(count.sum())
    w, h, S = 1, 1300, 600
    want, ev_c = rc.expected_by_tables(oracle, _osc(oracle), w, h, S, None, _edge_map())
    out, st = _render(api, torch, gpu, w, h, S, _edge_map())
    _assert_sums(out, want, ("RT_PATHS_BLOCKS", blocks, "edges"))
    assert _ev(st) == ev_c


def test_the_few_blocks_build_over_two_generations(api, torch, oracle, monkeypatch):
    """256 x 144 x 32 with one row left out is more than W = 2^20 ids: the slots' second generation."""
    monkeypatch.setenv("RT_PATHS_BLOCKS", "512")
    w, h, S = 256, 144, 32
    count = np.full((h, w), S, np.int64)
    count[70, :] = 0
    count = count.reshape(-1)
    assert int(count.sum()) > 1 << 20
    out, st = _render(api, torch, _gpu(api, "full_bsdf"), w, h, S, count)
    _assert_sums(out, rc.expected_by_frames(oracle, _osc(oracle), "full_bsdf", w, h, S, None, count), "two generations")
    assert st["camera_rays"] == int(count.sum())


def test_tree_built_on_the_device(api, torch, oracle, bunny_full_bsdf):
    w, h, S = 9, 7, 8
    first, count = _random_map(w, h, S)
    want, ev_c = rc.expected_by_tables(oracle, _osc(oracle), w, h, S, first, count)
    dev = api.Scene(bunny_full_bsdf, device_bvh=True)
    out, st = _render(api, torch, dev, w, h, S, count, first)
    dev.close()
    _assert_sums(out, want, "device-built tree")
    assert _ev(st) == ev_c


def test_four_bunnies(api, torch, oracle):
    w, h, S = 9, 7, 8
    first, count = _random_map(w, h, S)
    want, ev_c = rc.expected_by_tables(oracle, _osc(oracle, "four_bunnies"), w, h, S, first, count)
    out, st = _render(api, torch, _gpu(api, "four_bunnies"), w, h, S, count, first)
    _assert_sums(out, want, "four_bunnies")
    assert _ev(st) == ev_c


# ---- 8. refusals
def test_errors_name_the_entry_point_and_leave_the_buffers_untouched(api, torch, monkeypatch):
    from rtcuda_amd import scenes
    gpu = _gpu(api, "full_bsdf")
    w, h, S = 9, 7, 8
    n = w * h

    def refused(pattern, count=None, first=None, scene=gpu, **kw):
        buf = torch.full((n, 3), SENTINEL, dtype=torch.int64, device="cuda")
        samples = torch.full((n,), 5, dtype=torch.int32, device="cuda")
        with pytest.raises(api.RtError, match="rt_render_counts_fixed: .*" + pattern):
            _render(api, torch, scene, w, h, kw.pop("S", S), np.full(n, 2) if count is None else count, first, samples=samples, out=buf, **kw)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()) and bool((samples == 5).all())

    bad = np.full(n, 2)
    bad[7] = -1
    refused("1 pixel", count=bad)
    refused("1 pixel", first=-(bad < 0).astype(np.int64))
    first = np.zeros(n, np.int64)
    first[[3, 40, 62]] = (7, 8, 2 ** 31 - 1)  # 7 + 2 > 8; 8 + 2 > 8; an int32 sum that would wrap
    refused("3 pixel.*sample_stride \\(8\\)", first=first)
    refused("3 pixel", first=first, count=np.where(first == 2 ** 31 - 1, 2 ** 31 - 1, 2))
    refused("RT_FLAG_REFERENCE_WALK", flags=api.FLAG_REFERENCE_WALK)
    refused("flags other than", flags=api.FLAG_DETERMINISTIC)
    refused("max_bounces", max_bounces=-1)
    refused("camera-ray range", S=2 ** 31 - 1, count=np.full(n, 2 ** 31 - 1))
    monkeypatch.setenv("RT_BVH_WIDE", "0")
    pairs = api.Scene(scenes.cornell_bunny("full_bsdf"))
    monkeypatch.delenv("RT_BVH_WIDE")
    refused("RT_BVH_WIDE=0", scene=pairs)
    pairs.close()
    monkeypatch.setenv("RT_PERSISTENT", "0")
    refused("RT_PERSISTENT=0")


def test_flags_that_are_what_the_mode_is_change_nothing(api, torch, oracle):
    w, h, S = 19, 27, 3
    want, ev_c = _oracle_whole(oracle, w, h, S)
    for flags in (api.FLAG_RNG_PER_SAMPLE, api.FLAG_WATERTIGHT, api.FLAG_RNG_PER_SAMPLE | api.FLAG_WATERTIGHT | api.FLAG_TIME_KERNELS):
        out, st = _render(api, torch, _gpu(api, "full_bsdf"), w, h, S, np.full(w * h, S), flags=flags)
        _assert_sums(out, want, ("flags", flags))
        assert _ev(st) == ev_c


# ---- 9. a non-default stream
def test_call_is_ordered_on_the_callers_stream(api, torch, oracle):
    w, h, S = MAIN
    want, ev_c = _oracle_whole(oracle, w, h, S)
    cam = api.make_camera(aspect=w / h)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        acc = torch.full((w * h, 3), 123, dtype=torch.int64, device="cuda")
        big = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
        for _ in range(8):
            big.fill_(1.0)  # a long fill in front: the stream is busy while the call is made
        acc.zero_()
        count = (big[:w * h] * float(S)).to(torch.int32)  # the count map itself depends on the fill
        out, st = _gpu(api, "full_bsdf").render_counts(cam, w, h, S, count, out=acc, stream=s)
    _assert_sums(out, want, "non-default stream")
    assert _ev(st) == ev_c


# ---- 10. the per-pixel divisor
@pytest.mark.parametrize("n", [1, 255, 257, 14400])
def test_normalize_and_post_process_against_the_twins(api, torch, n):
    rng = np.random.default_rng(n)
    sums = rng.integers(-(1 << 40), 1 << 40, (n, 3))
    sums[rng.random((n, 3)) < 0.1] = 0
    samples = rng.integers(0, 10, n).astype(np.int32)
    samples[0] = 0 if n > 1 else 3
    samples[-1] = 3
    want = rc.normalize_twin(sums, samples)
    d_sums, d_samples = _dev(torch, sums, np.int64), _dev(torch, samples)
    got = api.normalize_counts(d_sums, d_samples)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(d_sums.cpu().numpy(), sums)
    pos = np.abs(sums)  # (the post-process takes a square root)
    pp = api.post_process_counts(_dev(torch, pos, np.int64), d_samples).cpu().numpy()
    assert np.array_equal(pp.view(np.uint32), rc.post_process_twin(pos, samples).view(np.uint32))
    same = api.normalize_counts(d_sums, d_samples, out=d_sums)  # in place
    assert same is d_sums and np.array_equal(d_sums.cpu().numpy(), want)
    ones = torch.ones_like(d_samples)
    assert torch.equal(api.normalize_counts(got, ones), got)  # n == 1: the identity
    neg = d_samples.clone()
    neg[n // 2] = -2
    keep = torch.full((n, 3), SENTINEL, dtype=torch.int64, device="cuda")
    with pytest.raises(api.RtError, match="rt_normalize_counts_fixed: 1 pixel"):
        api.normalize_counts(got, neg, out=keep)
    torch.cuda.synchronize()
    assert bool((keep == SENTINEL).all())


def test_a_normalised_frame_feeds_the_denoiser_unchanged(api, torch):
    w, h = 64, 48
    gpu = _gpu(api, "full_bsdf")
    cam = api.make_camera(aspect=w / h)
    samples = torch.zeros((w * h,), dtype=torch.int32, device="cuda")
    sums, _ = gpu.render_counts(cam, w, h, 1, torch.ones((w * h,), dtype=torch.int32, device="cuda"), samples=samples)
    aov, _, _ = gpu.render_aov(cam, w, h, 4, flags=api.FLAG_WATERTIGHT)
    assert bool((samples == 1).all()) and bool(sums.any())
    normalized = api.normalize_counts(sums, samples)
    assert torch.equal(normalized, sums)
    a = api.denoise(normalized, 1, aov, 4, w, h)
    b = api.denoise(sums, 1, aov, 4, w, h)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


# ---- 11. the allocator
def _weights(n, seed):
    rng = np.random.default_rng(seed)
    w = (rng.random(n) ** 4 * 8.0).astype(np.float32)
    if n >= 255:
        w[::7] = np.nan
        w[3::7] = -1.0
        w[5] = np.inf
        w[9] = 5000.0  # above the cap of 4096
        w[11] = 0.0
    return w


@pytest.mark.parametrize("n", [1, 255, 257, 14400])
def test_sample_allocate_against_the_twin(api, torch, n):
    w = _weights(n, n)
    d_w = _dev(torch, w, np.float32)
    cases = [(0, 64, 8 * n), (1, 4, 8 * n), (2, 2, 2 * n), (0, 2 ** 31 - 1, 2 ** 31 - 1), (3, 5, 3 * n)]
    for lo, hi, budget in cases:
        want, total = rc.allocate_twin(w, lo, hi, budget)
        got, got_total = api.sample_allocate(d_w, lo, hi, budget)
        assert np.array_equal(got.cpu().numpy(), want) and got_total == total <= budget, (lo, hi, budget)
    if n > 1:
        assert (rc.allocate_twin(w, 1, 4, 8 * n)[0] == 4).any()  # a cap that binds
    zero = torch.zeros((n,), dtype=torch.float32, device="cuda")
    want, total = rc.allocate_twin(np.zeros(n, np.float32), 1, 9, 3 * n + n // 2)
    got, got_total = api.sample_allocate(zero, 1, 9, 3 * n + n // 2)
    assert np.array_equal(got.cpu().numpy(), want) and got_total == total and (want == 3).all()
    keep = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    for lo, hi, budget, pattern in ((-1, 4, 8 * n, "min_count = -1"), (3, 2, 8 * n, "max_count = 2 is below"), (2, 4, 2 * n - 1, "is below num_pixels"),
                                    (0, 4, 2 ** 31, "exceeds 2147483647")):
        with pytest.raises(api.RtError, match="rt_sample_allocate: .*" + pattern):
            api.sample_allocate(d_w, lo, hi, budget, out=keep)
    torch.cuda.synchronize()
    assert bool((keep == 77).all())
