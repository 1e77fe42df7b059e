"""GPU tests of the keyed ray tables (rt_render_rays_keyed_device / rt_render_rays_keyed_fixed_device).  Run with -m gpu.

Row c of a keyed table has the key K = key_first + c * key_stride and the stream of camera ray K of an RT_FLAG_RNG_PER_SAMPLE
frame, so a table that holds a pinhole camera's own per-sample rays (tests/raytable_keyed.py, held to the oracle by
tests/test_render_rays_keyed_host.py) must give `oracle.render(..., rng_mode="per_sample")`: ALL int64 sums EQUAL and the six
event totals EQUAL, no tolerance, no masked pixel -- for the whole table, for rank r of R, for chunks in any order, for keys
beyond 2^32, through every build of k_paths<PathsKeyed>.  Test 11 (rays no pinhole makes) is GPU against itself: a consistency
check of the partition invariance; tests 1 - 5 are the correctness pins."""
import numpy as np
import pytest

from conftest import default_camera, oracle_scene, usable_cpus
import raygen
import raytable_keyed as rk

pytestmark = pytest.mark.gpu

KEYS = ("camera_rays", "shade_events", "any_rays", "emission_adds", "shadow_adds", "rr_draws")
FLT_MAX = np.float32(3.4028234663852886e38)
MAIN = (160, 90, 16)  # 230 400 rays: 450 chunks of 512 ids


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


_oracle_cache = {}


def _oracle(oracle, osc, tag, w, h, spp, max_bounces=10, seed=1, shard=(0, 1)):
    """(fixed sums (w * h, 3) int64, raw float sums (w * h, 3), the six event totals) of the oracle's per-sample frame; computed
    once per session and argument tuple, never modified."""
    key = (tag, w, h, spp, max_bounces, seed, shard)
    if key not in _oracle_cache:
        want = np.zeros((h, w, 3), np.int64)
        _, raw, st = osc.render(default_camera(oracle, w / h), w, h, spp, max_bounces=max_bounces, seed=seed, threads=usable_cpus(),
                                fixed_out=want, rng_mode="per_sample", shard=shard)
        assert st["ch_adds"] == 0
        ev = {"camera_rays": st["sum_gen"], "shade_events": st["sum_mat"], "any_rays": st["sum_ah"],
              "emission_adds": st["emission_adds"], "shadow_adds": st["ah_adds"], "rr_draws": st["rr_draws"]}
        want = want.reshape(-1, 3)
        want.setflags(write=False)
        _oracle_cache[key] = (want, raw.reshape(-1, 3), ev)
    return _oracle_cache[key]


def _oracle_full(oracle, w, h, spp, **kw):
    return _oracle(oracle, oracle_scene(oracle, "full_bsdf", True), "full_bsdf", w, h, spp, **kw)


_tables = {}


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _table(oracle, torch, w, h, spp, seed=1):
    """The whole per-sample frame's table (keys 0 .. w * h * spp) on the device, and its pixel array on the host."""
    if (w, h, spp, seed) not in _tables:
        o, d, pixel = rk.keyed_pinhole_table(oracle, default_camera(oracle, w / h), w, h, spp, seed, range(w * h * spp))
        _tables[(w, h, spp, seed)] = (_dev(torch, o), _dev(torch, d), pixel)
    return _tables[(w, h, spp, seed)]


def _ev(st):
    return {k: st[k] for k in KEYS}


def _assert_equal(got, ev_g, want, ev_c, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    bad = got != want
    print(what, "sums that differ:", int(bad.sum()), "of", bad.size, "events", ev_g, ev_c)
    assert not bad.any(), (what, "sums that differ: %d of %d" % (int(bad.sum()), bad.size), "first (pixel, channel):",
                           np.argwhere(bad)[:6].tolist(), "got", got[bad][:6].tolist(), "want", want[bad][:6].tolist())
    assert ev_g == ev_c, (what, ev_g, ev_c)


def _add(evs):
    return {k: sum(e[k] for e in evs) for k in KEYS}


# ---- 1. a pinhole's table is the oracle's per-sample frame
FRAMES = [(1, 1, 1), (1, 63, 1), (1, 65, 1), (1, 511, 1), (1, 513, 1), (19, 27, 3), MAIN, (256, 144, 40)]


@pytest.mark.parametrize("w,h,spp", FRAMES, ids=["%dx%dx%d" % f for f in FRAMES])
def test_pinhole_table_is_the_oracles_per_sample_frame(api, torch, oracle, w, h, spp):
    o, d, _ = _table(oracle, torch, w, h, spp)
    want, _, ev_c = _oracle_full(oracle, w, h, spp)
    assert ev_c["camera_rays"] == w * h * spp
    gpu = _gpu(api, "full_bsdf")
    out, st = gpu.render_rays_keyed(o, d, w * h, rays_per_pixel=spp, fixed=True)
    _assert_equal(out, _ev(st), want, ev_c, ("keyed table", w, h, spp))
    cam = torch.zeros((w * h, 3), dtype=torch.int64, device="cuda")
    st_c = gpu.render_shard_fixed(api.make_camera(aspect=w / h), w, h, spp, 0, 1, cam.data_ptr(), flags=api.FLAG_RNG_PER_SAMPLE)
    torch.cuda.synchronize()
    assert torch.equal(out, cam) and _ev(st_c) == _ev(st)


# ---- 2. stride: rank r of R
@pytest.mark.parametrize("w,h,spp,R", [(9, 7, 8, 2), (9, 7, 8, 8), MAIN + (4,)])
def test_strided_table_is_rank_r_of_R(api, torch, oracle, w, h, spp, R):
    o, d, _ = _table(oracle, torch, w, h, spp)
    gpu = _gpu(api, "full_bsdf")
    total = torch.zeros((w * h, 3), dtype=torch.int64, device="cuda")
    evs = []
    for r in range(R):
        want, _, ev_c = _oracle_full(oracle, w, h, spp, shard=(r, R))
        out, st = gpu.render_rays_keyed(o[r::R].contiguous(), d[r::R].contiguous(), w * h, rays_per_pixel=spp, key_first=r, key_stride=R,
                                        fixed=True)
        assert st["camera_rays"] == w * h * spp // R
        _assert_equal(out, _ev(st), want, ev_c, ("rank", r, R))
        total += out
        evs.append(_ev(st))
    full, _, ev_full = _oracle_full(oracle, w, h, spp)
    _assert_equal(total, _add(evs), full, ev_full, ("ranks added", R))


# ---- 3. contiguous chunks
def test_contiguous_chunks_add_up_in_any_order(api, torch, oracle):
    w, h, spp = MAIN
    n = w * h * spp
    o, d, _ = _table(oracle, torch, w, h, spp)
    want, _, ev_c = _oracle_full(oracle, w, h, spp)
    cuts = [0, 1, 511, 512, 4096 + 7, 100003, n]
    assert 100003 % spp != 0  # (mid-pixel)
    chunks = list(zip(cuts[:-1], cuts[1:]))
    gpu = _gpu(api, "full_bsdf")
    results = []
    for order in (chunks, chunks[::-1]):
        acc = torch.zeros((w * h, 3), dtype=torch.int64, device="cuda")
        evs = []
        for a, b in order:
            _, st = gpu.render_rays_keyed(o[a:b], d[a:b], w * h, rays_per_pixel=spp, key_first=a, fixed=True, out=acc)
            assert st["camera_rays"] == b - a
            evs.append(_ev(st))
        _assert_equal(acc, _add(evs), want, ev_c, "chunks")
        results.append(acc)
    assert torch.equal(results[0], results[1])


# ---- 4. explicit pixel maps
def test_explicit_pixel_map_and_permutation(api, torch, oracle):
    w, h, spp = MAIN
    o, d, pixel = _table(oracle, torch, w, h, spp)
    want, _, ev_c = _oracle_full(oracle, w, h, spp)
    gpu = _gpu(api, "full_bsdf")
    same, st1 = gpu.render_rays_keyed(o, d, w * h, pixel=_dev(torch, pixel), rays_per_pixel=0, fixed=True)
    _assert_equal(same, _ev(st1), want, ev_c, "d_pixel = K // spp")
    perm = np.random.default_rng(5).permutation(w * h).astype(np.int32)
    moved, st2 = gpu.render_rays_keyed(o, d, w * h, pixel=_dev(torch, perm[pixel]), fixed=True)
    _assert_equal(moved[_dev(torch, perm.astype(np.int64))], _ev(st2), want, ev_c, "permuted pixels")


# ---- 5. 64-bit keys
@pytest.mark.parametrize("F", [2 ** 32 - 100, 2 ** 40 + 5], ids=["across-2^32", "2^40+5"])
def test_keys_beyond_32_bits(api, torch, oracle, F):
    """Keys F .. F + n under seed s are the keys 0 .. n under the shifted seed s' (test_seed_shift_identity), so the frame is
    the oracle's at seed s' -- with the pixels given explicitly, since key // spp is far outside the frame."""
    w, h, spp = MAIN
    s = 1
    s2 = rk.shifted_seed(s, F)
    o, d, pixel = _table(oracle, torch, w, h, spp, seed=s2)
    want, _, ev_c = _oracle_full(oracle, w, h, spp, seed=s2)
    out, st = _gpu(api, "full_bsdf").render_rays_keyed(o, d, w * h, pixel=_dev(torch, pixel), key_first=F, seed=s, fixed=True)
    _assert_equal(out, _ev(st), want, ev_c, ("key_first", F))
    base, _, _ = _oracle_full(oracle, w, h, spp)
    assert not np.array_equal(want, base)


@pytest.mark.parametrize("seed", [0, 2 ** 32, 0xFFFFFFFF00000007], ids=hex)
def test_seeds_whose_high_word_matters(api, torch, oracle, seed):
    w, h, spp = MAIN
    o, d, _ = _table(oracle, torch, w, h, spp, seed=seed)
    want, _, ev_c = _oracle_full(oracle, w, h, spp, seed=seed)
    out, st = _gpu(api, "full_bsdf").render_rays_keyed(o, d, w * h, rays_per_pixel=spp, seed=seed, fixed=True)
    _assert_equal(out, _ev(st), want, ev_c, ("seed", seed))


# ---- 6. max_bounces
@pytest.mark.parametrize("max_bounces", [0, 1, 10])
def test_max_bounces(api, torch, oracle, max_bounces):
    w, h, spp = MAIN
    o, d, _ = _table(oracle, torch, w, h, spp)
    want, _, ev_c = _oracle_full(oracle, w, h, spp, max_bounces=max_bounces)
    out, st = _gpu(api, "full_bsdf").render_rays_keyed(o, d, w * h, rays_per_pixel=spp, max_bounces=max_bounces, fixed=True)
    _assert_equal(out, _ev(st), want, ev_c, ("max_bounces", max_bounces))
    assert (st["shade_events"] == 0) == (max_bounces == 0)
    assert st["emission_adds"] > 0 and want.any()


# ---- 7. the few_blocks build
@pytest.mark.parametrize("blocks", ["512", "64"])
def test_the_few_blocks_build(api, torch, oracle, monkeypatch, blocks):
    """A grid of at most two workgroups per CU launches the MIN_WAVES = 2 build: gen() inside the ADV block, row ids tied to
    slots (id = generation * W + slot; 256 x 144 x 40 is two generations), the stream re-seeded from the row's key."""
    monkeypatch.setenv("RT_PATHS_BLOCKS", blocks)
    gpu = _gpu(api, "full_bsdf")
    for w, h, spp in ((256, 144, 40), (1, 513, 1)):
        o, d, _ = _table(oracle, torch, w, h, spp)
        want, _, ev_c = _oracle_full(oracle, w, h, spp)
        out, st = gpu.render_rays_keyed(o, d, w * h, rays_per_pixel=spp, fixed=True)
        _assert_equal(out, _ev(st), want, ev_c, ("RT_PATHS_BLOCKS", blocks, w, h, spp))


# ---- 8. tables in global memory and other trees
def test_more_than_64_materials(api, torch, oracle):
    """Shading tables in global memory (the LDS_TABLES = false builds)."""
    import table_scenes as ts
    arrays = ts.table_scene(200, 100)
    assert not ts.lds_tables(200, 100)
    w, h, spp = MAIN
    o, d, _ = _table(oracle, torch, w, h, spp)
    want, _, ev_c = _oracle(oracle, oracle.scene(arrays).set_watertight(True), "table_scene(200, 100)", w, h, spp)
    gpu = api.Scene(arrays)
    out, st = gpu.render_rays_keyed(o, d, w * h, rays_per_pixel=spp, fixed=True)
    gpu.close()
    _assert_equal(out, _ev(st), want, ev_c, "table_scene(200, 100)")


def test_four_bunnies_overflow_stack(api, torch, oracle):
    w, h, spp = MAIN
    o, d, _ = _table(oracle, torch, w, h, spp)
    want, _, ev_c = _oracle(oracle, oracle_scene(oracle, "four_bunnies", True), "four_bunnies", w, h, spp)
    out, st = _gpu(api, "four_bunnies").render_rays_keyed(o, d, w * h, rays_per_pixel=spp, fixed=True)
    _assert_equal(out, _ev(st), want, ev_c, "four_bunnies")


def test_tree_built_and_rebuilt_on_the_device(api, torch, oracle, bunny_full_bsdf):
    w, h, spp = MAIN
    o, d, _ = _table(oracle, torch, w, h, spp)
    want, _, ev_c = _oracle_full(oracle, w, h, spp)
    dev = api.Scene(bunny_full_bsdf, device_bvh=True)
    out, st = dev.render_rays_keyed(o, d, w * h, rays_per_pixel=spp, fixed=True)
    _assert_equal(out, _ev(st), want, ev_c, "RT_SCENE_DEVICE_BVH")
    dev.rebuild()
    out, st = dev.render_rays_keyed(o, d, w * h, rays_per_pixel=spp, fixed=True)
    dev.close()
    _assert_equal(out, _ev(st), want, ev_c, "RT_SCENE_DEVICE_BVH + rt_scene_rebuild")


# ---- 9. float entry point
@pytest.mark.parametrize("w,h", [(1, 513), (19, 27)])
def test_float_entry_point_with_one_ray_per_pixel(api, torch, oracle, w, h):
    """spp = 1: a pixel's float sum is ONE add of its camera ray's sum to zero, so the raw float sums are the oracle's fb_sum
    bit for bit."""
    o, d, _ = _table(oracle, torch, w, h, 1)
    _, raw, ev_c = _oracle_full(oracle, w, h, 1)
    out, st = _gpu(api, "full_bsdf").render_rays_keyed(o, d, w * h, rays_per_pixel=1)
    got = out.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.ascontiguousarray(raw, np.float32).view(np.uint32))
    assert _ev(st) == ev_c and raw.any()


# ---- 10. a non-default stream
def test_call_is_ordered_on_the_callers_stream(api, torch, oracle):
    w, h, spp = MAIN
    o, d, _ = _table(oracle, torch, w, h, spp)
    want, _, ev_c = _oracle_full(oracle, w, h, spp)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        acc = torch.full((w * h, 3), 123, dtype=torch.int64, device="cuda")
        big = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
        for _ in range(8):
            big.fill_(1.0)  # a long fill in front: the stream is busy while the call is made
        acc.zero_()
        d2 = d + big[:3] * 0.0  # the table itself depends on the fill
        out, st = _gpu(api, "full_bsdf").render_rays_keyed(o, d2, w * h, rays_per_pixel=spp, fixed=True, out=acc, stream=s)
    _assert_equal(out, _ev(st), want, ev_c, "non-default stream")


# ---- 11. partition invariance on rays no pinhole makes (GPU against itself: a consistency check)
def _ray_sets(api, gpu):
    n = 50000
    g = np.linspace(0.02, 0.98, 224, dtype=np.float32)
    ox, oy = np.meshgrid(g, g)
    ortho_o = np.stack([ox.ravel(), oy.ravel(), np.full(ox.size, 1.5, np.float32)], axis=1).astype(np.float32)[:n]
    ortho_d = np.tile(np.array([0, 0, -1], np.float32), (n, 1))
    po, pd = raygen.camera_rays(api.make_camera(), 1, 1, 70000, 3)
    tri, t, _, _ = gpu.trace_closest(po, pd, np.full(len(po), FLT_MAX, np.float32))
    bo, bd = raygen.bounce_rays(po, pd, t, tri >= 0, 4)
    assert len(bo) >= n
    return {"orthographic": (ortho_o, ortho_d), "bounce": (bo[:n], bd[:n])}


@pytest.mark.parametrize("name", ["orthographic", "bounce"])
def test_partition_invariance_on_rays_no_pinhole_makes(api, torch, name):
    """Consistency, not correctness: one call == three uneven chunks == four strided ranks, sums and events."""
    gpu = _gpu(api, "full_bsdf")
    o_h, d_h = _ray_sets(api, gpu)[name]
    n, npix = len(o_h), 4096
    o, d = _dev(torch, o_h), _dev(torch, d_h)
    pixel = _dev(torch, ((np.arange(n) * 7) % npix).astype(np.int32))
    one, st = gpu.render_rays_keyed(o, d, npix, pixel=pixel, fixed=True)
    assert st["camera_rays"] == n and st["shade_events"] > n // 4 and bool(one.any())
    acc = torch.zeros_like(one)
    evs = []
    for a, b in ((0, 777), (777, 30001), (30001, n)):
        _, s = gpu.render_rays_keyed(o[a:b], d[a:b], npix, pixel=pixel[a:b], key_first=a, fixed=True, out=acc)
        evs.append(_ev(s))
    assert torch.equal(acc, one) and _add(evs) == _ev(st)
    acc = torch.zeros_like(one)
    evs = []
    for r in range(4):
        _, s = gpu.render_rays_keyed(o[r::4].contiguous(), d[r::4].contiguous(), npix, pixel=pixel[r::4].contiguous(), key_first=r,
                                     key_stride=4, fixed=True, out=acc)
        evs.append(_ev(s))
    assert torch.equal(acc, one) and _add(evs) == _ev(st)


# ---- 12. refusals
def test_errors_name_the_entry_point_and_leave_the_sum_buffer_untouched(api, torch, monkeypatch):
    from rtcuda_amd import scenes
    gpu = _gpu(api, "full_bsdf")
    n, npix = 4096, 1024
    o_h, d_h = raygen.camera_rays(api.make_camera(), 1, 1, n, 11)
    o, d = _dev(torch, o_h), _dev(torch, d_h)
    pixel = _dev(torch, (np.arange(n) % npix).astype(np.int32))
    sentinel = 0x5A5A5A5A

    def refused(pattern, fixed=False, scene=gpu, **kw):
        args = dict(o_ptr=o.data_ptr(), d_ptr=d.data_ptr(), pixel_ptr=pixel.data_ptr(), n_rays=n, n_pixels=npix, rays_per_pixel=1, flags=0)
        args.update(kw)
        buf = torch.full((npix, 3), sentinel, dtype=torch.int64 if fixed else torch.int32, device="cuda")
        ptr = 0 if args.pop("null_sum", False) else buf.data_ptr()
        name = "rt_render_rays_keyed_fixed_device" if fixed else "rt_render_rays_keyed_device"
        with pytest.raises(api.RtError, match=name + ": .*" + pattern):
            scene.render_rays_keyed_device(d_sum_ptr=ptr, fixed=fixed, **args)
        torch.cuda.synchronize()
        assert bool((buf == sentinel).all())

    monkeypatch.setenv("RT_BVH_WIDE", "0")
    pairs = api.Scene(scenes.cornell_bunny("full_bsdf"))
    monkeypatch.delenv("RT_BVH_WIDE")
    for fixed in (False, True):
        refused("key_stride = 0", fixed, key_stride=0)
        refused("wraps 2\\^64", fixed, key_first=2 ** 64 - n + 1)  # the last key would be 2^64
        refused("wraps 2\\^64", fixed, key_first=2 ** 64 - 1, key_stride=2 ** 32 - 1)
        refused("falls on pixel", fixed, pixel_ptr=0, rays_per_pixel=3, n_pixels=npix)  # key 4095 -> pixel 1365 of 1024
        refused("falls on pixel 1024 of 1024", fixed, pixel_ptr=0, rays_per_pixel=4, key_first=1)  # key 4096
        refused("falls on pixel", fixed, pixel_ptr=0, rays_per_pixel=4, key_stride=2)
        refused("rays_per_pixel = 0", fixed, pixel_ptr=0, rays_per_pixel=0)
        refused("n_rays = 0", fixed, n_rays=0)
        refused("n_pixels = 0", fixed, n_pixels=0)
        refused("null d_origin_xyz", fixed, o_ptr=0)
        refused("null d_dir_xyz", fixed, d_ptr=0)
        refused("null sum buffer", fixed, null_sum=True)
        for bad, count in ((float("nan"), 3), (float("inf"), 2), (2.0 ** 126, 1)):
            dd = d.clone()
            dd[torch.arange(count, device="cuda") * 7 + 5, 1] = bad
            refused(f"{count} of {n} directions", fixed, d_ptr=dd.data_ptr())
        for bad in (-1, npix):
            pp = pixel.clone()
            pp[17] = bad
            pp[n - 1] = bad
            refused(f"2 of {n} pixel indices", fixed, pixel_ptr=pp.data_ptr())
        refused("RT_FLAG_REFERENCE_WALK", fixed, flags=api.FLAG_REFERENCE_WALK)
        refused("RT_FLAG_REFERENCE_WALK", fixed, flags=api.FLAG_REFERENCE_WALK | api.FLAG_RNG_PER_SAMPLE)
        refused("flags other than", fixed, flags=api.FLAG_DETERMINISTIC)
        refused("max_bounces", fixed, max_bounces=-1)
        refused("RT_BVH_WIDE=0", fixed, scene=pairs)
    pairs.close()


def test_flags_that_are_what_the_mode_is_change_nothing(api, torch, oracle):
    w, h, spp = 19, 27, 3
    o, d, _ = _table(oracle, torch, w, h, spp)
    want, _, ev_c = _oracle_full(oracle, w, h, spp)
    gpu = _gpu(api, "full_bsdf")
    for flags in (api.FLAG_RNG_PER_SAMPLE, api.FLAG_WATERTIGHT, api.FLAG_RNG_PER_SAMPLE | api.FLAG_WATERTIGHT | api.FLAG_TIME_KERNELS):
        out = torch.zeros((w * h, 3), dtype=torch.int64, device="cuda")
        st = gpu.render_rays_keyed_device(o.data_ptr(), d.data_ptr(), 0, w * h * spp, w * h, out.data_ptr(), rays_per_pixel=spp, flags=flags,
                                          fixed=True)
        _assert_equal(out, _ev(st), want, ev_c, ("flags", flags))


# ---- 13. stats
def test_stats_and_run_twice(api, torch, oracle):
    w, h, spp = MAIN
    o, d, _ = _table(oracle, torch, w, h, spp)
    gpu = _gpu(api, "full_bsdf")
    outs = []
    for _ in range(2):
        out = torch.zeros((w * h, 3), dtype=torch.int64, device="cuda")
        raw = api.RtStats()
        rc = gpu.L.rt_render_rays_keyed_fixed_device(gpu.h, w * h * spp, o.data_ptr(), d.data_ptr(), None, spp, w * h, 10, 1, 0, 1, 0,
                                                     out.data_ptr(), None, raw)
        assert rc == 0, gpu.L.rt_last_error()
        assert raw.camera_rays == w * h * spp and raw.reserved[1] == 1
        outs.append((out, _ev(raw.as_dict())))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
