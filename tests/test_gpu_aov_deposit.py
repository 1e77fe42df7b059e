"""GPU tests of the deposit end of k_aov (aov_deposit: pack the depositing lanes, segmented scan over lane distances 1 .. 32,
one set of atomics per run) at the run lengths a user renders with, of the kernel's to_fixed at its edges and of rt_aov_resolve
on sums no frame of the suite holds.  Run with -m gpu.

Expected values come from tests/aov_expected.py; tests/test_aov_deposit_host.py shows on the CPU that they hold what each case
claims to reach.  Every comparison is EQUALITY of all 11 int64 channels on every pixel (and of the ids where they are written):
no tolerance, no masked pixel."""
import ctypes
import time

import numpy as np
import pytest

from conftest import default_camera, oracle_scene, usable_cpus  # noqa: F401  (usable_cpus: the oracle's thread count, as test_gpu_aov)
import aov_expected as ae
import raytable_keyed as rk

pytestmark = pytest.mark.gpu

POISON = -7


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


def _gpu(api):
    if "full_bsdf" not in _gpu_cache:
        from rtcuda_amd import scenes
        _gpu_cache["full_bsdf"] = api.Scene(scenes.cornell_bunny("full_bsdf"))
    return _gpu_cache["full_bsdf"]


def _flags(api, mode):
    return {"default": 0, "reference-walk": api.FLAG_REFERENCE_WALK, "watertight": api.FLAG_WATERTIGHT}[mode]


_expected = {}


def _frame(oracle, w, h, spp, watertight, wide=False, shard=(0, 1)):
    """The helper's frame on full_bsdf, computed once per session and argument tuple and never modified."""
    key = (w, h, spp, watertight, wide, shard)
    if key not in _expected:
        osc = oracle_scene(oracle, "full_bsdf", watertight)
        cam = ae.wide_camera(oracle.camera, w / h) if wide else default_camera(oracle, w / h)
        sums, ids, rest = ae.frame_expected(oracle, osc, cam, w, h, spp, shard=shard)
        sums.setflags(write=False)
        ids.setflags(write=False)
        _expected[key] = (sums, ids, rest)
    return _expected[key]


def _table(oracle, torch, watertight):
    """The base table on the device (once) and its features in the hit mode (once per mode), never modified."""
    if "table" not in _expected:
        w, h, spp = ae.DEPOSIT_BASE_TABLE
        o, d, _ = rk.keyed_pinhole_table(oracle, default_camera(oracle, w / h), w, h, spp, 1, range(w * h * spp))
        _expected["table"] = (o, d, _dev(torch, o), _dev(torch, d))
    o, d, o_dev, d_dev = _expected["table"]
    if ("features", watertight) not in _expected:
        tri, mat, vals = ae.sample_features(oracle, oracle_scene(oracle, "full_bsdf", watertight), o, d)
        for a in (tri, mat, vals):
            a.setflags(write=False)
        _expected["features", watertight] = (tri, mat, vals, {c[0]: c[1:] for c in ae.table_cases(tri)})
    return (o_dev, d_dev) + _expected["features", watertight]


def _camera(api, w, h, wide=False):
    return ae.wide_camera(api.make_camera, w / h) if wide else api.make_camera(aspect=w / h)


def _assert_sums(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    bad = got != want
    print(what, "sums that differ:", int(bad.sum()), "of", bad.size)
    at = np.argwhere(bad)[:6]
    assert not bad.any(), (what, "sums that differ: %d of %d" % (int(bad.sum()), bad.size), "first (pixel, channel, got, want):",
                           [(int(p), int(c), int(got[p, c]), int(want[p, c])) for p, c in at])


def _assert_ids(got, want, what=""):
    got = got.cpu().numpy()
    bad = (got != want).any(axis=1)
    assert not bad.any(), (what, "ids that differ: %d of %d" % (int(bad.sum()), bad.size), "first (pixel, got, want):",
                           [(int(p), got[p].tolist(), want[p].tolist()) for p in np.flatnonzero(bad)[:6]])


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poisoned_ids(torch, n_pixels):
    return torch.full((n_pixels, 2), POISON, dtype=torch.int32, device="cuda")


def _name(f):
    return "%dx%dx%d%s" % (f[0], f[1], f[2], "-wide" if f[3] else "")


# ---- 1. camera frames whose pixels are long runs of lanes
@pytest.mark.parametrize("mode", ["default", "watertight"])
@pytest.mark.parametrize("w,h,spp,wide", ae.DEPOSIT_FRAMES, ids=[_name(f) for f in ae.DEPOSIT_FRAMES])
def test_long_run_frames_are_the_helpers(api, torch, oracle, w, h, spp, wide, mode):
    want, want_ids, _ = _frame(oracle, w, h, spp, mode == "watertight", wide)
    t0 = time.perf_counter()
    out, ids, st = _gpu(api).render_aov(_camera(api, w, h, wide), w, h, spp, flags=_flags(api, mode), ids=_poisoned_ids(torch, w * h))
    _assert_sums(out, want, (mode, w, h, spp, wide))
    _assert_ids(ids, want_ids, (mode, w, h, spp, wide))  # (every pixel has a first sample: no poison is left)
    assert st["camera_rays"] == st["closest_rays"] == w * h * spp
    print("GPU side %.1f ms" % (1e3 * (time.perf_counter() - t0)))


def test_a_long_run_frame_under_the_reference_walk(api, torch, oracle):
    w, h, spp, wide = ae.DEPOSIT_FRAMES[2]  # 4 x 3 x 64: the chunk that is one pixel
    want, want_ids, _ = _frame(oracle, w, h, spp, False, wide)
    out, ids, st = _gpu(api).render_aov(_camera(api, w, h, wide), w, h, spp, flags=api.FLAG_REFERENCE_WALK, ids=_poisoned_ids(torch, w * h))
    _assert_sums(out, want, ("reference-walk", w, h, spp))
    _assert_ids(ids, want_ids, "reference-walk")
    assert (st["literal_retraces"], st["reference_lost_hits"], st["exact_ties"]) == (0, 0, 0)


@pytest.mark.parametrize("mode", ["default", "watertight"])
def test_shards_of_the_one_pixel_chunk_frame(api, torch, oracle, mode):
    """shard (r, 4): local spp 16 under key_mul = 4, each its own subset, the four added into one buffer the whole frame;
    shard (r, 64): local spp 1, a frame of 64 spp without a single run."""
    w, h, spp = ae.DEPOSIT_SHARD_FRAME
    gpu, cam, flags, watertight = _gpu(api), _camera(api, w, h), _flags(api, mode), mode == "watertight"
    total = torch.zeros((w * h, ae.CHANNELS), dtype=torch.int64, device="cuda")
    for r in range(4):
        want, want_ids, _ = _frame(oracle, w, h, spp, watertight, shard=(r, 4))
        out, ids, st = gpu.render_aov(cam, w, h, spp, flags=flags, shard=(r, 4), ids=_poisoned_ids(torch, w * h))
        _assert_sums(out, want, (mode, "rank", r, 4))
        _assert_ids(ids, want_ids, (mode, "rank", r, 4))
        assert st["camera_rays"] == w * h * spp // 4 and (r == 0 or bool((ids == POISON).all()))
        gpu.render_aov(cam, w, h, spp, flags=flags, shard=(r, 4), out=total)
    _assert_sums(total, _frame(oracle, w, h, spp, watertight)[0], (mode, "ranks added"))
    for r in (0, 37):
        want, want_ids, _ = _frame(oracle, w, h, spp, watertight, shard=(r, 64))
        out, ids, st = gpu.render_aov(cam, w, h, spp, flags=flags, shard=(r, 64), ids=_poisoned_ids(torch, w * h))
        _assert_sums(out, want, (mode, "rank", r, 64))
        _assert_ids(ids, want_ids, (mode, "rank", r, 64))
        assert st["camera_rays"] == w * h


# ---- 2. tables with crafted pixel arrays
TABLE_CASES = ["H-full-waves", "H-split-across-chunks", "H-one-address", "H-alternating", "B-drawn-runs", "B-descending-sevens",
               "M-nothing-deposits", "H-interleaved-halves"]


@pytest.mark.parametrize("mode", ["default", "watertight"])
@pytest.mark.parametrize("case", TABLE_CASES)
def test_crafted_pixel_arrays_give_the_helpers_sums(api, torch, oracle, case, mode):
    o_dev, d_dev, tri, mat, vals, cases = _table(oracle, torch, mode == "watertight")
    assert sorted(cases) == sorted(TABLE_CASES)
    rows, pixel, n_pixels, claim = cases[case]
    want = ae.deposit(tri[rows], vals[rows], pixel, n_pixels)
    fill = 123 if case == "M-nothing-deposits" else 0  # nothing deposits: the buffer is unchanged
    out = torch.full((n_pixels, ae.CHANNELS), fill, dtype=torch.int64, device="cuda")
    whole = rows.size == tri.size
    idx = None if whole else _dev(torch, rows)
    t0 = time.perf_counter()
    got, ids, st = _gpu(api).render_aov_rays(o_dev if whole else o_dev[idx].contiguous(), d_dev if whole else d_dev[idx].contiguous(), n_pixels,
                                             pixel=_dev(torch, pixel), flags=_flags(api, mode), out=out)
    assert ids is None and got is out and st["camera_rays"] == rows.size
    _assert_sums(out, want + fill, (case, mode))
    if case == "M-nothing-deposits":
        assert not want.any()
    print("GPU side %.1f ms" % (1e3 * (time.perf_counter() - t0)))


def test_runs_of_64_rays_per_pixel_under_keys_that_cross_2_to_32(api, torch, oracle):
    """d_pixel NULL: pixel = K // 64 for K from 2^32 - 100 on, runs of 64 whose pixel index lies around 2^26; the one row of each
    pixel whose key is a multiple of 64 writes the ids.  (The kernel divides the OFFSET from the first pixel's first key, which
    stays below 2^32 here: the 64-bit quotient of aov_pixel is reached by the next test.)"""
    o_dev, d_dev, tri, mat, vals, _ = _table(oracle, torch, False)
    rows = np.flatnonzero(tri >= 0)[:ae.KEYS_ROWS]
    keys = ae.KEYS_FIRST + np.arange(rows.size, dtype=np.int64)
    pixel = keys // ae.KEYS_RPP
    lo, n_pixels = int(pixel[0]), int(pixel[-1]) + 1
    want = ae.deposit(tri[rows], vals[rows], pixel - lo, n_pixels - lo)
    first = keys % ae.KEYS_RPP == 0
    want_ids = np.full((n_pixels - lo, 2), POISON, np.int32)
    want_ids[pixel[first] - lo] = np.stack([tri[rows][first], mat[rows][first]], 1)
    idx = _dev(torch, rows)
    out = torch.zeros((n_pixels, ae.CHANNELS), dtype=torch.int64, device="cuda")
    ids = _poisoned_ids(torch, n_pixels)
    _gpu(api).render_aov_rays(o_dev[idx].contiguous(), d_dev[idx].contiguous(), n_pixels, rays_per_pixel=ae.KEYS_RPP, key_first=ae.KEYS_FIRST,
                              out=out, ids=ids)
    _assert_sums(out[lo:], want, "keys around 2^32")
    _assert_ids(ids[lo:], want_ids, "keys around 2^32")
    assert bool((want_ids[0] == POISON).all()) and bool((want_ids[1:] != POISON).all())
    # the pixels in front of the first key's: nothing added, no id written (compared on the device: 5.9 GB of sums)
    assert int(torch.count_nonzero(out[:lo])) == 0 and bool((ids[:lo] == POISON).all())
    del out, ids
    torch.cuda.empty_cache()


def test_runs_across_the_64_bit_quotient_of_the_key_rule(api, torch, oracle):
    """A stride of 2^25 under rays_per_pixel = 3 * 2^28: runs of 24, and row * stride passes 2^32 inside the run of pixel 5, where
    aov_pixel goes from its 32-bit to its 64-bit quotient."""
    o_dev, d_dev, tri, mat, vals, _ = _table(oracle, torch, False)
    rows = np.flatnonzero(tri >= 0)[:ae.WIDE_KEYS_ROWS]
    t = np.arange(rows.size, dtype=np.int64) * ae.WIDE_KEYS_STRIDE
    pixel = t // ae.WIDE_KEYS_RPP
    n_pixels = int(pixel[-1]) + 1
    want = ae.deposit(tri[rows], vals[rows], pixel, n_pixels)
    first = t % ae.WIDE_KEYS_RPP == 0
    want_ids = np.full((n_pixels, 2), POISON, np.int32)
    want_ids[pixel[first]] = np.stack([tri[rows][first], mat[rows][first]], 1)
    idx = _dev(torch, rows)
    out, ids, _ = _gpu(api).render_aov_rays(o_dev[idx].contiguous(), d_dev[idx].contiguous(), n_pixels, rays_per_pixel=ae.WIDE_KEYS_RPP,
                                            key_stride=ae.WIDE_KEYS_STRIDE, ids=_poisoned_ids(torch, n_pixels))
    _assert_sums(out, want, "stride 2^25")
    _assert_ids(ids, want_ids, "stride 2^25")


# ---- 3. values at the edges of the kernel's to_fixed
def test_extreme_albedos_and_radiance_go_through_to_fixed_as_documented(api, torch, oracle, bunny_full_bsdf):
    """Albedos from {3e9, -3e9, +-inf, NaN, -0.5, 1e-10, 1.5 * 2^-31, 1} and L = (3e9, -inf, NaN): clamped to +-2^31, NaN and
    what rounds to 0 not added.  2 spp: no sum leaves int64 (the helper checks it in Python integers)."""
    arrays = ae.extreme_arrays(bunny_full_bsdf)
    w, h, spp = ae.EXTREME_FRAME
    gpu = api.Scene(arrays)
    for mode in ("default", "watertight"):
        osc = oracle.scene(arrays).set_watertight(mode == "watertight")
        want, want_ids, (tri, mat, vals, pixel, keys) = ae.frame_expected(oracle, osc, default_camera(oracle, w / h), w, h, spp)
        osc.close()
        assert np.array_equal(ae.exact_sums(tri, vals, pixel, w * h), want)
        out, ids, _ = gpu.render_aov(_camera(api, w, h), w, h, spp, flags=_flags(api, mode), ids=_poisoned_ids(torch, w * h))
        _assert_sums(out, want, ("extreme", mode))
        _assert_ids(ids, want_ids, ("extreme", mode))
    gpu.close()


# ---- 4. the resolve on sums no frame holds
@pytest.mark.parametrize("n_pixels", ae.RESOLVE_PIXELS)
def test_resolve_of_synthetic_sums_is_the_numpy_restatement_bit_for_bit(api, torch, n_pixels):
    sums = ae.synthetic_sums(n_pixels)
    dev = _dev(torch, sums)
    sentinel = np.float32(-12345.0)
    for spp in ae.RESOLVE_SAMPLES:
        want = ae.resolve(sums, spp).view(np.uint32)
        got = api.aov_resolve(dev, spp).cpu().numpy()
        bad = got.view(np.uint32) != want
        assert got.dtype == np.float32 and not bad.any(), (n_pixels, spp, "values that differ: %d" % int(bad.sum()), "first (pixel, channel):",
                                                            np.argwhere(bad)[:6].tolist(), "got", got[bad][:6].tolist(), "want",
                                                            want.view(np.float32)[bad][:6].tolist(), "sums", sums[bad][:6].tolist())
        # the library's own launch into a buffer 64 floats longer: the grid's last block writes nothing past the last value
        buf = torch.full((n_pixels * ae.CHANNELS + 64,), float(sentinel), dtype=torch.float32, device="cuda")
        rc = api.lib().rt_aov_resolve(ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(buf.data_ptr()), n_pixels, spp, None)
        assert rc == 0, api.lib().rt_last_error().decode()
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.array_equal(host[:n_pixels * ae.CHANNELS].view(np.uint32), want.ravel()) and (host[n_pixels * ae.CHANNELS:] == sentinel).all()
    assert np.array_equal(dev.cpu().numpy(), sums)  # (the sums are read only)
