"""GPU tests of the first-hit feature buffers (rt_render_aov_fixed / rt_render_aov_rays_fixed_device / rt_aov_resolve).  Run
with -m gpu.

What a frame must hold comes from tests/aov_expected.py (numpy + the oracle's trace_closest, held to the oracle's own per-sample
frame by tests/test_aov_host.py).  Every comparison is EQUALITY of all 11 int64 channels on all pixels: no tolerance, no masked
pixel."""
import dataclasses

import numpy as np
import pytest

from conftest import default_camera, oracle_scene, usable_cpus
import aov_expected as ae
import placed_scenes
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


def _modes(api):
    """(name, flags, the oracle's watertight switch)"""
    return [("default", 0, False), ("reference-walk", api.FLAG_REFERENCE_WALK, False), ("watertight", api.FLAG_WATERTIGHT, True)]


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


def _camera(api, w, h, wide=False):
    return ae.wide_camera(api.make_camera, w / h) if wide else api.make_camera(aspect=w / h)


def _assert_sums(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    bad = got != want
    print(what, "sums that differ:", int(bad.sum()), "of", bad.size)
    assert not bad.any(), (what, "sums that differ: %d of %d" % (int(bad.sum()), bad.size), "first (pixel, channel):",
                           np.argwhere(bad)[:6].tolist(), "got", got[bad][:6].tolist(), "want", want[bad][:6].tolist())


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poisoned_ids(torch, n_pixels):
    return torch.full((n_pixels, 2), POISON, dtype=torch.int32, device="cuda")


# ---- 1. frames either side of one wave and one chunk, spp that does not divide 64, and a wide view with many misses
FRAMES = [(1, 1, 1, False), (1, 63, 1, False), (8, 8, 1, False), (1, 65, 1, False), (19, 27, 3, False), (64, 48, 4, False),
          ae.WIDE_FRAME + (True,)]


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["default", "reference-walk", "watertight"])
@pytest.mark.parametrize("w,h,spp,wide", FRAMES, ids=["%dx%dx%d%s" % (f[0], f[1], f[2], "-wide" if f[3] else "") for f in FRAMES])
def test_frames_are_the_helpers(api, torch, oracle, w, h, spp, wide, mode):
    name, flags, watertight = _modes(api)[mode]
    want, want_ids, (tri, mat, _, _, _) = _frame(oracle, w, h, spp, watertight, wide)
    if wide:
        ae.assert_wide_content(oracle_scene(oracle, "full_bsdf", watertight).arrays, tri, mat, want)
    out, ids, st = _gpu(api).render_aov(_camera(api, w, h, wide), w, h, spp, flags=flags, ids=_poisoned_ids(torch, w * h))
    _assert_sums(out, want, (name, w, h, spp, wide))
    assert np.array_equal(ids.cpu().numpy(), want_ids)  # (every pixel has a first sample: no poison is left)
    assert st["camera_rays"] == st["closest_rays"] == w * h * spp and st["seconds_render"] > 0
    if flags != 0:
        assert (st["literal_retraces"], st["reference_lost_hits"], st["exact_ties"]) == (0, 0, 0)
    if watertight and not wide:
        # the emission channels are the oracle's own per-sample frame at max_bounces = 0
        ref = np.zeros((h, w, 3), np.int64)
        oracle_scene(oracle, "full_bsdf", True).render(default_camera(oracle, w / h), w, h, spp, max_bounces=0, threads=usable_cpus(),
                                                       fixed_out=ref, rng_mode="per_sample")
        assert np.array_equal(out.cpu().numpy()[:, ae.EMISSION:ae.EMISSION + 3], ref.reshape(-1, 3))


# ---- 2. the rare path: a scene shifted by 1e4 sends camera rays through the literal re-trace
def test_shifted_scene_takes_the_literal_retrace_and_equals_the_literal_oracle(api, torch, oracle):
    arrays, s3, t3 = placed_scenes.scene("shift_1e4", "full_bsdf")
    w, h, spp = 64, 48, 4
    osc = oracle.scene(arrays)  # literal
    want, want_ids, _ = ae.frame_expected(oracle, osc, placed_scenes.placed_camera(oracle.camera, s3, t3, w / h), w, h, spp)
    gpu = api.Scene(arrays)
    out, ids, st = gpu.render_aov(placed_scenes.placed_camera(api.make_camera, s3, t3, w / h), w, h, spp, ids=True)
    print("re-traced", st["literal_retraces"], "lost", st["reference_lost_hits"], "ties", st["exact_ties"])
    _assert_sums(out, want, "shift_1e4")
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert st["literal_retraces"] > 0  # the re-trace really ran
    gpu.close()
    osc.close()


# ---- 3. shards
@pytest.mark.parametrize("R", [2, 4])
def test_every_rank_is_its_subset_and_the_ranks_add_up(api, torch, oracle, R):
    w, h, spp = 19, 27, 4
    gpu = _gpu(api)
    cam = _camera(api, w, h)
    for name, flags, watertight in _modes(api):
        total = torch.zeros((w * h, ae.CHANNELS), dtype=torch.int64, device="cuda")
        for r in range(R):
            want, want_ids, _ = _frame(oracle, w, h, spp, watertight, shard=(r, R))
            out, ids, st = gpu.render_aov(cam, w, h, spp, flags=flags, shard=(r, R), ids=_poisoned_ids(torch, w * h))
            _assert_sums(out, want, (name, "rank", r, R))
            assert st["camera_rays"] == w * h * spp // R
            # only rank 0 touches the ids; the helper leaves the poison where a rank writes nothing
            assert np.array_equal(ids.cpu().numpy(), want_ids)
            assert r == 0 or bool((ids == POISON).all())
            gpu.render_aov(cam, w, h, spp, flags=flags, shard=(r, R), out=total)
        _assert_sums(total, _frame(oracle, w, h, spp, watertight)[0], (name, "ranks added", R))


# ---- 4. tables
def _pinhole(oracle, torch, w, h, spp):
    o, d, pixel = rk.keyed_pinhole_table(oracle, default_camera(oracle, w / h), w, h, spp, 1, range(w * h * spp))
    return _dev(torch, o), _dev(torch, d), pixel


def test_pinhole_table_is_the_camera_form_and_chunks_add_up(api, torch, oracle):
    w, h, spp = 64, 48, 4
    n = w * h * spp
    gpu = _gpu(api)
    o, d, pixel = _pinhole(oracle, torch, w, h, spp)
    for name, flags, watertight in _modes(api):
        cam_out, cam_ids, _ = gpu.render_aov(_camera(api, w, h), w, h, spp, flags=flags, ids=True)
        out, ids, st = gpu.render_aov_rays(o, d, w * h, rays_per_pixel=spp, flags=flags, ids=True)
        assert torch.equal(out, cam_out) and torch.equal(ids, cam_ids) and st["camera_rays"] == n
        _assert_sums(out, _frame(oracle, w, h, spp, watertight)[0], (name, "pinhole table"))
    # chunks cut at {1, 63, 64, 65, 4103} into one buffer, forwards and backwards (in the last mode of the loop above)
    cuts = [0, 1, 63, 64, 65, 4103, n]
    pieces = list(zip(cuts[:-1], cuts[1:]))
    for order in (pieces, pieces[::-1]):
        acc = torch.zeros((w * h, ae.CHANNELS), dtype=torch.int64, device="cuda")
        acc_ids = _poisoned_ids(torch, w * h)
        for a, b in order:
            gpu.render_aov_rays(o[a:b].contiguous(), d[a:b].contiguous(), w * h, rays_per_pixel=spp, key_first=a, flags=flags, out=acc, ids=acc_ids)
        assert torch.equal(acc, cam_out) and torch.equal(acc_ids, cam_ids)
    # rank r of R by stride
    acc = torch.zeros((w * h, ae.CHANNELS), dtype=torch.int64, device="cuda")
    for r in range(4):
        part, _, _ = gpu.render_aov_rays(o[r::4].contiguous(), d[r::4].contiguous(), w * h, rays_per_pixel=spp, key_first=r, key_stride=4,
                                         flags=api.FLAG_WATERTIGHT)
        _assert_sums(part, _frame(oracle, w, h, spp, True, shard=(r, 4))[0], ("stride rank", r))
        acc += part
    _assert_sums(acc, _frame(oracle, w, h, spp, True)[0], "stride ranks added")


def test_permuted_pixel_array_gives_the_permuted_sums(api, torch, oracle):
    w, h, spp = 19, 27, 3
    gpu = _gpu(api)
    o, d, pixel = _pinhole(oracle, torch, w, h, spp)
    perm = np.random.default_rng(3).permutation(w * h).astype(np.int32)
    out, ids, _ = gpu.render_aov_rays(o, d, w * h, pixel=_dev(torch, perm[pixel]))
    assert ids is None
    want = np.zeros((w * h, ae.CHANNELS), np.int64)
    want[perm] = _frame(oracle, w, h, spp, False)[0]
    _assert_sums(out, want, "permuted d_pixel")


def test_orthographic_table_and_keys_around_2_to_32(api, torch, oracle):
    """Rays no pinhole makes (parallel, from a grid in front of the box), against the helper on those rays; then the same rows
    under keys that cross 2^32 with 2^22 rays per pixel: the pixel is K // 2^22 in 64-bit arithmetic, and the one row whose key
    is a multiple of 2^22 writes its pixel's ids."""
    gpu = _gpu(api)
    g = 24
    xs, ys = np.meshgrid((np.arange(g) + 0.5) / g * 1.2 - 0.1, (np.arange(g) + 0.5) / g * 1.2 - 0.1)
    o = np.stack([xs.ravel(), ys.ravel(), np.full(g * g, 1.0)], 1).astype(np.float32)
    axis = np.array([0.1, -0.05, -1.0])
    d = np.tile((axis / np.linalg.norm(axis)).astype(np.float32), (g * g, 1))
    for name, flags, watertight in _modes(api):
        osc = oracle_scene(oracle, "full_bsdf", watertight)
        pixel = np.arange(g * g, dtype=np.int32)
        want, want_ids = ae.table_expected(oracle, osc, o, d, pixel, g * g, first=np.ones(g * g, bool))
        assert 0 < int((want[:, ae.HITS] == 0).sum()) < g * g
        out, ids, _ = gpu.render_aov_rays(_dev(torch, o), _dev(torch, d), g * g, flags=flags, ids=True)
        _assert_sums(out, want, (name, "orthographic"))
        assert np.array_equal(ids.cpu().numpy(), want_ids)
    rpp, first_key, n = 1 << 22, (1 << 32) - 100, 300
    keys = np.arange(first_key, first_key + n, dtype=np.int64)
    pixel = (keys // rpp).astype(np.int32)
    assert pixel.min() == 1023 and pixel.max() == 1024
    osc = oracle_scene(oracle, "full_bsdf", False)
    want, want_ids = ae.table_expected(oracle, osc, o[:n], d[:n], pixel, 1025, first=keys % rpp == 0)
    out, ids, _ = gpu.render_aov_rays(_dev(torch, o[:n]), _dev(torch, d[:n]), 1025, rays_per_pixel=rpp, key_first=first_key,
                                      ids=_poisoned_ids(torch, 1025))
    _assert_sums(out, want, "keys around 2^32")
    assert np.array_equal(ids.cpu().numpy(), want_ids) and bool((want_ids[1024] != POISON).all()) and bool((want_ids[:1024] == POISON).all())


# ---- 5. ids
def test_ids_are_the_triangle_and_material_of_each_pixels_first_sample(api, torch, oracle):
    w, h, spp = ae.WIDE_FRAME
    for name, flags, watertight in _modes(api):
        _, _, (tri, mat, _, _, _) = _frame(oracle, w, h, spp, watertight, True)
        _, ids, _ = _gpu(api).render_aov(_camera(api, w, h, True), w, h, spp, flags=flags, ids=True)
        got = ids.cpu().numpy()
        assert np.array_equal(got[:, 0], tri[::spp]) and np.array_equal(got[:, 1], mat[::spp])
        miss = tri[::spp] < 0
        assert miss.any() and (got[miss] == -1).all() and (got[~miss] >= 0).all()


# ---- 6. resolve
def test_resolve_is_the_numpy_restatement_bit_for_bit(api, torch, oracle):
    for (w, h, spp), wide in ((ae.WIDE_FRAME, True), ((64, 48, 4), False)):
        out, _, _ = _gpu(api).render_aov(_camera(api, w, h, wide), w, h, spp)
        sums = out.cpu().numpy()
        got = api.aov_resolve(out, spp).cpu().numpy()
        want = ae.resolve(sums, spp)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        empty = sums[:, ae.HITS] == 0
        assert (not wide or empty.any()) and (got[empty] == 0).all()
        full = sums[:, ae.HITS] == spp
        assert full.any() and (got[full, ae.HITS] == 1).all() and (got[full, ae.DEPTH] > 0).all()


# ---- 7. plumbing
def test_a_busy_non_default_stream(api, torch, oracle):
    w, h, spp = 64, 48, 4
    gpu = _gpu(api)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        acc = torch.full((w * h, ae.CHANNELS), 123, dtype=torch.int64, device="cuda")
        big = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
        for _ in range(8):
            big.fill_(1.0)  # a long fill in front: the stream is busy while the call is made
        acc.zero_()  # (ordered on s: the call must follow it)
        out, _, _ = gpu.render_aov(_camera(api, w, h), w, h, spp, out=acc)
        got = out.cpu().numpy()
    s.synchronize()
    _assert_sums(got, _frame(oracle, w, h, spp, False)[0], "busy stream")


def test_edited_moved_and_device_built_scenes_equal_a_scene_created_anew(api, torch, oracle, bunny_full_bsdf):
    w, h, spp = 64, 48, 4
    cam = _camera(api, w, h)
    gpu = api.Scene(bunny_full_bsdf)
    base = gpu.render_aov(cam, w, h, spp, ids=True)
    # set_materials: albedo follows
    mats = bunny_full_bsdf.materials.copy()
    mats["albedo"] = mats["albedo"][::-1] * np.float32(0.5)
    edited = dataclasses.replace(bunny_full_bsdf, materials=mats)
    gpu.set_materials(mats)
    out, ids, _ = gpu.render_aov(cam, w, h, spp, ids=True)
    anew = api.Scene(edited)
    ref, ref_ids, _ = anew.render_aov(cam, w, h, spp, ids=True)
    assert torch.equal(out, ref) and torch.equal(ids, ref_ids)
    assert not torch.equal(out[:, :3], base[0][:, :3]) and torch.equal(out[:, 3:], base[0][:, 3:])
    osc = oracle.scene(edited)
    _assert_sums(out, ae.frame_expected(oracle, osc, default_camera(oracle, w / h), w, h, spp)[0], "after set_materials")
    anew.close()
    osc.close()
    # update: depth and normal follow (the bunny's vertices pulled towards the camera and sheared)
    tris = np.asarray(edited.tris, np.float32).reshape(-1, 3, 3).copy()
    tris[:, :, 2] += np.float32(0.125) * tris[:, :, 0]
    moved = dataclasses.replace(edited, tris=np.ascontiguousarray(tris.reshape(-1, 9)))
    gpu.update(moved.tris)
    out2, ids2, _ = gpu.render_aov(cam, w, h, spp, ids=True)
    anew = api.Scene(moved)
    ref2, ref_ids2, _ = anew.render_aov(cam, w, h, spp, ids=True)
    assert torch.equal(out2, ref2) and torch.equal(ids2, ref_ids2)
    assert not torch.equal(out2[:, 3:6], out[:, 3:6]) and not torch.equal(out2[:, 9], out[:, 9])
    osc = oracle.scene(moved)
    _assert_sums(out2, ae.frame_expected(oracle, osc, default_camera(oracle, w / h), w, h, spp)[0], "after update")
    osc.close()
    # a device-built tree
    dev = api.Scene(moved, device_bvh=True)
    for name, flags, _ in _modes(api):
        a = dev.render_aov(cam, w, h, spp, flags=flags, ids=True)
        b = anew.render_aov(cam, w, h, spp, flags=flags, ids=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name
    for s in (gpu, anew, dev):
        s.close()


@pytest.mark.parametrize("env", [{"RT_BVH_WIDE": "0"}, {"RT_STACK_CAP": "2"}], ids=["pairs", "wide-overflow"])
def test_the_two_wide_tree_and_the_small_stack(api, torch, oracle, bunny_full_bsdf, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gpu = api.Scene(bunny_full_bsdf)
    o, d, _ = _pinhole(oracle, torch, 64, 48, 4)
    for w, h, spp, wide in ((64, 48, 4, False), ae.WIDE_FRAME + (True,)):
        for name, flags, watertight in _modes(api):
            want, want_ids, _ = _frame(oracle, w, h, spp, watertight, wide)
            out, ids, _ = gpu.render_aov(_camera(api, w, h, wide), w, h, spp, flags=flags, ids=True)
            _assert_sums(out, want, (env, name, wide))
            assert np.array_equal(ids.cpu().numpy(), want_ids)
    out, _, _ = gpu.render_aov_rays(o, d, 64 * 48, rays_per_pixel=4)
    _assert_sums(out, _frame(oracle, 64, 48, 4, False)[0], (env, "table"))
    gpu.close()


# ---- 8. refusals
def test_errors_name_the_entry_point_and_leave_the_buffers_untouched(api, torch, oracle):
    gpu = _gpu(api)
    w, h, spp = 8, 8, 4
    n = w * h * spp
    cam = _camera(api, w, h)
    o, d, pixel = _pinhole(oracle, torch, w, h, spp)
    buf = torch.full((w * h, ae.CHANNELS), POISON, dtype=torch.int64, device="cuda")
    ids = _poisoned_ids(torch, w * h)
    c = api.ctypes.c_void_p

    def untouched():
        torch.cuda.synchronize()
        assert bool((buf == POISON).all()) and bool((ids == POISON).all())

    def refused_camera(fragment, camera=cam, width=w, height=h, samples=spp, shard=(0, 1), flags=0, sums=True):
        rc = gpu.L.rt_render_aov_fixed(gpu.h, None if camera is None else camera.ctypes.data, width, height, samples, 1, shard[0], shard[1],
                                       flags, c(buf.data_ptr() if sums else None), c(ids.data_ptr()), None, None)
        msg = gpu.L.rt_last_error().decode()
        assert rc != 0 and msg.startswith("rt_render_aov_fixed: ") and fragment in msg, (fragment, rc, msg)
        untouched()

    def refused_rays(fragment, origins=o, dirs=d, pix=None, rpp=spp, n_pixels=w * h, key_first=0, key_stride=1, flags=0, sums=True,
                     with_ids=True, n_rays=None):
        rc = gpu.L.rt_render_aov_rays_fixed_device(gpu.h, n if n_rays is None else n_rays, c(None if origins is None else origins.data_ptr()),
                                                   c(None if dirs is None else dirs.data_ptr()), c(None if pix is None else pix.data_ptr()), rpp,
                                                   n_pixels, key_first, key_stride, flags, c(buf.data_ptr() if sums else None),
                                                   c(ids.data_ptr() if with_ids else None), None, None)
        msg = gpu.L.rt_last_error().decode()
        assert rc != 0 and msg.startswith("rt_render_aov_rays_fixed_device: ") and fragment in msg, (fragment, rc, msg)
        untouched()

    refused_camera("null camera", camera=None)
    refused_camera("null d_aov_fixed", sums=False)
    refused_camera("at least 1", width=0)
    refused_camera("at least 1", samples=0)
    refused_camera("int32 camera-ray range", width=32768, height=16384, samples=4)
    refused_camera("715827882 pixels", width=65536, height=16384, samples=1)
    refused_camera("not divisible by shard_count", shard=(0, 3))
    refused_camera("shard_index", shard=(2, 2))
    refused_camera("shard_index", shard=(0, 0))
    refused_camera("flags other than", flags=api.FLAG_DETERMINISTIC)
    refused_camera("flags other than", flags=api.FLAG_RNG_PER_SAMPLE)
    refused_camera("exclude each other", flags=api.FLAG_REFERENCE_WALK | api.FLAG_WATERTIGHT)

    refused_rays("null d_origin_xyz", origins=None)
    refused_rays("null d_dir_xyz", dirs=None)
    refused_rays("null d_aov_fixed", sums=False)
    refused_rays("flags other than", flags=api.FLAG_DETERMINISTIC)
    refused_rays("exclude each other", flags=api.FLAG_REFERENCE_WALK | api.FLAG_WATERTIGHT)
    refused_rays("d_ids together with d_pixel", pix=_dev(torch, pixel))
    refused_rays("n_rays = 0", n_rays=0)
    refused_rays("n_pixels = 0", n_pixels=0)
    refused_rays("key_stride = 0", key_stride=0)
    refused_rays("wraps 2^64", key_first=2 ** 64 - 10)
    refused_rays("rays_per_pixel = 0", rpp=0)
    refused_rays("falls on pixel", n_pixels=w * h - 1)
    refused_rays("falls on pixel", key_first=1)
    bad_pixel = pixel.copy()
    bad_pixel[[3, 77]] = (w * h, -1)
    refused_rays("2 of %d pixel indices" % n, pix=_dev(torch, bad_pixel), with_ids=False)
    bad_d = d.clone()
    bad_d[5, 1] = float("nan")
    bad_d[9, 0] = float("inf")
    bad_d[200, 2] = 2.0 ** 126
    refused_rays("3 of %d directions" % n, dirs=bad_d)
    # the wrapper raises with the library's message
    with pytest.raises(api.RtError, match="rt_render_aov_fixed: num_samples = 4 is not divisible by shard_count = 3"):
        gpu.render_aov(cam, w, h, spp, shard=(0, 3))
    # and the scene still renders
    out, _, _ = gpu.render_aov(cam, w, h, spp)
    _assert_sums(out, _frame(oracle, w, h, spp, False)[0], "after the refusals")
