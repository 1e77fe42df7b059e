"""GPU parity of RT_FLAG_RNG_PER_SAMPLE against the CPU oracle's restatement of that mode, bit for bit.  Run with -m gpu.

The mode is the product's own, not the reference's, but nothing in it is random once the seed is fixed:
camera ray G has the pixel G / spp and a stream that is a function of (seed, G), and its path is the reference's estimator on
that stream with the watertight hit definition.  So a frame has exactly ONE right array of fixed-point sums, which
oracle.cpp render_per_sample states as a loop over camera rays -- no slots, no chunks, no waves -- and every case here holds
`rt_render_shard_fixed(..., RT_FLAG_RNG_PER_SAMPLE)` to it: all w * h * 3 int64 sums EQUAL and six event totals EQUAL, no
tolerance, no masked pixel.

The cases walk the code paths of the builds the mode runs: the DRAW_CIDS build of k_paths (camera-ray ids drawn 512 at a time
from the frame's counter: ray counts around the wave, chunk and pool sizes; several generations), its `few_blocks` build (ids
tied to slots; RT_PATHS_BLOCKS), tables in LDS and in global memory, both tree widths, the overflow stack, trees built and
rebuilt on the device, the key arithmetic of the shards, seeds whose high word matters, and the float and multi-device entry
points.
"""
import dataclasses

import numpy as np
import pytest

from conftest import default_camera, oracle_scene, usable_cpus

pytestmark = pytest.mark.gpu

W = 1 << 20
KEYS = ("camera_rays", "shade_events", "any_rays", "emission_adds", "shadow_adds", "rr_draws")
ALL_ONES_HIGH = 0xFFFFFFFF00000007  # a seed with every bit of the high word set


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()  # raises if the HIP library is missing: there is no fallback
    return _api


_gpu_cache = {}


def _gpu(api, variant):
    if variant not in _gpu_cache:
        from rtcuda_amd import scenes
        _gpu_cache[variant] = api.Scene(scenes.cornell_bunny(variant))
    return _gpu_cache[variant]


def _oracle_sums(oracle, osc, w, h, spp, max_bounces=10, seed=1, shard=(0, 1), cam=None):
    """(fixed sums (h, w, 3) int64, post-processed image, the six event totals under the product's names) of the oracle's frame."""
    want = np.zeros((h, w, 3), np.int64)
    cam = default_camera(oracle, w / h) if cam is None else cam
    img, _, st = osc.render(cam, w, h, spp, max_bounces=max_bounces, seed=seed, threads=usable_cpus(), fixed_out=want,
                            rng_mode="per_sample", shard=shard)
    assert st["ch_adds"] == 0  # the one ray kind the product does not trace never contributes
    ev = {"camera_rays": st["sum_gen"], "shade_events": st["sum_mat"], "any_rays": st["sum_ah"],
          "emission_adds": st["emission_adds"], "shadow_adds": st["ah_adds"], "rr_draws": st["rr_draws"]}
    return want, img, ev


def _gpu_sums(api, gpu, w, h, spp, max_bounces=10, seed=1, shard=(0, 1), flags=0):
    import torch
    got = torch.zeros(h * w * 3, dtype=torch.int64, device="cuda")
    st = gpu.render_shard_fixed(api.make_camera(aspect=w / h), w, h, spp, shard[0], shard[1], got.data_ptr(),
                                max_bounces=max_bounces, seed=seed, flags=flags | api.FLAG_RNG_PER_SAMPLE)
    torch.cuda.synchronize()
    return got.cpu().numpy().reshape(h, w, 3), {k: st[k] for k in KEYS}


def _assert_equal(got, ev_g, want, ev_c, what=""):
    """Every sum and every event total; on a mismatch: how many sums differ and the first few (y, x, channel)."""
    bad = got != want
    assert not bad.any(), (what, "sums that differ: %d of %d" % (int(bad.sum()), bad.size), "first (y, x, channel):",
                           np.argwhere(bad)[:6].tolist(), "got", got[bad][:6].tolist(), "want", want[bad][:6].tolist())
    assert ev_g == ev_c, (what, ev_g, ev_c)


def _check(api, oracle, variant, w, h, spp, max_bounces=10, seed=1, shard=(0, 1)):
    osc = oracle_scene(oracle, variant, True)
    want, _, ev_c = _oracle_sums(oracle, osc, w, h, spp, max_bounces, seed, shard)
    got, ev_g = _gpu_sums(api, _gpu(api, variant), w, h, spp, max_bounces, seed, shard)
    assert ev_c["camera_rays"] == w * h * spp // shard[1]
    _assert_equal(got, ev_g, want, ev_c, (variant, w, h, spp, max_bounces, seed, shard))
    return want, ev_c


# ---------------------------------------------------------------------------------------------- frames with spp = 1
# Each pixel is ONE camera ray, so a mismatch names the ray.  Ray counts around a wave (64), a chunk of camera-ray ids (512) and
# the slot pool (W = 1 048 576 = 1024 x 1024; W - 1 = 1025 x 1023; W + 1 = 61681 x 17), as columns (1 x n: the rays sweep the
# scene top to bottom) and as rows.
ONE_SPP_FRAMES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 511), (1, 512), (1, 513), (63, 1), (65, 1), (513, 1), (19, 27),
                  (1025, 1023), (1024, 1024), (61681, 17)]


@pytest.mark.parametrize("w,h", ONE_SPP_FRAMES, ids=[f"{w}x{h}" for w, h in ONE_SPP_FRAMES])
def test_one_sample_per_pixel_frames_are_the_oracles_ray_for_ray(api, oracle, w, h):
    want, ev = _check(api, oracle, "full_bsdf", w, h, 1)
    if w * h >= 511 and w == 1:
        assert ev["shade_events"] > w * h // 4 and want.any()  # (the column looks at the scene)


# ---------------------------------------------------------------------------------------------- several generations
MULTIGEN = [
    # variant, w, h, spp, max_bounces, seed
    ("full_bsdf", 301, 199, 48, 10, 1),       # 2.7 W rays: a multiple of neither 512 (5 615.5 chunks) nor W
    ("full_bsdf", 300, 200, 48, 10, 1),       # (exactly 5 625 chunks)
    ("matte", 240, 135, 256, 10, 1),          # 7.9 W rays
    ("sixteen_lights", 320, 180, 40, 10, 1),
    ("four_bunnies", 320, 180, 40, 10, 1),    # the deep tree: global overflow stack in k_paths
]


@pytest.mark.parametrize("variant,w,h,spp,max_bounces,seed", MULTIGEN)
def test_multi_generation_frames_equal_the_oracle_bit_for_bit(api, oracle, variant, w, h, spp, max_bounces, seed):
    assert w * h * spp > 2 * W
    want, ev = _check(api, oracle, variant, w, h, spp, max_bounces, seed)
    assert ev["shade_events"] > w * h * spp // 2 and ev["rr_draws"] > 0 and ev["emission_adds"] > 0


def test_a_frame_with_a_non_finite_contribution(api, oracle):
    """full_bsdf 300x200x48 with seed 14 (found by a search over seeds on the CPU: seeds 1 - 13 have none): the oracle's float
    sums of pixel (y 5, x 53) are not finite -- a camera ray whose three-float sum is NaN or Inf, which to_fixed drops (NaN)
    or clamps (Inf) per channel.  The fixed-point sums must still be the oracle's everywhere, and the float entry point must
    show the non-finite pixel where the oracle's image has it."""
    w, h, spp, seed = 300, 200, 48, 14
    osc = oracle_scene(oracle, "full_bsdf", True)
    _, raw, _ = osc.render(default_camera(oracle, w / h), w, h, spp, seed=seed, threads=usable_cpus(), rng_mode="per_sample")
    bad = ~np.isfinite(raw).all(axis=2)
    assert 1 <= bad.sum() <= 3 and bad[5, 53]
    _check(api, oracle, "full_bsdf", w, h, spp, seed=seed)
    _, img_c, _ = _oracle_sums(oracle, osc, w, h, spp, seed=seed)
    img_g, _ = _gpu(api, "full_bsdf").render(api.make_camera(aspect=w / h), w, h, spp, seed=seed, flags=api.FLAG_RNG_PER_SAMPLE)
    assert np.array_equal(np.isfinite(img_g), np.isfinite(img_c)) and not np.isfinite(img_g[5, 53]).all()


def test_run_twice_gives_the_same_array(api, oracle):
    w, h, spp = 300, 200, 48
    a, ev_a = _gpu_sums(api, _gpu(api, "full_bsdf"), w, h, spp)
    b, ev_b = _gpu_sums(api, _gpu(api, "full_bsdf"), w, h, spp)
    assert np.array_equal(a, b) and ev_a == ev_b


# ---------------------------------------------------------------------------------------------- seeds and bounces
@pytest.mark.parametrize("seed", [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, ALL_ONES_HIGH], ids=hex)
def test_seeds_on_both_sides_of_the_32_bit_boundary(api, oracle, seed):
    """seed_lo and seed_hi both reach the key: seeds that differ only in the high word give different frames, each the oracle's."""
    want, _ = _check(api, oracle, "full_bsdf", 160, 90, 16, seed=seed)
    other, _, _ = _oracle_sums(oracle, oracle_scene(oracle, "full_bsdf", True), 160, 90, 16, seed=seed ^ (1 << 32))
    assert not np.array_equal(want, other)  # (the oracle itself: the high word matters)


@pytest.mark.parametrize("max_bounces", [0, 1, 2, 10])
def test_max_bounces(api, oracle, max_bounces):
    want, ev = _check(api, oracle, "full_bsdf", 256, 144, 40, max_bounces=max_bounces)  # 1.4 W rays
    assert (ev["shade_events"] == 0) == (max_bounces == 0)
    assert ev["emission_adds"] > 0 and want.any()


# ---------------------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("shards", [2, 4, 8])
def test_every_rank_of_a_sharded_frame_is_the_oracles_subset(api, oracle, shards):
    """Rank r of R renders the camera rays G with G % R == r (key = local id * R + r): each rank against the oracle's (r, R)
    subset -- not only the ranks' total against the GPU's own 1-rank frame."""
    w, h, spp = 240, 135, 64  # 2 W rays
    total = np.zeros((h, w, 3), np.int64)
    for r in range(shards):
        want, ev = _check(api, oracle, "full_bsdf", w, h, spp, shard=(r, shards))
        assert ev["camera_rays"] == w * h * spp // shards
        total += want
    full, _, _ = _oracle_sums(oracle, oracle_scene(oracle, "full_bsdf", True), w, h, spp)
    assert np.array_equal(total, full)


@pytest.mark.parametrize("shards", [2, 8])
def test_a_shard_with_fewer_rays_than_one_chunk(api, oracle, shards):
    w, h, spp = 9, 7, 8  # 504 rays: 252 / 63 per rank
    for r in range(shards):
        _check(api, oracle, "full_bsdf", w, h, spp, shard=(r, shards))


@pytest.mark.parametrize("blocks", ["512", "64"])
def test_the_few_blocks_build_with_per_sample_streams(api, oracle, monkeypatch, blocks):
    """A grid of at most two workgroups per CU launches the MIN_WAVES = 2 build: gen() inside the ADV block, camera-ray ids tied
    to slots (id = generation * W + slot) instead of drawn from the counter, the stream re-seeded from the same key."""
    monkeypatch.setenv("RT_PATHS_BLOCKS", blocks)
    _check(api, oracle, "full_bsdf", 300, 200, 48)
    _check(api, oracle, "full_bsdf", 240, 135, 64, shard=(3, 4))
    _check(api, oracle, "full_bsdf", 1, 513, 1)


# ---------------------------------------------------------------------------------------------- tables, trees, stacks
def test_more_than_64_materials(api, oracle):
    """Shading tables in global memory (the LDS_TABLES = false build)."""
    import table_scenes as ts
    arrays = ts.table_scene(200, 100)
    assert not ts.lds_tables(200, 100)
    w, h, spp = 256, 144, 40
    gpu = api.Scene(arrays)
    want, _, ev_c = _oracle_sums(oracle, oracle.scene(arrays).set_watertight(True), w, h, spp)
    got, ev_g = _gpu_sums(api, gpu, w, h, spp)
    gpu.close()
    _assert_equal(got, ev_g, want, ev_c, "table_scene(200, 100)")


@pytest.mark.parametrize("variant", ["full_bsdf", "four_bunnies"])
def test_binary_tree_and_overflow_stack(api, oracle, monkeypatch, variant):
    """RT_STACK_CAP=2 (nearly every push through the global overflow column) on the 4-wide tree, and RT_BVH_WIDE=0 (read at
    scene creation) with and without it: the mode accepts both, and hits do not depend on the tree."""
    from rtcuda_amd import scenes
    w, h, spp = 256, 144, 40
    osc = oracle_scene(oracle, variant, True)
    want, _, ev_c = _oracle_sums(oracle, osc, w, h, spp)
    monkeypatch.setenv("RT_STACK_CAP", "2")
    got, ev_g = _gpu_sums(api, _gpu(api, variant), w, h, spp)
    _assert_equal(got, ev_g, want, ev_c, "RT_STACK_CAP=2")
    monkeypatch.setenv("RT_BVH_WIDE", "0")
    pairs = api.Scene(scenes.cornell_bunny(variant))
    monkeypatch.delenv("RT_BVH_WIDE")
    got, ev_g = _gpu_sums(api, pairs, w, h, spp)
    _assert_equal(got, ev_g, want, ev_c, "RT_BVH_WIDE=0 RT_STACK_CAP=2")
    monkeypatch.delenv("RT_STACK_CAP")
    got, ev_g = _gpu_sums(api, pairs, w, h, spp)
    pairs.close()
    _assert_equal(got, ev_g, want, ev_c, "RT_BVH_WIDE=0")


def _moved(arrays):
    """The scene with the bunny shifted and squeezed a little (every bunny vertex moves; walls and lights stay)."""
    tris = np.array(arrays.tris, np.float32)
    n_bunny = arrays.n_tris - 12
    v = tris[:n_bunny].reshape(-1, 3, 3)
    v = v * np.array([0.9, 1.05, 0.9], np.float32) + np.array([0.07, 0.0, -0.04], np.float32)
    tris[:n_bunny] = v.reshape(-1, 9).astype(np.float32)
    return tris


def test_trees_built_and_rebuilt_on_the_device(api, oracle, bunny_full_bsdf):
    """A scene created with RT_SCENE_DEVICE_BVH, and one after rt_scene_update + rt_scene_rebuild: the same bits as the oracle's
    frame of the same triangles."""
    w, h, spp = 256, 144, 40
    want, _, ev_c = _oracle_sums(oracle, oracle_scene(oracle, "full_bsdf", True), w, h, spp)
    dev = api.Scene(bunny_full_bsdf, device_bvh=True)
    got, ev_g = _gpu_sums(api, dev, w, h, spp)
    _assert_equal(got, ev_g, want, ev_c, "RT_SCENE_DEVICE_BVH")
    new = _moved(bunny_full_bsdf)
    want2, _, ev_c2 = _oracle_sums(oracle, oracle.scene(dataclasses.replace(bunny_full_bsdf, tris=new)).set_watertight(True), w, h, spp)
    assert not np.array_equal(want, want2)
    dev.update(new)
    got, ev_g = _gpu_sums(api, dev, w, h, spp)
    _assert_equal(got, ev_g, want2, ev_c2, "rt_scene_update")
    dev.rebuild()
    got, ev_g = _gpu_sums(api, dev, w, h, spp)
    dev.close()
    _assert_equal(got, ev_g, want2, ev_c2, "rt_scene_update + rt_scene_rebuild")


# ---------------------------------------------------------------------------------------------- the other entry points
def test_rt_render_with_float_atomics(api, oracle):
    """rt_render (float atomics) with the flag against the oracle's post-processed image, in the band of the reference-mode
    float test (test_multi_generation_render_against_the_literal_reference_fixture): at most 2 pixels over 1e-4, RMS under
    1e-4, the same NaN mask.  The accumulation is the same -- one float triple per camera ray -- so the same band applies."""
    w, h, spp = 300, 200, 48
    _, img_c, ev_c = _oracle_sums(oracle, oracle_scene(oracle, "full_bsdf", True), w, h, spp)
    img_g, st = _gpu(api, "full_bsdf").render(api.make_camera(aspect=w / h), w, h, spp, flags=api.FLAG_RNG_PER_SAMPLE)
    assert {k: st[k] for k in KEYS} == ev_c
    assert np.array_equal(np.isnan(img_g), np.isnan(img_c))
    d = np.nan_to_num(np.abs(img_g.astype(np.float64) - img_c))
    print("float image: pixels over 1e-4:", int((d.max(axis=2) > 1e-4).sum()), "rms:", float(np.sqrt(np.mean(d ** 2))))
    assert (d.max(axis=2) > 1e-4).sum() <= 2
    assert np.sqrt(np.mean(d ** 2)) < 1e-4


def test_rt_render_multi_over_four_shards_of_one_device(api, oracle):
    """rt_render_multi(..., RT_FLAG_DETERMINISTIC | RT_FLAG_RNG_PER_SAMPLE, devices = [0, 0, 0, 0]): four shards summed in fixed
    point and post-processed -- the image of the oracle's sums, bit for bit (sqrt(sum * 2^-30 / spp) in fp32, as
    rt_post_process_fixed computes it from the same integers)."""
    import torch
    w, h, spp = 240, 135, 64
    want, _, ev_c = _oracle_sums(oracle, oracle_scene(oracle, "full_bsdf", True), w, h, spp)
    gpu = _gpu(api, "full_bsdf")
    img, st = gpu.render_multi(api.make_camera(aspect=w / h), w, h, spp, [0, 0, 0, 0],
                               flags=api.FLAG_DETERMINISTIC | api.FLAG_RNG_PER_SAMPLE)
    assert st["device_shards"] == 4 and {k: st[k] for k in KEYS} == ev_c
    fixed = torch.from_numpy(want.reshape(-1)).cuda()
    out = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    api.post_process_fixed(fixed.data_ptr(), out.data_ptr(), w * h, spp)
    torch.cuda.synchronize()
    ref = out.cpu().numpy().reshape(h, w, 3)
    bad = img.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:6].tolist())
