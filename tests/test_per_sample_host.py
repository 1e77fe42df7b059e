"""The oracle's per-sample mode (oracle.cpp render_per_sample: RT_FLAG_RNG_PER_SAMPLE restated as a loop over camera rays),
checked on the CPU: its key function against an independent restatement and published known answers, no two camera rays
sharing a stream, shards and thread counts, a frame recomputed ray by ray without the path code, and the estimator against
the slot-mode oracle.  tests/test_gpu_per_sample.py holds the GPU to this mode bit for bit."""
import numpy as np

from conftest import default_camera, usable_cpus

M64 = (1 << 64) - 1
# the first three outputs of splitmix64 seeded with 0 (Steele, Lea, Flood 2014; Vigna's splitmix64.c: x += 0x9e3779b97f4a7c15,
# then the finaliser) -- the published test vector of the algorithm
SPLITMIX64_OF_0 = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def splitmix_word(seed, key):
    """Test-side restatement in Python integers: the (key + 1)-th output of splitmix64 started at `seed`."""
    z = (seed + 0x9E3779B97F4A7C15 * (key + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _per_sample(osc, cam, w, h, spp, threads=None, **kw):
    fx = np.zeros((h, w, 3), np.int64)
    img, raw, st = osc.render(cam, w, h, spp, threads=threads or usable_cpus(), fixed_out=fx, rng_mode="per_sample", **kw)
    return fx, img, raw, st


EVENTS = ("sum_mat", "sum_gen", "sum_ah", "sum_ch", "emission_adds", "ah_adds", "ch_adds", "rr_draws", "rr_kills")


def test_key_function_against_an_independent_restatement(oracle):
    for seed in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1):
        for key in (0, 1, 2 ** 31 - 1, 2 ** 32, 2 ** 52):
            z = splitmix_word(seed, key)
            assert oracle.sample_stream(seed, key).tolist() == oracle.xorwow_init(z, 0).tolist(), (seed, key)
            assert int(oracle.sample_stream_words(seed, key, 1)[0]) == z
    # seed_lo / seed_hi and the width of the key all matter
    states = {tuple(oracle.sample_stream(s, k).tolist()) for s in (1, 1 << 32, (1 << 32) + 1) for k in (0, 1 << 32, 1 << 33)}
    assert len(states) == 9


def test_key_function_gives_the_published_splitmix64_outputs(oracle):
    assert [splitmix_word(0, k) for k in range(3)] == SPLITMIX64_OF_0
    for k, z in enumerate(SPLITMIX64_OF_0):
        assert oracle.sample_stream(0, k).tolist() == oracle.xorwow_init(z, 0).tolist()
    assert oracle.sample_stream_words(0, 0, 3).tolist() == SPLITMIX64_OF_0


def test_no_two_camera_rays_share_a_stream(oracle):
    """The first 2^22 keys of two seeds, as 64-bit words (the seed scramble behind them is a bijection of the word: two odd
    multipliers and xors), against a vectorised restatement too."""
    n = 1 << 22
    words = []
    for seed in (1, 2 ** 32 + 1):
        got = oracle.sample_stream_words(seed, 0, n)
        with np.errstate(over="ignore"):
            z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (np.arange(n, dtype=np.uint64) + np.uint64(1))
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        assert np.array_equal(got, z)
        words.append(got)
    allw = np.concatenate(words)
    assert np.unique(allw).size == allw.size


def test_shards_add_up_exactly(oracle, bunny_full_bsdf):
    w, h, spp = 48, 27, 24
    osc = oracle.scene(bunny_full_bsdf)
    cam = default_camera(oracle, w / h)
    full, _, _, st = _per_sample(osc, cam, w, h, spp)
    assert st["sum_gen"] == w * h * spp and full.any()
    for R in (2, 3, 8):
        acc = np.zeros_like(full)
        tot = {k: 0 for k in EVENTS}
        for r in range(R):
            fx, _, _, s = _per_sample(osc, cam, w, h, spp, shard=(r, R))
            assert s["sum_gen"] == w * h * spp // R
            acc += fx
            for k in EVENTS:
                tot[k] += s[k]
        assert np.array_equal(acc, full), R
        assert tot == {k: st[k] for k in EVENTS}, R


def test_thread_count_changes_nothing(oracle, bunny_full_bsdf):
    w, h, spp = 64, 36, 16
    osc = oracle.scene(bunny_full_bsdf)
    cam = default_camera(oracle, w / h)
    a = _per_sample(osc, cam, w, h, spp, threads=1)
    b = _per_sample(osc, cam, w, h, spp, threads=max(2, usable_cpus()))
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert {k: a[3][k] for k in EVENTS} == {k: b[3][k] for k in EVENTS}


def test_the_mode_keeps_the_watertight_hits_whatever_the_scene_says(oracle, bunny_full_bsdf):
    w, h, spp = 64, 36, 16
    cam = default_camera(oracle, w / h)
    a = _per_sample(oracle.scene(bunny_full_bsdf), cam, w, h, spp)
    b = _per_sample(oracle.scene(bunny_full_bsdf).set_watertight(True), cam, w, h, spp)
    assert np.array_equal(a[0], b[0])


def test_max_bounces_0_is_bounce_0_emission_recomputed_ray_by_ray(oracle, bunny_full_bsdf):
    """max_bounces = 0: a camera ray contributes the radiance of the light it hits, nothing else.  Recomputed here from the
    stream's first two draws (x, then y), camera_get_ray and exhaustive search over the triangles alone -- which pins the
    jitter order, the pixel mapping, the stream seeding and the shard rule without any of the path code."""
    w, h, spp, seed = 24, 32, 6, 2 ** 32 + 5
    cam = oracle.camera((0.5, 0.6, -0.5), (0.5, 1.0, -0.5), (0.0, 0.0, -1.0), 60.0, w / h)  # (above the bunny, looks up at the light)
    osc = oracle.scene(bunny_full_bsdf)
    n = w * h * spp
    o3, d3 = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    for G in range(n):
        pixel = G // spp
        st = oracle.sample_stream(seed, G)
        _, u = oracle.xorwow_draw(st, 2)
        x = (np.float32(pixel % w) + u[0]) / np.float32(w)
        y = (np.float32(pixel // w) + u[1]) / np.float32(h)
        ray = oracle.camera_get_ray(cam, float(x), float(y))
        o3[G], d3[G] = ray[:3], ray[3:]
    tri, _, _, _ = osc.trace_closest_brute(o3, d3, np.full(n, np.finfo(np.float32).max, np.float32), threads=usable_cpus())
    light_of = np.asarray(bunny_full_bsdf.tri_light)
    L = np.asarray(bunny_full_bsdf.lights["L"], np.float32)
    for shard in ((0, 1), (1, 3)):
        want = np.zeros((h, w, 3), np.int64)
        emitted = 0
        for G in range(shard[0], n, shard[1]):
            if tri[G] >= 0 and light_of[tri[G]] >= 0:
                rgb = L[light_of[tri[G]]]
                want.reshape(-1, 3)[G // spp] += np.rint(rgb.astype(np.float64) * 2.0 ** 30).astype(np.int64)
                emitted += 1
        fx, _, _, s = _per_sample(osc, cam, w, h, spp, max_bounces=0, seed=seed, shard=shard)
        assert emitted > n // (20 * shard[1]) and s["emission_adds"] == emitted
        assert s["sum_mat"] == 0 and s["sum_ah"] == 0 and s["rr_draws"] == 0 and s["sum_gen"] == n // shard[1]
        assert np.array_equal(fx, want), (shard, np.argwhere(fx != want)[:4].tolist())


def test_same_estimator_as_the_slot_mode_oracle(oracle, bunny_matte):
    """Against the watertight slot-mode oracle on the matte scene, in the band of
    test_per_sample_rng_mode_is_partition_invariant_and_statistically_equivalent (tests/test_gpu_multigen.py, same frame): the
    median absolute difference within 0.8 - 1.25 x of the seed-to-seed noise of the slot mode, mean radiance and shade events
    within 0.5 %."""
    w, h, spp = 240, 135, 256
    osc = oracle.scene(bunny_matte).set_watertight(True)
    cam = default_camera(oracle, w / h)
    _, img_ps, _, st_ps = _per_sample(osc, cam, w, h, spp)
    img_a, _, st_a = osc.render(cam, w, h, spp, seed=1, threads=usable_cpus())
    img_b, _, _ = osc.render(cam, w, h, spp, seed=2, threads=usable_cpus())

    def mad(x, y):
        return float(np.nanmedian(np.abs(x.astype(np.float64) - y)))
    noise = mad(img_a, img_b)
    assert noise > 0
    print("mad", mad(img_ps, img_a), "noise", noise, "means", np.nanmean(img_ps), np.nanmean(img_a), "shades", st_ps["sum_mat"], st_a["sum_mat"])
    assert 0.8 * noise < mad(img_ps, img_a) < 1.25 * noise, (mad(img_ps, img_a), noise)
    assert abs(np.nanmean(img_ps) - np.nanmean(img_a)) < 0.005 * np.nanmean(img_a)
    assert abs(st_ps["sum_mat"] - st_a["sum_mat"]) < 0.005 * st_a["sum_mat"]
