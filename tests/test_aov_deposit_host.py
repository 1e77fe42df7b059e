"""CPU side of tests/test_gpu_aov_deposit.py: the expected arrays those tests compare with hold what each case claims to reach
-- pixels that every sample hits, pixels that some miss, empty pixels, negative sums, pixel arrays with the run lengths their
names promise, values at every edge of to_fixed, sums at every edge of the resolve -- so that no GPU test passes for want of
content.  Nothing here renders."""
import numpy as np
import pytest

from conftest import default_camera, oracle_scene
import aov_expected as ae
import raytable_keyed as rk


def _camera(oracle, w, h, wide):
    return ae.wide_camera(oracle.camera, w / h) if wide else default_camera(oracle, w / h)


# ---- 1. frames with long runs
@pytest.mark.parametrize("watertight", [False, True], ids=["literal", "watertight"])
def test_long_run_frames_hold_full_partial_and_empty_pixels_and_negative_sums(oracle, watertight):
    osc = oracle_scene(oracle, "full_bsdf", watertight)
    for w, h, spp, wide in ae.DEPOSIT_FRAMES:
        sums, ids, (tri, mat, vals, pixel, keys) = ae.frame_expected(oracle, osc, _camera(oracle, w, h, wide), w, h, spp)
        full, partial, empty = ae.frame_census(sums, spp)
        print("%dx%dx%d%s %s: full %d partial %d empty %d, runs of rows per pixel %s" %
              (w, h, spp, " wide" if wide else "", "watertight" if watertight else "literal", full, partial, empty, ae.run_histogram(pixel)))
        assert ae.run_histogram(pixel) == {spp: w * h}
        assert np.array_equal(ae.exact_sums(tri, vals, pixel, w * h), sums)
        assert int(sums[:, ae.HITS].sum()) == int((tri >= 0).sum()) > 0
        assert (sums[:, ae.NORMAL:ae.NORMAL + 3] < 0).any()  # negative sums, from the normals
        assert not (ids == -7).any()
        if (w, h, spp) in ((4, 3, 64), (8, 6, 16), (5, 4, 64)):
            assert partial >= 1, "no pixel with 0 < hits < spp"
        if spp == 64:  # (a full wave of one pixel in which every lane deposits; 2 x 2 x 200 and 1 x 1 x 1000 have no such pixel)
            assert full >= 1, "no pixel that every sample hits"
        if wide:
            assert empty >= 1, "no empty pixel in the wide frame"
        if (w, h, spp) == (1, 1, 1000):
            assert full + partial == 1  # every deposit of the frame lands on one address
        if not watertight:  # what the literal oracle gives for the frames whose content the suite leans on
            want = {(4, 3, 64): (2, 10, 0), (8, 6, 16): (19, 17, 12), (5, 4, 64): (1, 8, 11)}.get((w, h, spp))
            assert want is None or (full, partial, empty) == want, (w, h, spp, full, partial, empty)


def test_shards_of_the_one_pixel_chunk_frame_add_up(oracle):
    w, h, spp = ae.DEPOSIT_SHARD_FRAME
    for watertight in (False, True):
        osc = oracle_scene(oracle, "full_bsdf", watertight)
        cam = default_camera(oracle, w / h)
        whole, ids, _ = ae.frame_expected(oracle, osc, cam, w, h, spp)
        parts = [ae.frame_expected(oracle, osc, cam, w, h, spp, shard=(r, 4)) for r in range(4)]
        assert np.array_equal(sum(p[0] for p in parts), whole) and np.array_equal(parts[0][1], ids)
        for r, (sums, part_ids, (tri, _, _, pixel, keys)) in enumerate(parts):
            assert ae.run_histogram(pixel) == {spp // 4: w * h} and (keys % 4 == r).all()  # local spp 16
            assert int(sums[:, ae.HITS].sum()) > 0 and (r == 0 or (part_ids == -7).all())
        for r in (0, 37):
            sums, part_ids, (tri, _, _, pixel, keys) = ae.frame_expected(oracle, osc, cam, w, h, spp, shard=(r, 64))
            assert ae.run_histogram(pixel) == {1: w * h}  # local spp 1: no run at all
            assert 0 < int(sums[:, ae.HITS].sum()) == int((tri >= 0).sum()) and (sums[:, ae.HITS] <= 1).all()


# ---- 2. crafted pixel arrays
def _base_table(oracle):
    w, h, spp = ae.DEPOSIT_BASE_TABLE
    return rk.keyed_pinhole_table(oracle, default_camera(oracle, w / h), w, h, spp, 1, range(w * h * spp))


@pytest.mark.parametrize("watertight", [False, True], ids=["literal", "watertight"])
def test_crafted_pixel_arrays_have_the_runs_they_claim(oracle, watertight):
    o, d, _ = _base_table(oracle)
    tri, mat, vals = ae.sample_features(oracle, oracle_scene(oracle, "full_bsdf", watertight), o, d)
    n = tri.size
    n_hit = int((tri >= 0).sum())
    assert n == 12288 and n_hit >= 0.2 * n and n - n_hit >= 0.2 * n, (n, n_hit)
    cases = {name: (rows, pixel, n_pixels, claim) for name, rows, pixel, n_pixels, claim in ae.table_cases(tri)}
    assert sorted(cases) == sorted(["H-full-waves", "H-split-across-chunks", "H-one-address", "H-alternating", "B-drawn-runs",
                                    "B-descending-sevens", "M-nothing-deposits", "H-interleaved-halves"])
    for name, (rows, pixel, n_pixels, claim) in cases.items():
        hist = ae.run_histogram(pixel)
        print(name, "rows", rows.size, "n_pixels", n_pixels, "runs", hist)
        assert hist == claim, (name, hist, claim)
        hits = tri[rows] >= 0
        assert hits.all() if name[0] == "H" else not hits.any() if name[0] == "M" else (hits.any() and not hits.all())
        want = ae.deposit(tri[rows], vals[rows], pixel, n_pixels)
        assert int(want[:, ae.HITS].sum()) == int(hits.sum())
        assert np.array_equal(want[:, ae.HITS], np.bincount(pixel[hits], minlength=n_pixels))
    longest = {name: max(ae.run_histogram(c[1])) for name, c in cases.items()}
    assert longest["H-full-waves"] == longest["H-split-across-chunks"] == 64 and longest["H-alternating"] == 1
    assert longest["H-one-address"] == n_hit and longest["H-interleaved-halves"] == 1 and longest["B-descending-sevens"] == 7
    # full waves: all but the last pixel take 64 hits; split: the first run is the half one
    assert (np.bincount(cases["H-full-waves"][1])[:-1] == 64).all() and ae.run_lengths(cases["H-split-across-chunks"][1])[0] == 32
    # one address: pixels 0 and 2 of the three stay empty
    rows, pixel, n_pixels, _ = cases["H-one-address"]
    want = ae.deposit(tri[rows], vals[rows], pixel, n_pixels)
    assert n_pixels == 3 and not want[0].any() and not want[2].any() and want[1, ae.HITS] == n_hit
    # drawn runs: every length of the set occurs, every pixel comes back in separate runs, and misses cut the runs
    rows, pixel, n_pixels, claim = cases["B-drawn-runs"]
    assert set(claim) >= set(ae.FIBONACCI_RUNS) and n_pixels == 16
    starts = np.concatenate([[0], np.cumsum(ae.run_lengths(pixel))[:-1]])
    assert (np.bincount(pixel[starts], minlength=16) >= 2).all()
    cut = [0 < int((tri[s:s + k] >= 0).sum()) < k for s, k in zip(starts, ae.run_lengths(pixel)) if k >= 34]
    assert sum(cut) >= 10, sum(cut)
    # interleaved: every pixel but the last of each half occurs 64 times, never in two neighbouring rows
    rows, pixel, n_pixels, _ = cases["H-interleaved-halves"]
    assert (np.bincount(pixel)[:rows.size // 2 // 64] == 64).all() and (pixel[1:] != pixel[:-1]).all()
    # descending: the pixels fall
    assert (np.diff(cases["B-descending-sevens"][1]) <= 0).all()


def test_key_cases_lie_where_they_claim(oracle):
    # rays_per_pixel = 64 under keys that cross 2^32: runs of 64, the first cut to 36
    keys = ae.KEYS_FIRST + np.arange(ae.KEYS_ROWS, dtype=np.int64)
    pixel = keys // ae.KEYS_RPP
    assert keys[0] < 1 << 32 <= keys[-1] and pixel[0] == 67108862 and pixel.max() < 0x7fffffff // 3
    hist = ae.run_histogram(pixel)
    assert ae.run_lengths(pixel)[0] == 36 and hist[64] == 15 and int((keys % ae.KEYS_RPP == 0).sum()) == 16
    # a stride of 2^25 under rays_per_pixel = 3 * 2^28: runs of 24, and the offset row * stride passes 2^32 inside the run of pixel 5
    t = np.arange(ae.WIDE_KEYS_ROWS, dtype=np.int64) * ae.WIDE_KEYS_STRIDE
    pixel = t // ae.WIDE_KEYS_RPP
    assert ae.run_histogram(pixel) == {24: 12} and ae.WIDE_KEYS_RPP < 1 << 31
    cross = int(np.flatnonzero(t >= 1 << 32)[0])
    assert pixel[cross] == pixel[cross - 1] == 5 and int((t % ae.WIDE_KEYS_RPP == 0).sum()) == 12


# ---- 3. values at the edges of to_fixed
def test_extreme_frame_holds_the_clamped_the_dropped_and_the_emitted(oracle, bunny_full_bsdf):
    arrays = ae.extreme_arrays(bunny_full_bsdf)
    albedo = arrays.materials["albedo"]
    for v in ae.EXTREME_VALUES:  # the three materials of the walls and the light hold every value
        held = np.isnan(albedo[:3]).any() if np.isnan(v) else (albedo[:3] == np.float32(v)).any()
        assert held, v
    assert (np.isnan(arrays.lights["L"][:, 2])).all() and (arrays.lights["L"][:, 1] == -np.inf).all()
    w, h, spp = ae.EXTREME_FRAME
    for watertight in (False, True):
        osc = oracle.scene(arrays).set_watertight(watertight)
        sums, ids, (tri, mat, vals, pixel, keys) = ae.frame_expected(oracle, osc, default_camera(oracle, w / h), w, h, spp)
        osc.close()
        assert np.array_equal(ae.exact_sums(tri, vals, pixel, w * h), sums)  # (asserts that nothing leaves int64)
        feat = sums[:, :ae.DEPTH]
        for v in (1 << 62, -(1 << 62), 1 << 61, -(1 << 61), -(1 << 30), 2, 1):  # 2 = two samples of 1.5 * 2^-31, rounded to 1 each
            print("entries equal to", v, int((feat == v).sum()))
            assert (feat == v).any(), v
        hit = tri >= 0
        fx = ae.to_fixed(vals[hit])
        with np.errstate(invalid="ignore"):
            gone = np.isnan(vals[hit]) | (vals[hit] == np.float32(1e-10))
        assert gone[:, :3].any() and gone[:, ae.EMISSION + 2].any() and (fx[gone] == 0).all()
        # a pixel whose samples all land on a material with such a channel keeps a zero there although it is hit
        al = vals[:, ae.ALBEDO:ae.ALBEDO + 3]
        with np.errstate(invalid="ignore"):
            dropped = np.isnan(al) | (al == np.float32(1e-10)) | ~hit[:, None]
        all_dropped = dropped.reshape(w * h, spp, 3).all(axis=1) & (sums[:, ae.HITS] == spp)[:, None]
        assert all_dropped.any() and (sums[:, :3][all_dropped] == 0).all()
        lit = sums[:, ae.EMISSION] != 0
        assert lit.any() and (sums[lit, ae.EMISSION] > 0).all() and (sums[lit, ae.EMISSION + 1] < 0).all() and (sums[:, ae.EMISSION + 2] == 0).all()


# ---- 4. sums at the edges of the resolve
def test_synthetic_sums_reach_the_edges_of_the_resolve():
    for n_pixels in ae.RESOLVE_PIXELS:
        sums = ae.synthetic_sums(n_pixels)
        assert sums.shape == (n_pixels, ae.CHANNELS) and sums.dtype == np.int64
        assert np.array_equal(sums, ae.synthetic_sums(n_pixels))  # seeded
        assert int(np.abs(sums).max()) <= 1 << 62
        if n_pixels >= 23:
            assert set(sums[:, ae.HITS].tolist()) == set(ae.RESOLVE_HITS)
            vals = set(sums[:, :ae.HITS].ravel().tolist())
            assert all(v in vals and -v in vals for v in ae.RESOLVE_LITERALS)
            assert (sums[:, :ae.HITS] < 0).any() and (np.abs(sums[:, :ae.HITS]) > 1 << 53).any()
        for spp in ae.RESOLVE_SAMPLES:
            out = ae.resolve(sums, spp)
            assert out.dtype == np.float32 and np.isfinite(out).all()
            assert (out[sums[:, ae.HITS] <= 0, ae.DEPTH] == 0).all()
    # the block edges the pixel counts are chosen for: 23 and 24 pixels are 253 and 264 values around one block of 256 threads
    assert 23 * ae.CHANNELS < 256 < 24 * ae.CHANNELS
    # float32(hits) above 2^24 rounds, the sum above 2^53 rounds twice (to double, then to float): the restatement does both
    sums = np.zeros((2, ae.CHANNELS), np.int64)
    sums[0] = [(1 << 53) + 1] * 9 + [1 << 61, (1 << 24) + 1]
    sums[1] = [-(1 << 53) - 1] * 9 + [-(1 << 61), -1]
    out = ae.resolve(sums, 1)
    assert out[0].tolist() == [float(1 << 23)] * 9 + [float(1 << 31) / float(1 << 24), float(1 << 24)]
    assert out[1].tolist() == [-float(1 << 23)] * 9 + [0.0, -1.0]
    assert ae.resolve(sums, (1 << 31) - 1)[0, 0] == np.float32(2.0 ** 23) * (np.float32(1) / np.float32(2.0 ** 31))
