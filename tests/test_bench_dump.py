"""bench.py --dump-outputs: what the files hold, the 64 MB limit and the fixed sample of a larger frame (no GPU needed)."""
import os

import numpy as np

import bench


def _totals():
    return {k: float(i) * 1e9 + 7 for i, k in enumerate(bench.TOTAL_KEYS)}


def _finite_dump(path, files):
    for f in files:
        arr = np.load(path / f)
        assert arr.dtype in (np.float32, np.float64) and np.isfinite(arr).all(), f
    assert sum(os.path.getsize(path / f) for f in files) <= bench.DUMP_LIMIT_BYTES


def test_dump_writes_the_whole_image_and_the_event_totals(tmp_path):
    img = np.random.default_rng(1).random((36, 64, 3), dtype=np.float32)
    rec = bench.dump_outputs(str(tmp_path), img, _totals())
    assert rec["files"] == ["event_totals.npy", "image.npy", "image_nonfinite.npy"]
    assert rec["event_totals_keys"] == list(bench.TOTAL_KEYS) and rec["nonfinite_values"] == 0
    _finite_dump(tmp_path, rec["files"])
    assert np.array_equal(np.load(tmp_path / "image.npy"), img)
    assert not np.load(tmp_path / "image_nonfinite.npy").any()
    assert np.array_equal(np.load(tmp_path / "event_totals.npy"), [_totals()[k] for k in bench.TOTAL_KEYS])


def test_dump_marks_nonfinite_channels_and_keeps_every_value_finite(tmp_path):
    """A NaN contribution of the reference's estimator reaches its pixel in the default mode: the dump stores 0 there and
    marks the channel in image_nonfinite.npy; every other channel is the framebuffer's value."""
    img = np.random.default_rng(3).random((1080, 1920, 3), dtype=np.float32)  # the headline frame's size
    img[5, 7, :] = np.nan
    img[100, 200, 1] = np.inf
    rec = bench.dump_outputs(str(tmp_path), img, _totals())
    assert rec["files"] == ["event_totals.npy", "image.npy", "image_nonfinite.npy"] and rec["nonfinite_values"] == 4
    _finite_dump(tmp_path, rec["files"])
    got, mask = np.load(tmp_path / "image.npy"), np.load(tmp_path / "image_nonfinite.npy")
    bad = ~np.isfinite(img)
    assert np.array_equal(mask, bad.astype(np.float32))
    assert np.array_equal(got[~bad], img[~bad]) and not got[bad].any()


def test_dump_of_a_frame_over_the_limit_is_a_fixed_sample_under_it(tmp_path):
    img = np.random.default_rng(2).random((2160, 3840, 3), dtype=np.float32)  # 99.5 MB
    img[0, ::97, 2] = np.nan
    for d in ("a", "b"):
        rec = bench.dump_outputs(str(tmp_path / d), img, _totals())
        assert rec["files"] == ["event_totals.npy", "image_sample.npy", "image_sample_nonfinite.npy", "image_sample_pixels.npy"]
        _finite_dump(tmp_path / d, rec["files"])
    idx = np.load(tmp_path / "a" / "image_sample_pixels.npy")
    assert np.array_equal(idx, np.load(tmp_path / "b" / "image_sample_pixels.npy"))
    want = img.reshape(-1, 3)[idx.astype(np.int64)]
    bad = ~np.isfinite(want)
    assert np.array_equal(np.load(tmp_path / "a" / "image_sample_nonfinite.npy"), bad.astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "image_sample.npy")[~bad], want[~bad])
