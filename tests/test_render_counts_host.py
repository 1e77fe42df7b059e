"""CPU tests of the counted frames (rt_render_counts_fixed, rt_normalize_counts_fixed, rt_post_process_counts_fixed,
rt_sample_allocate): the helper the GPU tests compare with (tests/render_counts_expected.py) is held to the oracle -- its two
routes to a counted frame's sums agree, and a whole frame of counts is the oracle's per-sample frame --, the Python-integer twins
of the normaliser and the allocator are checked on their own, and the entry points are declared / exported / bound / built and
refuse what they can refuse without a device.  Everything that renders is in tests/test_gpu_render_counts.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, default_camera, oracle_scene, usable_cpus
import render_counts_expected as rc

NEW = ("rt_render_counts_fixed", "rt_normalize_counts_fixed", "rt_post_process_counts_fixed", "rt_sample_allocate")


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


# ---- the helper against the oracle
def test_the_two_routes_agree_on_a_random_map(oracle):
    w, h, S = 9, 7, 8
    osc = oracle_scene(oracle, "full_bsdf", True)
    rng = np.random.default_rng(3)
    count = rng.integers(0, S + 1, w * h)
    first = (rng.random(w * h) * (S - count + 1)).astype(np.int64)
    assert (count == 0).any() and (count == S).any() and (first > 0).any()
    by_frames = rc.expected_by_frames(oracle, osc, "full_bsdf", w, h, S, first, count)
    by_tables, ev = rc.expected_by_tables(oracle, osc, w, h, S, first, count)
    assert np.array_equal(by_frames, by_tables) and by_frames.any()
    assert ev["camera_rays"] == int(count.sum()) and ev["shade_events"] > 0


def test_a_whole_frame_of_counts_is_the_oracles_per_sample_frame(oracle):
    w, h, S = 9, 7, 8
    osc = oracle_scene(oracle, "full_bsdf", True)
    want = np.zeros((h, w, 3), np.int64)
    _, _, st = osc.render(default_camera(oracle, w / h), w, h, S, threads=usable_cpus(), fixed_out=want, rng_mode="per_sample")
    count = np.full(w * h, S)
    assert np.array_equal(rc.expected_by_frames(oracle, osc, "full_bsdf", w, h, S, None, count), want.reshape(-1, 3))
    by_tables, ev = rc.expected_by_tables(oracle, osc, w, h, S, None, count)
    assert np.array_equal(by_tables, want.reshape(-1, 3)) and ev == rc.events_of(st)


# ---- the twins
def test_normalize_twin():
    sums = np.array([[10, -10, 0], [7, -7, 1], [5, 5, 5], [9, -9, 3], [-(2 ** 62), 2 ** 62, 1]], np.int64)
    samples = np.array([1, 2, 0, 3, 4], np.int32)
    got = rc.normalize_twin(sums, samples)
    assert got.tolist() == [[10, -10, 0], [4, -4, 1], [0, 0, 0], [3, -3, 1], [-(2 ** 60), 2 ** 60, 0]]
    with pytest.raises(ValueError):
        rc.normalize_twin(sums, np.array([1, 1, -1, 1, 1], np.int32))
    pp = rc.post_process_twin(np.array([[1 << 30, 4 << 30, 0], [1 << 30, 1, 2]], np.int64), np.array([4, 0], np.int32))
    assert pp.dtype == np.float32 and pp.tolist() == [[0.5, 1.0, 0.0], [0.0, 0.0, 0.0]]


def test_allocate_twin():
    rng = np.random.default_rng(11)
    w = rng.random(1000).astype(np.float32)
    w[::7] = np.nan
    w[3::7] = -1.0
    w[5] = np.inf
    w[9] = 5000.0
    for lo, hi, budget in ((0, 64, 8000), (1, 4, 8000), (2, 2, 2000), (0, 1 << 30, (1 << 31) - 1)):
        counts, total = rc.allocate_twin(w, lo, hi, budget)
        assert total == int(counts.astype(np.int64).sum()) <= budget and counts.min() >= lo and counts.max() <= hi
        assert (counts[::7] == lo).all() and (counts[3::7] == lo).all()  # NaN and negative weights get min_count
    assert rc.quantised_weight(np.array([np.inf, 5000.0, 4096.0, 2.0 ** -20, 2.0 ** -21, 0.0, -0.0], np.float32)) == [1 << 32, 1 << 32, 1 << 32, 1, 0, 0, 0]
    counts, total = rc.allocate_twin(np.zeros(10, np.float32), 1, 9, 35)  # T = 0: the even split
    assert counts.tolist() == [3] * 10 and total == 30
    counts, total = rc.allocate_twin(np.array([1, 3], np.float32), 0, 100, 8)
    assert counts.tolist() == [2, 6] and total == 8
    for bad in ((-1, 4, 100), (3, 2, 100), (2, 4, 19), (0, 4, 1 << 31)):
        with pytest.raises(ValueError):
            rc.allocate_twin(np.ones(10, np.float32), *bad)


# ---- the library, without a device
def test_new_entry_points_are_declared_exported_and_bound(api):
    header = open(os.path.join(ROOT, "include", "rtcuda_amd.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in api.EXPORTS
        assert re.search(rf"^int {name}\(", header, re.M)
        assert getattr(api.lib(), name).argtypes is not None
        assert re.search(rf"\bT {name}$", syms, re.M), name
    assert callable(api.Scene.render_counts)
    for name in ("normalize_counts", "post_process_counts", "sample_allocate"):
        assert callable(getattr(api, name))


def test_symbol_table_has_the_four_builds_of_k_paths_counts(api):
    syms = subprocess.run(["nm", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for lds in (0, 1):
        for waves, draw in ((4, 1), (2, 0)):
            assert f" _Z7k_pathsI11PathsCountsLb{lds}ELb1ELi{waves}ELb{draw}ELb0ELb0EE" in syms, (lds, waves, draw)
    for name in ("k_counts_sums", "k_counts_scan", "k_counts_offsets", "k_normalize_counts", "k_post_process_counts", "k_allocate_total", "k_allocate_counts"):
        assert re.search(rf" _Z\d+{name}", syms), name


def test_what_is_refused_before_a_device_is_needed(api):
    L = api.lib()
    sums = (ctypes.c_int64 * 3)(7, 7, 7)
    n32 = (ctypes.c_int32 * 1)(7)
    cam = (ctypes.c_float * 12)()
    wgt = (ctypes.c_float * 1)(1.0)
    total = ctypes.c_int64(7)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)

    def refused(rc_, message):
        assert rc_ != 0 and L.rt_last_error().decode() == message, L.rt_last_error().decode()

    refused(L.rt_render_counts_fixed(None, p(cam), 1, 1, 1, None, p(n32), 10, 1, 0, p(sums), p(n32), None, None), "rt_render_counts_fixed: null scene")
    refused(L.rt_normalize_counts_fixed(None, p(n32), 1, p(sums), None), "rt_normalize_counts_fixed: null d_sum_fixed")
    refused(L.rt_normalize_counts_fixed(p(sums), None, 1, p(sums), None), "rt_normalize_counts_fixed: null d_samples")
    refused(L.rt_normalize_counts_fixed(p(sums), p(n32), 0, p(sums), None), "rt_normalize_counts_fixed: num_pixels must be at least 1")
    refused(L.rt_post_process_counts_fixed(p(sums), p(n32), 1, None, None), "rt_post_process_counts_fixed: null d_rgb_out")
    refused(L.rt_sample_allocate(None, 1, 0, 1, 1, p(n32), ctypes.byref(total), None), "rt_sample_allocate: null d_weight")
    refused(L.rt_sample_allocate(p(wgt), 1, -1, 1, 1, p(n32), ctypes.byref(total), None), "rt_sample_allocate: min_count = -1 is negative")
    refused(L.rt_sample_allocate(p(wgt), 1, 3, 2, 8, p(n32), ctypes.byref(total), None), "rt_sample_allocate: max_count = 2 is below min_count = 3")
    refused(L.rt_sample_allocate(p(wgt), 1, 2, 4, 1, p(n32), ctypes.byref(total), None),
            "rt_sample_allocate: budget = 1 is below num_pixels * min_count = 2")
    refused(L.rt_sample_allocate(p(wgt), 1, 0, 4, 1 << 31, p(n32), ctypes.byref(total), None),
            "rt_sample_allocate: budget - num_pixels * min_count = 2147483648 exceeds 2147483647")
    assert list(sums) == [7, 7, 7] and n32[0] == 7 and total.value == 7


def test_python_wrappers_refuse_bad_arguments(api):
    with pytest.raises(api.RtError, match="sample_allocate: weight must be a torch tensor on a GPU"):
        api.sample_allocate(np.ones(4, np.float32), 0, 4, 8)
    with pytest.raises(api.RtError, match="normalize_counts: sums must be a torch tensor on a GPU"):
        api.normalize_counts(np.zeros((4, 3), np.int64), np.ones(4, np.int32))
    with pytest.raises(api.RtError, match="post_process_counts: sums must be a torch tensor on a GPU"):
        api.post_process_counts(np.zeros((4, 3), np.int64), np.ones(4, np.int32))


def test_cpp_wrappers_link_and_throw_the_library_message():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "countscheck"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "render_counts_api_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "render_counts=render_counts: rt_render_counts_fixed: null scene" in lines
    assert "normalize_counts=normalize_counts: rt_normalize_counts_fixed: null d_samples" in lines
    assert "post_process_counts=post_process_counts: rt_post_process_counts_fixed: null d_rgb_out" in lines
    assert "sample_allocate=sample_allocate: rt_sample_allocate: budget = 1 is below num_pixels * min_count = 2" in lines
    assert "sample_allocate=sample_allocate: rt_sample_allocate: max_count = 2 is below min_count = 3" in lines
    assert lines[-1] == "out=7 7 1 7"
