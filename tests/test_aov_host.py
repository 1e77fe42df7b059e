"""CPU tests of the first-hit feature buffers (rt_render_aov_fixed / rt_render_aov_rays_fixed_device / rt_aov_resolve): the
helper the GPU tests compare with (tests/aov_expected.py) is held to the oracle -- its watertight emission channels to the
oracle's own per-sample frame at max_bounces = 0 on every pixel, its hits to exhaustive search -- and the entry points are
declared / exported / bound / built.  Everything that renders is in tests/test_gpu_aov.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, default_camera, oracle_scene, usable_cpus
import aov_expected as ae
import raytable_keyed as rk

NEW = ("rt_render_aov_fixed", "rt_render_aov_rays_fixed_device", "rt_aov_resolve")


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


@pytest.mark.parametrize("w,h,spp", [(64, 48, 4), (19, 27, 3)])
def test_helper_emission_and_hits_are_the_oracles_per_sample_frame(oracle, w, h, spp):
    osc = oracle_scene(oracle, "full_bsdf", True)
    cam = default_camera(oracle, w / h)
    sums, ids, (tri, mat, vals, pixel, keys) = ae.frame_expected(oracle, osc, cam, w, h, spp)
    want = np.zeros((h, w, 3), np.int64)
    _, _, st = osc.render(cam, w, h, spp, max_bounces=0, threads=usable_cpus(), fixed_out=want, rng_mode="per_sample")
    assert st["sum_gen"] == w * h * spp
    assert np.array_equal(sums[:, ae.EMISSION:ae.EMISSION + 3], want.reshape(-1, 3))
    assert int(want.sum()) > 0
    # every emission deposit of the oracle's frame is a sample that hit a light triangle
    on_light = np.asarray(osc.arrays.tri_light)[tri[tri >= 0]] >= 0
    assert st["emission_adds"] == int(on_light.sum()) > 0
    # hits, ties included, are exhaustive search's on those rays
    o, d, _ = rk.keyed_pinhole_table(oracle, cam, w, h, spp, 1, range(w * h * spp))
    b_tri, b_t, _, _ = osc.trace_closest_brute(o, d, np.full(len(o), ae.FLT_MAX, np.float32))
    assert np.array_equal(tri, b_tri)
    hit = tri >= 0
    assert np.array_equal(vals[hit, ae.DEPTH].view(np.uint32), b_t[hit].view(np.uint32))
    assert np.array_equal(sums[:, ae.HITS], np.bincount(pixel[hit], minlength=w * h))
    # the ids are those of sample spp * p
    assert np.array_equal(ids[:, 0], tri[::spp]) and np.array_equal(ids[:, 1], mat[::spp])


def test_shards_of_the_helper_add_up_and_ids_are_shard_zeros(oracle):
    w, h, spp = 19, 27, 4
    osc = oracle_scene(oracle, "full_bsdf", True)
    cam = default_camera(oracle, w / h)
    full, ids, _ = ae.frame_expected(oracle, osc, cam, w, h, spp)
    for R in (2, 4):
        parts = [ae.frame_expected(oracle, osc, cam, w, h, spp, shard=(r, R)) for r in range(R)]
        assert np.array_equal(sum(p[0] for p in parts), full)
        assert np.array_equal(parts[0][1], ids)
        assert all((p[1] == -7).all() for p in parts[1:])


def test_wide_view_holds_misses_hits_emission_and_specular_hits(oracle):
    w, h, spp = ae.WIDE_FRAME
    for watertight in (False, True):
        osc = oracle_scene(oracle, "full_bsdf", watertight)
        sums, _, (tri, mat, _, _, _) = ae.frame_expected(oracle, osc, ae.wide_camera(oracle.camera, w / h), w, h, spp)
        ae.assert_wide_content(osc.arrays, tri, mat, sums)


def test_to_fixed_and_resolve_restatements():
    x = np.array([0.0, 1.0, -1.0, 0.73, 2.0 ** -31, 3.0 * 2.0 ** -31, -3.0 * 2.0 ** -31, 5.0 * 2.0 ** -31, 3e9, -3e9, np.inf, np.nan], np.float32)
    want = [0, 1 << 30, -(1 << 30), int(np.float32(0.73) * 2.0 ** 30), 0, 2, -2, 2, 1 << 61, -(1 << 61), 1 << 61, 0]
    assert ae.to_fixed(x).tolist() == want
    sums = np.zeros((3, ae.CHANNELS), np.int64)
    sums[1] = [1 << 30] * 10 + [1]
    sums[2] = [3 << 29] * 9 + [5 << 30, 2]
    out = ae.resolve(sums, 4)
    assert out.dtype == np.float32 and (out[0] == 0).all()
    assert out[1].tolist() == [0.25] * 9 + [1.0, 0.25]
    assert out[2].tolist() == [0.375] * 9 + [2.5, 0.5]


def test_new_entry_points_are_declared_exported_and_bound(api):
    header = open(os.path.join(ROOT, "include", "rtcuda_amd.h")).read()
    for name in NEW:
        assert name in api.EXPORTS
        assert f"int {name}(" in header
        assert getattr(api.lib(), name).argtypes is not None
    assert "#define RT_AOV_CHANNELS 11" in header and api.AOV_CHANNELS == ae.CHANNELS == 11
    assert (api.AOV_ALBEDO, api.AOV_NORMAL, api.AOV_EMISSION, api.AOV_DEPTH, api.AOV_HITS) == (0, 3, 6, 9, 10)
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bT {name}$", syms, re.M), name
    for name in ("render_aov", "render_aov_rays"):
        assert callable(getattr(api.Scene, name))
    assert callable(api.aov_resolve)


def test_symbol_table_has_the_ten_builds_of_k_aov(api):
    """k_aov<SRC, WIDE, LITERAL, VERIFY>: per ray source the 4-wide and the 2-wide walk with and without the reference's
    decisions, and the literal walk."""
    syms = subprocess.run(["nm", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for src in ("9AovCamera", "13KeyedRayTable"):
        for wide, literal, verify in ((1, 0, 1), (0, 0, 1), (1, 0, 0), (0, 0, 0), (0, 1, 0)):
            assert f" _Z5k_aovI{src}Lb{wide}ELb{literal}ELb{verify}EE" in syms, (src, wide, literal, verify)


def test_host_side_argument_errors_name_the_entry_point_and_write_nothing(api):
    """What the library refuses before it needs a device: the null scene comes first."""
    L = api.lib()
    rays = np.zeros(6, np.float32)
    cam = np.zeros(12, np.float32)
    out = np.full(ae.CHANNELS, 7, np.int64)
    ids = np.full(2, 7, np.int32)
    p = rays.ctypes.data
    assert L.rt_render_aov_fixed(None, cam.ctypes.data, 1, 1, 1, 1, 0, 1, 0, out.ctypes.data, ids.ctypes.data, None, None) != 0
    msg = L.rt_last_error().decode()
    assert msg.startswith("rt_render_aov_fixed: ") and "null scene" in msg, msg
    assert L.rt_render_aov_rays_fixed_device(None, 1, p, p, None, 1, 1, 0, 1, 0, out.ctypes.data, ids.ctypes.data, None, None) != 0
    msg = L.rt_last_error().decode()
    assert msg.startswith("rt_render_aov_rays_fixed_device: ") and "null scene" in msg, msg
    assert L.rt_aov_resolve(None, out.ctypes.data, 1, 1, None) != 0
    assert L.rt_last_error().decode().startswith("rt_aov_resolve: null d_aov_fixed")
    assert L.rt_aov_resolve(out.ctypes.data, out.ctypes.data, 1, 0, None) != 0
    assert L.rt_last_error().decode().startswith("rt_aov_resolve: ")
    assert (out == 7).all() and (ids == 7).all()


class _Scene:
    """A Scene without a device scene: the wrapper's checks run before the library is reached."""

    def __new__(cls, api):
        s = api.Scene.__new__(api.Scene)
        s.L, s.h = api.lib(), None
        return s


def test_wrappers_reject_bad_tensors_before_reaching_the_library(api):
    torch = pytest.importorskip("torch")

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    def gpu(x):
        return x.as_subclass(OnGpu)

    sc = _Scene(api)
    o, d = gpu(torch.zeros(8, 3)), gpu(torch.zeros(8, 3))
    cam = np.zeros(12, np.float32)
    cases = [
        ("render_aov_rays: origins must be on the scene's GPU", lambda: sc.render_aov_rays(torch.zeros(8, 3), torch.zeros(8, 3), 8)),
        ("dirs must be torch.float32", lambda: sc.render_aov_rays(o, gpu(torch.zeros(8, 3, dtype=torch.float64)), 8)),
        (r"dirs must have shape \(n, 3\)", lambda: sc.render_aov_rays(o, gpu(torch.zeros(7, 3)), 8)),
        ("pixel must be torch.int32", lambda: sc.render_aov_rays(o, d, 8, pixel=gpu(torch.zeros(8, dtype=torch.int64)))),
        ("n_pixels must be a positive int", lambda: sc.render_aov_rays(o, d, 0)),
        ("ids together with a pixel tensor", lambda: sc.render_aov_rays(o, d, 8, pixel=gpu(torch.zeros(8, dtype=torch.int32)), ids=True)),
        ("out must be a torch tensor on the scene's GPU", lambda: sc.render_aov_rays(o, d, 8, out=torch.zeros(8, 11, dtype=torch.int64))),
        (r"out must be a contiguous \(8, 11\) torch.int64", lambda: sc.render_aov_rays(o, d, 8, out=gpu(torch.zeros(8, 3, dtype=torch.int64)))),
        ("key_first must be an int in 0 .. 2\\^64 - 1", lambda: sc.render_aov_rays(o, d, 8, key_first=2 ** 64)),
        ("key_stride must be an int in 0 .. 2\\^32 - 1", lambda: sc.render_aov_rays(o, d, 8, key_stride=2 ** 32)),
        ("render_aov: spp must be a positive int", lambda: sc.render_aov(cam, 4, 4, 0)),
        ("render_aov: seed must be an int", lambda: sc.render_aov(cam, 4, 4, 1, seed=-1)),
        ("render_aov: camera must be the 12 floats", lambda: sc.render_aov(cam[:9], 4, 4, 1)),
        ("aov_resolve: sums must be a torch tensor on a GPU", lambda: api.aov_resolve(torch.zeros(8, 11, dtype=torch.int64), 1)),
        (r"aov_resolve: sums must be a contiguous \(n_pixels, 11\)", lambda: api.aov_resolve(gpu(torch.zeros(8, 3, dtype=torch.int64)), 1)),
        ("aov_resolve: spp must be a positive int", lambda: api.aov_resolve(gpu(torch.zeros(8, 11, dtype=torch.int64)), 0)),
    ]
    for pattern, call in cases:
        with pytest.raises(api.RtError, match=pattern):
            call()


def test_cpp_wrappers_link_and_throw_the_library_message():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "aovcheck"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "aov_api_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(l.split("=", 1) for l in out.stdout.splitlines())
    assert lines["render_aov"] == "render_aov: rt_render_aov_fixed: null scene"
    assert lines["render_aov_rays"] == "render_aov_rays: rt_render_aov_rays_fixed_device: null scene"
    assert lines["aov_resolve"] == "aov_resolve: rt_aov_resolve: null d_out"
    assert lines["out"] == "7 7 7 7"


def test_recorded_resources_and_timings_are_committed():
    """profiles/aov_resources.md: the eleven new kernels, none with a spill or scratch; profiles/aov_time.json: the frame the
    issue names, both flag values, the route of before on another build, and the two variant builds."""
    import json
    rows = [l for l in open(os.path.join(ROOT, "profiles", "aov_resources.md")) if l.startswith("| `k_aov")]
    assert len(rows) == 11
    for r in rows:
        c = [x.strip() for x in r.strip().strip("|").split("|")]
        assert (c[3], c[4]) == ("0", "0") and int(c[5]) >= 4, r
    t = json.load(open(os.path.join(ROOT, "profiles", "aov_time.json")))
    assert t["frame"] == [1920, 1080, 16] and t["reps"] == 7
    for k in ("flags_0", "watertight"):
        assert t["aov"][k]["kernel"]["ms"] > 0 and t["today"][k]["route"]["ms"] > 0
        assert t["no_deposit"][k]["kernel"]["ms"] < t["aov"][k]["kernel"]["ms"] < t["per_lane_atomics"][k]["kernel"]["ms"]
        assert 0 < t[f"deposit_share_{k}"] < 1
    assert len({t["aov"]["build_id"], t["today"]["build_id"], t["no_deposit"]["build_id"], t["per_lane_atomics"]["build_id"]}) == 4
