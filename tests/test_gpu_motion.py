"""GPU tests of the motion buffer (rt_render_motion).  Run with -m gpu.

What a frame must hold comes from tests/temporal_expected.py: numpy float32 on the hits of OracleScene.trace_closest along the
oracle's pixel-centre rays (held to the CPU twin by tests/test_temporal_host.py).  Every comparison is EQUALITY of the bits of
all four floats of every record."""
import numpy as np
import pytest

from conftest import default_camera, oracle_scene
import aov_expected as ae
import temporal_expected as te

pytestmark = pytest.mark.gpu

POISON = -7.0
MOVED_VIEW = dict(lookfrom=(0.56, 0.52, 1.46), lookat=(0.5, 0.5, 0.0), up=(0.0, 1.0, 0.0), vfov=37.8)
# a previous camera inside the box, looking at the left wall: the back wall and the right half of the box lie behind its pinhole
BEHIND_VIEW = dict(lookfrom=(0.6, 0.5, -0.5), lookat=(0.0, 0.5, -0.5), up=(0.0, 1.0, 0.0), vfov=60.0)
DELTA = (0.03, 0.0, -0.02)


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
    return [("default", 0, False), ("reference-walk", api.FLAG_REFERENCE_WALK, False), ("watertight", api.FLAG_WATERTIGHT, True)]


def _view(make_camera, v, aspect):
    return make_camera(v["lookfrom"], v["lookat"], v["up"], v["vfov"], aspect)


def _cam(make_camera, which, aspect):
    if which == "default":
        return make_camera((0.5, 0.5, 1.5), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8, aspect)
    if which == "wide":
        return ae.wide_camera(make_camera, aspect)
    return _view(make_camera, MOVED_VIEW if which == "moved" else BEHIND_VIEW, aspect)


_expected = {}


def _want(oracle, w, h, cam, prev, watertight):
    """The restatement's records on full_bsdf (vertices did not move), once per session and argument tuple, never modified."""
    key = (w, h, cam, prev, watertight)
    if key not in _expected:
        osc = oracle_scene(oracle, "full_bsdf", watertight)
        rec, tri = te.motion_expected(oracle, osc, _cam(oracle.camera, cam, w / h), w, h, _cam(oracle.camera, prev, w / h))
        rec.setflags(write=False)
        _expected[key] = (rec, tri)
    return _expected[key]


def _assert_records(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    bad = te.bits(got) != te.bits(want)
    print(what, "record words that differ:", int(bad.sum()), "of", bad.size)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[bad][:6].tolist(), want[bad][:6].tolist())


def _poisoned(torch, n):
    return torch.full((n, 4), POISON, dtype=torch.float32, device="cuda")


FRAMES = [(1, 1, "default"), (1, 63, "default"), (1, 65, "default"), (19, 27, "default"), (64, 48, "default"), ae.WIDE_FRAME[:2] + ("wide",)]


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["default", "reference-walk", "watertight"])
@pytest.mark.parametrize("w,h,cam", FRAMES, ids=["%dx%d-%s" % f for f in FRAMES])
def test_same_camera_and_vertices(api, torch, oracle, w, h, cam, mode):
    """NULL previous vertices, the previous camera the current one: the records of the scene's own stored triangles; the poisoned
    output is fully overwritten; stats are filled as rt_render_aov_fixed fills them."""
    name, flags, watertight = _modes(api)[mode]
    want, tri = _want(oracle, w, h, cam, cam, watertight)
    if cam == "wide":
        assert 0.05 <= float(np.mean(tri < 0)) <= 0.95
    c = _cam(api.make_camera, cam, w / h)
    out, st = _gpu(api).render_motion(c, w, h, c, flags=flags, out=_poisoned(torch, w * h))
    _assert_records(out, want, (name, w, h, cam))
    assert st["camera_rays"] == st["closest_rays"] == w * h and st["seconds_render"] > 0
    if w * h >= 64 * 48:  # every hit lands on its own pixel centre, to a hundredth of a pixel
        g = out.cpu().numpy()
        hit = tri >= 0
        assert np.abs(g[hit, 0] - (np.arange(w * h) % w + 0.5)[hit]).max() < 0.01


def test_time_kernels_flag_changes_nothing(api, torch, oracle):
    w, h = 19, 27
    want, _ = _want(oracle, w, h, "default", "default", True)
    c = _cam(api.make_camera, "default", w / h)
    out, _ = _gpu(api).render_motion(c, w, h, c, flags=api.FLAG_WATERTIGHT | api.FLAG_TIME_KERNELS)
    _assert_records(out, want)


@pytest.mark.parametrize("prev", ["moved", "behind"])
def test_a_moved_previous_camera(api, torch, oracle, prev):
    w, h = 64, 48
    for name, flags, watertight in _modes(api)[::2]:
        want, tri = _want(oracle, w, h, "default", prev, watertight)
        if prev == "behind":  # part of the frame projects behind the previous pinhole, part in front of it
            behind = (tri >= 0) & (want[:, 0] == -1) & (want[:, 1] == -1)
            assert 0.1 < behind.mean() < 0.9 and ((tri >= 0) & ~behind).mean() > 0.1, behind.mean()
        out, _ = _gpu(api).render_motion(_cam(api.make_camera, "default", w / h), w, h, _cam(api.make_camera, prev, w / h), flags=flags,
                                         out=_poisoned(torch, w * h))
        _assert_records(out, want, (name, prev))


def test_moved_vertices_and_two_calls_and_a_side_stream(api, torch, oracle):
    """Scene.update to new positions, the old ones passed as previous, under a moved previous camera; then the same call again
    on a side stream into the same buffer; the triangle ids are query_closest's for the same rays."""
    from rtcuda_amd import scenes
    w, h = 64, 48
    old = scenes.cornell_bunny("full_bsdf")
    new = te.moved_arrays(old, DELTA)
    gpu = api.Scene(old)
    gpu.update(new.tris)
    osc = oracle.scene(new).set_watertight(True)
    cur, prev = _cam(oracle.camera, "default", w / h), _cam(oracle.camera, "moved", w / h)
    want, tri = te.motion_expected(oracle, osc, cur, w, h, prev, prev_tris=old.tris)
    still, _ = te.motion_expected(oracle, osc, cur, w, h, prev)
    assert (te.bits(want) != te.bits(still)).any()  # (the previous vertices matter)
    prev_dev = torch.from_numpy(np.ascontiguousarray(old.tris, np.float32).reshape(-1, 9)).cuda()
    out, _ = gpu.render_motion(cur, w, h, prev, prev_tris=prev_dev, flags=api.FLAG_WATERTIGHT, out=_poisoned(torch, w * h))
    _assert_records(out, want, "moved vertices")
    out2, _ = gpu.render_motion(cur, w, h, prev, flags=api.FLAG_WATERTIGHT)
    _assert_records(out2, still, "current vertices, second call")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out.fill_(POISON)
        gpu.render_motion(cur, w, h, prev, prev_tris=prev_dev.reshape(-1, 3, 3), flags=api.FLAG_WATERTIGHT, out=out, stream=side)
    side.synchronize()
    _assert_records(out, want, "side stream")
    o, d = te.centre_rays(oracle, cur, w, h)
    hit, _, _, _ = gpu.query_closest(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), flags=api.FLAG_WATERTIGHT)
    assert np.array_equal(te.tri_ids(out.cpu().numpy()), hit.cpu().numpy())
    assert np.array_equal(hit.cpu().numpy(), tri)
    gpu.close()
    osc.close()


def test_two_wide_scene_and_device_built_scene(api, torch, oracle, monkeypatch):
    """Both tree widths are served, previous vertices included (they are read by the caller's index)."""
    from rtcuda_amd import scenes
    w, h = 19, 27
    arrays = scenes.cornell_bunny("full_bsdf")
    want, _ = _want(oracle, w, h, "default", "moved", True)
    cur, prev = _cam(api.make_camera, "default", w / h), _cam(api.make_camera, "moved", w / h)
    prev_dev = torch.from_numpy(np.ascontiguousarray(arrays.tris, np.float32).reshape(-1, 9)).cuda()
    monkeypatch.setenv("RT_BVH_WIDE", "0")
    narrow = api.Scene(arrays)
    monkeypatch.delenv("RT_BVH_WIDE")
    for kw in (dict(), dict(prev_tris=prev_dev)):
        out, _ = narrow.render_motion(cur, w, h, prev, flags=api.FLAG_WATERTIGHT, **kw)
        _assert_records(out, want, ("2-wide", sorted(kw)))
    narrow.close()
    built = api.Scene(arrays, device_bvh=True)
    out, _ = built.render_motion(cur, w, h, prev, flags=api.FLAG_WATERTIGHT)
    _assert_records(out, want, "device-built")
    built.close()


def test_argument_errors_write_nothing(api, torch):
    gpu = _gpu(api)
    w, h = 8, 4
    cam = api.make_camera(aspect=2.0)
    out = _poisoned(torch, w * h)
    import ctypes
    L, c = api.lib(), ctypes.c_void_p
    p = cam.ctypes.data

    def call(scene=gpu.h, cur=p, ww=w, hh=h, prev=p, flags=0, o=out.data_ptr()):
        rc = L.rt_render_motion(scene, cur, ww, hh, prev, None, flags, c(o), None, None)
        return rc, L.rt_last_error().decode()

    for over, text in ((dict(cur=None), "null camera"), (dict(prev=None), "null prev_camera"), (dict(o=None), "null d_motion"), (dict(ww=0), "width and height"),
                       (dict(hh=-1), "width and height"), (dict(ww=1 << 20, hh=1 << 10), "715827882 pixels"),
                       (dict(flags=api.FLAG_WATERTIGHT | api.FLAG_REFERENCE_WALK), "RT_FLAG"), (dict(flags=api.FLAG_RNG_PER_SAMPLE), "flags other than"),
                       (dict(flags=64), "flags other than"), (dict(o=out.data_ptr() + 4), "16-byte aligned")):
        rc, msg = call(**over)
        assert rc != 0 and msg.startswith("rt_render_motion: ") and text in msg, (over, msg)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all()
