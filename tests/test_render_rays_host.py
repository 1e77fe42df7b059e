"""CPU tests of rendering along caller-supplied rays (rt_render_rays_device / rt_render_rays_fixed_device): the fixture
builder of the GPU tests is held to the oracle, the entry points are declared / exported / bound, and what the library and
the wrappers refuse without a device.  Everything that renders is in tests/test_gpu_render_rays.py."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, default_camera, usable_cpus
import raytable

NEW = ("rt_render_rays_device", "rt_render_rays_fixed_device")


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_vectorised_table_is_the_oracle_functions_ray_by_ray(oracle):
    """pinhole_table (numpy, float32) against Oracle.xorwow_draw + Oracle.camera_get_ray, every ray of two small frames."""
    for w, h, spp in ((24, 16, 4), (13, 7, 3)):
        cam = default_camera(oracle, w / h)
        o, d, pixel = raytable.pinhole_table(oracle, cam, w, h, spp)
        o_l, d_l = raytable.pinhole_table_literal(oracle, cam, w, h, spp)
        assert np.array_equal(_bits(o), _bits(o_l)) and np.array_equal(_bits(d), _bits(d_l))
        assert np.array_equal(pixel, np.arange(w * h * spp) // spp)


@pytest.mark.parametrize("w,h,spp,max_bounces", [(256, 256, 4, 10), (256, 256, 16, 0), (64, 36, 8, 10)])
def test_ray_table_is_the_oracles_first_generation(oracle, bunny_matte, w, h, spp, max_bounces):
    """The test's own ray table is the oracle's: the first n closest rays the oracle logs in a render of the same frame are
    iteration 1's camera rays; origins and directions are bit-equal, all n of them (in slot order, or -- if the log is
    ordered otherwise -- matched by sorting both sides on their bits: still every ray)."""
    n = w * h * spp
    cam = default_camera(oracle, w / h)
    o, d, _ = raytable.pinhole_table(oracle, cam, w, h, spp)
    sc = oracle.scene(bunny_matte)
    oracle.raylog_enable(True)
    try:
        sc.render(cam, w, h, spp, max_bounces=max_bounces, threads=usable_cpus())
        log = oracle.raylog_fetch()
    finally:
        oracle.raylog_enable(False)
    lo, ld = log["closest_o"][:n], log["closest_d"][:n]
    assert len(lo) == n
    mine = np.concatenate([_bits(o), _bits(d)], axis=1)
    theirs = np.concatenate([_bits(lo), _bits(ld)], axis=1)
    if not np.array_equal(mine, theirs):
        mine = mine[np.lexsort(mine.T[::-1])]
        theirs = theirs[np.lexsort(theirs.T[::-1])]
    assert np.array_equal(mine, theirs)


def test_degenerate_camera_sends_every_ray_one_way(oracle):
    cam, o, d = raytable.degenerate_camera(oracle, (0.5, 0.5, 1.5), (0.45, 0.3, 0.4))
    for x, y in ((0.0, 0.0), (0.999, 0.001), (0.3, 0.7)):
        r = oracle.camera_get_ray(cam, x, y)
        assert np.array_equal(_bits(r[0:3]), _bits(o)) and np.array_equal(_bits(r[3:6]), _bits(d))


def test_new_entry_points_are_declared_exported_and_bound(api):
    header = open(os.path.join(ROOT, "include", "rtcuda_amd.h")).read()
    for name in NEW:
        assert name in api.EXPORTS
        assert f"int {name}(" in header
        assert getattr(api.lib(), name).argtypes is not None


def test_host_side_argument_errors_name_the_entry_point_and_write_nothing(api):
    """What the library refuses before it needs a device (the null scene comes first; everything else needs a scene and is
    in the GPU file)."""
    L = api.lib()
    rays = np.zeros(6, np.float32)
    out = np.full(3, 7, np.int64)
    p = rays.ctypes.data
    for name in NEW:
        assert getattr(L, name)(None, 1, p, p, None, 1, 1, 10, 1, 0, out.ctypes.data, None, None) != 0
        msg = L.rt_last_error().decode()
        assert name in msg and "null scene" in msg, msg
    assert (out == 7).all()


class _Scene:
    """A Scene without a device scene: the wrapper's checks run before the library is reached."""

    def __new__(cls, api):
        s = api.Scene.__new__(api.Scene)
        s.L, s.h = api.lib(), None
        return s


def test_torch_wrapper_rejects_bad_tensors_before_reaching_the_library(api):
    torch = pytest.importorskip("torch")

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    def gpu(x):
        return x.as_subclass(OnGpu)

    sc = _Scene(api)
    o, d = gpu(torch.zeros(8, 3)), gpu(torch.zeros(8, 3))
    cases = [
        ("render_rays: origins must be on the scene's GPU", lambda: sc.render_rays(torch.zeros(8, 3), torch.zeros(8, 3), 8)),
        ("origins must be a torch tensor", lambda: sc.render_rays(np.zeros((8, 3), np.float32), d, 8)),
        ("dirs must be torch.float32", lambda: sc.render_rays(o, gpu(torch.zeros(8, 3, dtype=torch.float64)), 8)),
        ("origins must be contiguous", lambda: sc.render_rays(gpu(torch.zeros(3, 8).t()), d, 8)),
        (r"origins must have shape \(n, 3\)", lambda: sc.render_rays(gpu(torch.zeros(8, 4)), d, 8)),
        (r"dirs must have shape \(n, 3\)", lambda: sc.render_rays(o, gpu(torch.zeros(7, 3)), 8)),
        ("pixel must be torch.int32", lambda: sc.render_rays(o, d, 8, pixel=gpu(torch.zeros(8, dtype=torch.int64)))),
        (r"pixel must have shape \(n,\)", lambda: sc.render_rays(o, d, 8, pixel=gpu(torch.zeros(9, dtype=torch.int32)))),
        ("pixel must be contiguous", lambda: sc.render_rays(o, d, 8, pixel=gpu(torch.zeros(16, dtype=torch.int32)[::2]))),
        ("n_pixels must be a positive int", lambda: sc.render_rays(o, d, 0)),
        ("out must be a torch tensor on the rays' GPU", lambda: sc.render_rays(o, d, 8, out=torch.zeros(8, 3))),
    ]
    for pattern, call in cases:
        with pytest.raises(api.RtError, match=pattern):
            call()


def test_cpp_wrappers_link_and_throw_the_library_message():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "rayscheck"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "render_rays_api_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(l.split("=", 1) for l in out.stdout.splitlines())
    assert lines["render_rays"] == "render_rays: rt_render_rays_device: null scene"
    assert lines["render_rays_fixed"] == "render_rays_fixed: rt_render_rays_fixed_device: null scene"
    assert lines["out"] == "7 7"
