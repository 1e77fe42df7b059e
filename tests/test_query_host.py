"""CPU tests of the ray-query entry points (rt_query_closest_device / rt_query_any_device / rt_query_last_counters): what can
be checked without a device.  No scene can be created without a GPU, so the one argument check of the library that runs
here is the null scene; the torch wrappers refuse bad tensors before they reach the library (a fake CUDA tensor stands in
for the device side of those checks); the C++ wrappers link and throw with the library's message.  Everything that traces a
ray is in tests/test_gpu_query.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ("rt_query_closest_device", "rt_query_any_device", "rt_query_last_counters")


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


def test_new_entry_points_are_declared_exported_and_bound(api):
    header = open(os.path.join(ROOT, "include", "rtcuda_amd.h")).read()
    for name in NEW:
        assert name in api.EXPORTS
        assert f"int {name}(" in header
        assert getattr(api.lib(), name).argtypes is not None


def test_null_scene_is_an_error_with_a_message_for_every_new_entry_point(api):
    L = api.lib()
    rays = np.zeros(6, np.float32)
    out = np.full(4, 7, np.int64)
    p = rays.ctypes.data
    calls = {
        "rt_query_closest_device": lambda: L.rt_query_closest_device(None, 0, 1, p, p, None, out.ctypes.data, None, None, None, None),
        "rt_query_any_device": lambda: L.rt_query_any_device(None, 0, 1, p, p, None, None, out.ctypes.data, None),
        "rt_query_last_counters": lambda: L.rt_query_last_counters(None, out.ctypes.data),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = L.rt_last_error().decode()
        assert name in msg and "null" in msg, msg
    assert (out == 7).all()  # nothing was written


class _Scene:
    """The wrappers' checks run before the library is reached: a Scene without a device scene is enough to show it (a call
    that got past the checks would fail on the missing handle, with another message)."""

    def __new__(cls, api):
        s = api.Scene.__new__(api.Scene)
        s.L, s.h = api.lib(), None
        return s


def test_torch_wrappers_reject_cpu_tensors_before_reaching_the_library(api):
    torch = pytest.importorskip("torch")
    sc = _Scene(api)
    o = torch.zeros(8, 3)
    d = torch.zeros(8, 3)
    with pytest.raises(api.RtError, match="query_closest: origins must be on the scene's GPU"):
        sc.query_closest(o, d)
    with pytest.raises(api.RtError, match="query_any: origins must be on the scene's GPU"):
        sc.query_any(o, d)
    with pytest.raises(api.RtError, match="origins must be a torch tensor"):
        sc.query_closest(np.zeros((8, 3), np.float32), d)


def test_torch_wrappers_reject_dtype_layout_and_shape(api, monkeypatch):
    """The remaining checks need tensors that say they are on a GPU.  `is_cuda` is the only thing the wrapper asks about the
    device before those checks, so CPU tensors whose class answers True stand in; every case must raise before a pointer
    is taken."""
    torch = pytest.importorskip("torch")

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    def gpu(x):
        return x.as_subclass(OnGpu)

    sc = _Scene(api)
    o, d = gpu(torch.zeros(8, 3)), gpu(torch.zeros(8, 3))
    cases = [
        ("dirs must be torch.float32", lambda: sc.query_closest(o, gpu(torch.zeros(8, 3, dtype=torch.float64)))),
        ("origins must be torch.float32", lambda: sc.query_any(gpu(torch.zeros(8, 3, dtype=torch.float64)), d)),
        ("origins must be contiguous", lambda: sc.query_closest(gpu(torch.zeros(3, 8).t()), d)),
        ("dirs must be contiguous", lambda: sc.query_closest(o, gpu(torch.zeros(8, 6)[:, ::2]))),
        (r"origins must have shape \(n, 3\)", lambda: sc.query_closest(gpu(torch.zeros(8, 4)), d)),
        (r"origins must have shape \(n, 3\)", lambda: sc.query_closest(gpu(torch.zeros(24)), d)),
        (r"dirs must have shape \(n, 3\)", lambda: sc.query_closest(o, gpu(torch.zeros(7, 3)))),
        (r"tmax must have shape \(n,\)", lambda: sc.query_closest(o, d, gpu(torch.zeros(8, 1)))),
        ("tmax must be torch.float32", lambda: sc.query_any(o, d, gpu(torch.zeros(8, dtype=torch.float16)))),
        ("excluded must be torch.int32", lambda: sc.query_any(o, d, None, gpu(torch.zeros(8, dtype=torch.int64)))),
        (r"excluded must have shape \(n,\)", lambda: sc.query_any(o, d, None, gpu(torch.zeros(9, dtype=torch.int32)))),
    ]
    for pattern, call in cases:
        with pytest.raises(api.RtError, match=pattern):
            call()


def test_cpp_wrappers_link_and_throw_the_library_message():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "querycheck"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "query_api_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(l.split("=", 1) for l in out.stdout.splitlines())
    assert lines["query_closest"] == "query_closest: rt_query_closest_device: null scene"
    assert lines["query_any"] == "query_any: rt_query_any_device: null scene"
    assert lines["out"] == "7"
