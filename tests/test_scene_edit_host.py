"""Editing a scene in place, the part that needs no GPU: the five entry points are declared, exported and bound; each
refuses a null scene (or a null out-pointer) with its own name before it touches a device; the torch wrappers reject
tensors they cannot pass on before the library is reached; the C++ wrappers compile, link and throw the library's message.
The bits are pinned on the GPU (tests/test_gpu_scene_edit.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_query_host import _Scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rt_scene_set_materials", "rt_scene_set_lights", "rt_scene_set_triangles", "rt_scene_set_triangles_device",
         "rt_scene_create_device"]


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


def test_entry_points_are_declared_exported_and_bound(api):
    header = open(os.path.join(ROOT, "include", "rtcuda_amd.h")).read()
    L = api.lib()
    n_args = {"rt_scene_set_materials": 3, "rt_scene_set_lights": 4, "rt_scene_set_triangles": 9, "rt_scene_set_triangles_device": 10,
              "rt_scene_create_device": 10}
    for name in NAMES:
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M)
        assert decl, name
        assert decl.group(1).count(",") + 1 == n_args[name] == len(getattr(L, name).argtypes), name
        assert name in api.EXPORTS
    for method in ("set_materials", "set_lights", "set_triangles", "set_triangles_tensors", "from_tensors", "n_tris"):
        assert callable(getattr(api.Scene, method))


def test_null_scene_errors_carry_the_entry_points_name(api):
    L = api.lib()
    mats = np.zeros(1, np.dtype("V20"))
    lights = np.zeros(1, np.dtype("V32"))
    tris = np.zeros(9, np.float32)
    idx = np.zeros(1, np.int32)
    m, l, t, i = (x.ctypes.data for x in (mats, lights, tris, idx))
    calls = {
        "rt_scene_set_materials": lambda: L.rt_scene_set_materials(None, m, 1),
        "rt_scene_set_lights": lambda: L.rt_scene_set_lights(None, l, 1, None),
        "rt_scene_set_triangles": lambda: L.rt_scene_set_triangles(None, t, 1, i, None, m, 1, l, 0),
        "rt_scene_set_triangles_device": lambda: L.rt_scene_set_triangles_device(None, t, 1, i, None, m, 1, l, 0, None),
        "rt_scene_create_device": lambda: L.rt_scene_create_device(t, 1, i, None, m, 1, l, 0, None, None),
    }
    assert sorted(calls) == sorted(NAMES)
    for name, call in calls.items():
        assert call() != 0, name
        msg = L.rt_last_error().decode()
        assert msg.startswith(name + ": ") and "null" in msg, msg


def test_torch_wrappers_reject_cpu_tensors_before_reaching_the_library(api):
    torch = pytest.importorskip("torch")
    sc = _Scene(api)
    t, m, l = torch.zeros(4, 9), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    mats, lights = np.zeros(1, np.dtype("V20")), np.zeros(0, np.dtype("V32"))
    with pytest.raises(api.RtError, match="set_triangles_tensors: tris must be on the scene's GPU"):
        sc.set_triangles_tensors(t, m, l, mats, lights)
    with pytest.raises(api.RtError, match="from_tensors: tris must be on the scene's GPU"):
        api.Scene.from_tensors(t, m, l, mats, lights)
    with pytest.raises(api.RtError, match="tris must be a torch tensor"):
        sc.set_triangles_tensors(np.zeros((4, 9), np.float32), m, l, mats, lights)


def test_torch_wrappers_reject_dtype_layout_and_shape(api):
    """As tests/test_query_host.py: CPU tensors whose class says they are on a GPU stand in; every case must raise before
    a pointer is taken."""
    torch = pytest.importorskip("torch")

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    def gpu(x):
        return x.as_subclass(OnGpu)

    sc = _Scene(api)
    t, m, l = gpu(torch.zeros(4, 9)), gpu(torch.zeros(4, dtype=torch.int32)), gpu(torch.zeros(4, dtype=torch.int32))
    mats, lights = np.zeros(1, np.dtype("V20")), np.zeros(0, np.dtype("V32"))
    i32 = dict(dtype=torch.int32)
    cases = [
        ("tris must be torch.float32", (gpu(torch.zeros(4, 9, dtype=torch.float64)), m, l)),
        (r"tris must have shape \(n, 9\) or \(n, 3, 3\)", (gpu(torch.zeros(4, 3)), m, l)),
        (r"tris must have shape \(n, 9\) or \(n, 3, 3\)", (gpu(torch.zeros(36)), m, l)),
        (r"tris must have shape \(n, 9\) or \(n, 3, 3\)", (gpu(torch.zeros(4, 3, 4)), m, l)),
        ("tris must be contiguous", (gpu(torch.zeros(9, 4).t()), m, l)),
        ("tri_material must be torch.int32", (t, gpu(torch.zeros(4, dtype=torch.int64)), l)),
        (r"tri_material must have shape \(4,\)", (t, gpu(torch.zeros(5, **i32)), l)),
        ("tri_material must be contiguous", (t, gpu(torch.zeros(8, **i32)[::2]), l)),
        ("tri_material must be a torch tensor", (t, None, l)),
        ("tri_light must be torch.int32", (t, m, gpu(torch.zeros(4)))),
        (r"tri_light must have shape \(4,\)", (t, m, gpu(torch.zeros(4, 1, **i32)))),
    ]
    for pattern, args in cases:
        with pytest.raises(api.RtError, match="set_triangles_tensors: " + pattern):
            sc.set_triangles_tensors(*args, mats, lights)
        with pytest.raises(api.RtError, match="from_tensors: " + pattern):
            api.Scene.from_tensors(*args, mats, lights)
    with pytest.raises(api.RtError, match="20 / 32 bytes"):
        sc.set_triangles_tensors(gpu(torch.zeros(4, 3, 3)), m, None, np.zeros(1, np.float32), lights)


def test_cpp_wrappers_link_and_throw_the_library_message():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "editcheck"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "scene_edit_api_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(l.split("=", 1) for l in out.stdout.splitlines())
    assert lines["set_lights"] == "2" and lines["set_triangles"] == "1"
    assert lines["set_triangles_device"] == "set_triangles_device: rt_scene_set_triangles_device: null scene"
    assert lines["create_scene_device"] == "rt_scene_create_device: out_scene is null"
