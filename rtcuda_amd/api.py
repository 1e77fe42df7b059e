"""ctypes binding of ``librtcuda_amd.so`` (the C-ABI in ``include/rtcuda_amd.h``).

Mirrors the reference's host interface for the render path -- ``Scene`` construction from
triangles / materials / lights, ``Camera(lookfrom, lookat, up, vfov, aspect)`` and
``render(width, height, spp, max_bounces, camera, scene)`` (render.cuh:366-367) -- on top of the
library.  Nothing here computes pixels: every call goes to the HIP library and raises
``RtError`` if it fails or ``ImportError`` if the library has not been built.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
import subprocess

import numpy as np

from .scenes import SceneArrays

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, os.environ.get("RT_LIB_NAME", "librtcuda_amd.so"))  # RT_LIB_NAME: instrumented dev builds
CSRC = os.path.join(_PKG, "csrc")

W = 1 << 20  # RT_NUM_WORKING_PATHS
FLAG_TIME_KERNELS = 1
FLAG_DETERMINISTIC = 2
FLAG_RNG_PER_SAMPLE = 4  # NOT the reference's random numbers (see include/rtcuda_amd.h): partition-invariant streams
FLAG_REFERENCE_WALK = 8  # cross-check mode: every ray walks the reference's own tree literally (slow; the default kernels give the same image)
SCENE_DEVICE_BVH = 1     # rt_scene_create_flags: build the BVH on the device (PLOC)
FLAG_WATERTIGHT = 16     # the triangle-list definition (no hit lost to a box test, ties by caller index) instead of the reference's
AOV_CHANNELS = 11        # rt_render_aov_*: int64 sums per pixel, interleaved
AOV_FOLLOW_MAX = 5       # RT_AOV_FOLLOW_MAX: the largest max_specular of the followed AOVs
AOV_ALBEDO, AOV_NORMAL, AOV_EMISSION, AOV_DEPTH, AOV_HITS = 0, 3, 6, 9, 10  # first channel of each feature

EXPORTS = [
    "rt_scene_create", "rt_scene_destroy", "rt_scene_info", "rt_scene_build_info", "rt_scene_update", "rt_scene_update_device",
    "rt_scene_refit_info", "rt_scene_create_flags", "rt_scene_rebuild", "rt_scene_rebuild_device", "rt_scene_set_materials",
    "rt_scene_set_lights", "rt_scene_set_triangles", "rt_scene_set_triangles_device", "rt_scene_create_device", "rt_camera_make", "rt_render", "rt_render_multi",
    "rt_render_shard", "rt_render_shard_fixed", "rt_render_rays_device", "rt_render_rays_fixed_device",
    "rt_render_rays_keyed_device", "rt_render_rays_keyed_fixed_device", "rt_post_process", "rt_post_process_fixed", "rt_trace_closest", "rt_trace_any",
    "rt_trace_closest_flags", "rt_trace_any_flags", "rt_query_closest_device", "rt_query_any_device", "rt_query_last_counters",
    "rt_render_aov_fixed", "rt_render_aov_rays_fixed_device", "rt_aov_resolve",
    "rt_render_aov_follow_fixed", "rt_render_aov_follow_rays_fixed_device",
    "rt_render_counts_fixed", "rt_normalize_counts_fixed", "rt_post_process_counts_fixed", "rt_sample_allocate",
    "rt_denoise_scratch_bytes", "rt_denoise_default_params", "rt_denoise_fixed",
    "rt_denoise_dual_scratch_bytes", "rt_denoise_dual_default_params", "rt_denoise_dual_fixed",
    "rt_render_motion", "rt_temporal_default_params", "rt_temporal_accumulate_fixed",
    "rt_temporal_moments_default_params", "rt_temporal_accumulate_moments_fixed", "rt_denoise_variance_fixed",
    "rt_upsample_default_params", "rt_upsample_fixed", "rt_upsample_rgb",
    "rt_xorwow_states", "rt_shutdown", "rt_peer_access_log", "rt_last_error", "rt_version", "rt_build_id",
]
# the lab (include/rtcuda_amd_tools.h, librtcuda_amd_tools.so): measurement tools, not part of the drop-in C-ABI
TOOLS_LIB_PATH = os.path.join(_PKG, "librtcuda_amd_tools.so")
TOOLS_EXPORTS = ["rt_measure_copy_bandwidth", "rt_calibrate_valu", "rt_calibrate_valu_packed", "rt_probe_issue", "rt_split_probe",
                 "rt_scene_tree_copy", "rt_shade_table", "rt_shade_records", "rt_denoise_pass_time",
                 "rt_denoise_dual_pass_time"]


class RtError(RuntimeError):
    pass


class RtStats(ctypes.Structure):
    _fields_ = [
        ("camera_rays", ctypes.c_int64), ("shade_events", ctypes.c_int64), ("closest_rays", ctypes.c_int64),
        ("any_rays", ctypes.c_int64), ("emission_adds", ctypes.c_int64), ("shadow_adds", ctypes.c_int64),
        ("rr_draws", ctypes.c_int64), ("iterations", ctypes.c_int64), ("bvh_nodes", ctypes.c_int64),
        ("bvh_depth", ctypes.c_int64), ("seconds_render", ctypes.c_double), ("seconds_rng_init", ctypes.c_double),
        ("seconds_trace", ctypes.c_double), ("seconds_reference_tree", ctypes.c_double), ("seconds_advance", ctypes.c_double),
        ("launches_trace", ctypes.c_int64), ("reserved", ctypes.c_int64 * 7),
    ]

    def as_dict(self) -> dict:
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}
        d["lds_top_records"] = int(self.reserved[2])  # BVH records the persistent kernel staged in LDS
        d["slot_chunk"] = max((int(self.reserved[1]) & 0xffffffff) - 1, 0)  # camera rays per task of k_paths<PathsChunked>'s deal; 0: the static deal
        d["slot_head"] = (int(self.reserved[1]) >> 32) & 0xffff  # slot sets a lane ran as in the static deal before that deal began
        d["background_skip"] = (int(self.reserved[1]) >> 48) & 1  # the launch was k_paths<PathsBg> / k_paths<PathsChunkedBg>
        # default kernels (no RT_FLAG_WATERTIGHT): closest hits re-traced through the reference's own tree, accepted hits the
        # reference's box test loses, exact ties at the final distance
        d["literal_retraces"], d["reference_lost_hits"], d["exact_ties"] = (int(self.reserved[k]) for k in (4, 5, 6))
        return d


class RtDenoiseParams(ctypes.Structure):
    _fields_ = [("passes", ctypes.c_int32), ("sigma_color", ctypes.c_float), ("sigma_depth", ctypes.c_float),
                ("normal_power_log2", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class RtDenoiseDualParams(ctypes.Structure):
    _fields_ = [("passes", ctypes.c_int32), ("sigma_variance", ctypes.c_float), ("sigma_depth", ctypes.c_float),
                ("normal_power_log2", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class RtUpsampleParams(ctypes.Structure):
    _fields_ = [("sigma_depth", ctypes.c_float), ("normal_power_log2", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class RtTemporalParams(ctypes.Structure):
    _fields_ = [("max_history", ctypes.c_int32), ("alpha_min", ctypes.c_float), ("depth_tolerance", ctypes.c_float),
                ("normal_cos_min", ctypes.c_float), ("flags", ctypes.c_uint32)]


class RtTemporalMomentsParams(ctypes.Structure):
    _fields_ = [("max_history", ctypes.c_int32), ("alpha_min", ctypes.c_float), ("depth_tolerance", ctypes.c_float),
                ("normal_cos_min", ctypes.c_float), ("emission_tolerance", ctypes.c_float), ("variance_min_history", ctypes.c_int32),
                ("flags", ctypes.c_uint32)]


def build(verbose: bool = False) -> str:
    """Compile the library in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", CSRC], stdout=out)
    return LIB_PATH


_lib = None


def _preload_hip_runtime() -> None:
    """Make ONE HIP runtime globally visible before the library is loaded.

    librtcuda_amd.so deliberately carries no DT_NEEDED on libamdhip64 (see csrc/Makefile): a
    PyTorch-ROCm wheel ships its own libamdhip64.so, and a second runtime in the same process
    finds no GPU.  When torch is installed its copy is used (bench.py needs torch.distributed in
    the same process); otherwise the system ROCm runtime.
    """
    candidates = []
    try:
        import torch  # noqa: F401
        candidates.append(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    except ImportError:
        pass
    candidates += ["/opt/rocm/lib/libamdhip64.so", "libamdhip64.so"]
    for c in candidates:
        if os.path.isabs(c) and not os.path.exists(c):
            continue
        try:
            ctypes.CDLL(c, mode=ctypes.RTLD_GLOBAL)
            return
        except OSError:
            continue
    raise ImportError("no HIP runtime (libamdhip64.so) could be loaded")


def lib():
    """Load the library (once).  Raises ImportError with the build command if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP library is the product and there is no fallback. "
            f"Build it with `make -C {CSRC}` (or python -c 'import __graft_entry__ as g; g.build()').")
    _preload_hip_runtime()
    _lib = _bind(ctypes.CDLL(LIB_PATH))
    return _lib


def _bind(L):
    """Argument types of the drop-in C-ABI (include/rtcuda_amd.h) on a loaded library."""
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.rt_last_error.restype = ctypes.c_char_p
    L.rt_version.restype = ctypes.c_char_p
    L.rt_build_id.restype = ctypes.c_char_p
    L.rt_scene_create.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, ctypes.POINTER(vp)]
    L.rt_scene_destroy.argtypes = [vp]
    L.rt_scene_destroy.restype = None
    L.rt_scene_info.argtypes = [vp, vp]
    L.rt_scene_build_info.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_double)]
    L.rt_scene_update.argtypes = [vp, vp, ci]
    L.rt_scene_update_device.argtypes = [vp, vp, ci, vp]
    L.rt_scene_refit_info.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double),
                                      ctypes.POINTER(ctypes.c_double)]
    L.rt_scene_create_flags.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, ctypes.c_uint32, ctypes.POINTER(vp)]
    L.rt_scene_rebuild.argtypes = [vp, vp, ci]
    L.rt_scene_rebuild_device.argtypes = [vp, vp, ci, vp]
    L.rt_scene_set_materials.argtypes = [vp, vp, ci]
    L.rt_scene_set_lights.argtypes = [vp, vp, ci, vp]
    L.rt_scene_set_triangles.argtypes = [vp, vp, ci, vp, vp, vp, ci, vp, ci]
    L.rt_scene_set_triangles_device.argtypes = [vp, vp, ci, vp, vp, vp, ci, vp, ci, vp]
    L.rt_scene_create_device.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, vp, ctypes.POINTER(vp)]
    L.rt_camera_make.argtypes = [vp, vp, vp, cf, cf, vp]
    L.rt_render.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.c_uint64, ctypes.c_uint32, vp, ctypes.POINTER(RtStats)]
    L.rt_render_multi.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.c_uint64, ctypes.c_uint32, vp, ci, vp, ctypes.POINTER(RtStats)]
    L.rt_render_shard.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.c_uint64, ci, ci, ctypes.c_uint32, vp, vp,
                                  ctypes.POINTER(RtStats)]
    L.rt_post_process.argtypes = [vp, ci, ci, vp]
    L.rt_render_shard_fixed.argtypes = L.rt_render_shard.argtypes
    L.rt_post_process_fixed.argtypes = [vp, vp, ci, ci, vp]
    L.rt_render_rays_device.argtypes = [vp, ctypes.c_int64, vp, vp, vp, ci, ci, ci, ctypes.c_uint64, ctypes.c_uint32, vp, vp,
                                        ctypes.POINTER(RtStats)]
    L.rt_render_rays_fixed_device.argtypes = L.rt_render_rays_device.argtypes
    L.rt_render_rays_keyed_device.argtypes = [vp, ctypes.c_int64, vp, vp, vp, ci, ci, ci, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                              ctypes.c_uint32, vp, vp, ctypes.POINTER(RtStats)]
    L.rt_render_rays_keyed_fixed_device.argtypes = L.rt_render_rays_keyed_device.argtypes
    L.rt_render_counts_fixed.argtypes = [vp, vp, ci, ci, ci, vp, vp, ci, ctypes.c_uint64, ctypes.c_uint32, vp, vp, vp, ctypes.POINTER(RtStats)]
    L.rt_normalize_counts_fixed.argtypes = [vp, vp, ci, vp, vp]
    L.rt_post_process_counts_fixed.argtypes = [vp, vp, ci, vp, vp]
    L.rt_sample_allocate.argtypes = [vp, ci, ci, ci, ctypes.c_int64, vp, ctypes.POINTER(ctypes.c_int64), vp]
    L.rt_render_aov_fixed.argtypes = [vp, vp, ci, ci, ci, ctypes.c_uint64, ci, ci, ctypes.c_uint32, vp, vp, vp, ctypes.POINTER(RtStats)]
    L.rt_render_aov_follow_fixed.argtypes = [vp, vp, ci, ci, ci, ctypes.c_uint64, ci, ci, ctypes.c_uint32, ci, vp, vp, vp, ctypes.POINTER(RtStats)]
    L.rt_render_aov_follow_rays_fixed_device.argtypes = [vp, ctypes.c_int64, vp, vp, vp, ci, ci, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                                         ctypes.c_uint32, ci, vp, vp, vp, ctypes.POINTER(RtStats)]
    L.rt_render_aov_rays_fixed_device.argtypes = [vp, ctypes.c_int64, vp, vp, vp, ci, ci, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                                  vp, vp, vp, ctypes.POINTER(RtStats)]
    L.rt_aov_resolve.argtypes = [vp, vp, ci, ci, vp]
    L.rt_denoise_scratch_bytes.argtypes = [ci, ci]
    L.rt_denoise_scratch_bytes.restype = ctypes.c_int64
    L.rt_denoise_default_params.argtypes = [ctypes.POINTER(RtDenoiseParams)]
    L.rt_denoise_fixed.argtypes = [vp, ci, vp, ci, ci, ci, ctypes.POINTER(RtDenoiseParams), vp, vp, vp]
    L.rt_denoise_dual_scratch_bytes.argtypes = [ci, ci]
    L.rt_denoise_dual_scratch_bytes.restype = ctypes.c_int64
    L.rt_denoise_dual_default_params.argtypes = [ctypes.POINTER(RtDenoiseDualParams)]
    L.rt_denoise_dual_fixed.argtypes = [vp, ci, vp, ci, vp, ci, ci, ci, ctypes.POINTER(RtDenoiseDualParams), vp, vp, vp]
    L.rt_render_motion.argtypes = [vp, vp, ci, ci, vp, vp, ctypes.c_uint32, vp, vp, ctypes.POINTER(RtStats)]
    L.rt_temporal_default_params.argtypes = [ctypes.POINTER(RtTemporalParams)]
    L.rt_temporal_accumulate_fixed.argtypes = [vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ctypes.POINTER(RtTemporalParams),
                                               vp, vp, vp, vp]
    L.rt_temporal_moments_default_params.argtypes = [ctypes.POINTER(RtTemporalMomentsParams)]
    L.rt_temporal_accumulate_moments_fixed.argtypes = [vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, ci, ci,
                                                       ctypes.POINTER(RtTemporalMomentsParams), vp, vp, vp, vp, vp, vp]
    L.rt_denoise_variance_fixed.argtypes = [vp, ci, vp, vp, ci, ci, ci, ctypes.POINTER(RtDenoiseDualParams), vp, vp, vp]
    L.rt_upsample_default_params.argtypes = [ctypes.POINTER(RtUpsampleParams)]
    L.rt_upsample_fixed.argtypes = [vp, ci, vp, ci, ci, ci, ci, vp, ci, ctypes.POINTER(RtUpsampleParams), vp, vp, vp]
    L.rt_upsample_rgb.argtypes = [vp, vp, ci, ci, ci, ci, vp, ci, ctypes.POINTER(RtUpsampleParams), vp, vp, vp]
    L.rt_trace_closest.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
    L.rt_trace_any.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.rt_trace_closest_flags.argtypes = [vp, ctypes.c_uint32, ci, vp, vp, vp, vp, vp, vp, vp]
    L.rt_trace_any_flags.argtypes = [vp, ctypes.c_uint32, ci, vp, vp, vp, vp, vp]
    L.rt_query_closest_device.argtypes = [vp, ctypes.c_uint32, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rt_query_any_device.argtypes = [vp, ctypes.c_uint32, ci, vp, vp, vp, vp, vp, vp]
    L.rt_query_last_counters.argtypes = [vp, vp]
    L.rt_xorwow_states.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ci, vp, vp]
    L.rt_shutdown.restype = None
    L.rt_peer_access_log.restype = ctypes.c_char_p
    return L


_tools = None


def tools_lib():
    """The LAB library (librtcuda_amd_tools.so: the product's translation unit + the measurement tools of
    include/rtcuda_amd_tools.h).  Loaded on first use by bench.py's roofline block and tools/*.py -- never by a render."""
    global _tools
    if _tools is not None:
        return _tools
    if not os.path.exists(TOOLS_LIB_PATH):
        raise ImportError(f"{TOOLS_LIB_PATH} not found: build it with `make -C {CSRC}`")
    _preload_hip_runtime()
    L = _bind(ctypes.CDLL(TOOLS_LIB_PATH))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.rt_measure_copy_bandwidth.argtypes = [ctypes.c_int64, ci, ctypes.POINTER(ctypes.c_double)]
    L.rt_calibrate_valu.argtypes = [ci, ci, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.rt_calibrate_valu_packed.argtypes = [ci, ci, ci, ctypes.POINTER(ctypes.c_double)]
    L.rt_probe_issue.argtypes = [ci, ci, ci, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.rt_split_probe.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.c_uint64, ctypes.c_int64, vp, ci]
    L.rt_scene_tree_copy.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp]
    L.rt_shade_table.argtypes = [ci, ci, vp, vp]
    L.rt_shade_records.argtypes = [vp, ci, ci, ci, vp, vp]
    L.rt_denoise_pass_time.argtypes = [vp, ci, ci, ci, ci, ctypes.c_float, ctypes.c_float, ci, ci, vp]
    L.rt_denoise_dual_pass_time.argtypes = [vp, ci, ci, ci, ci, ci, ctypes.c_float, ctypes.c_float, ci, ci, vp]
    _tools = L
    return L


def shutdown() -> None:
    """Release the library's hidden device allocations (render contexts, cached output buffers): rt_shutdown."""
    lib().rt_shutdown()


def peer_access_log() -> str:
    """rt_render_multi: what became of peer access between the listed devices (rt_peer_access_log)."""
    return lib().rt_peer_access_log().decode()


def build_id() -> str:
    """Hash of the sources + flags the LOADED library's device code was built from (rt_build_id)."""
    return lib().rt_build_id().decode()


def _check(rc: int, what: str, library=None) -> None:
    if rc != 0:
        raise RtError(f"{what}: {(library or lib()).rt_last_error().decode(errors='replace')}")


def _p(a):
    return None if a is None else a.ctypes.data


def make_camera(lookfrom=(0.5, 0.5, 1.5), lookat=(0.5, 0.5, 0.0), up=(0.0, 1.0, 0.0), vfov=37.8,
                aspect=1.0) -> np.ndarray:
    """``Camera(lookfrom, lookat, up, vfov, aspect)`` (camera.cuh:15-29) -> the 12-float POD."""
    a, b, c = (np.asarray(v, np.float32) for v in (lookfrom, lookat, up))
    out = np.zeros(12, np.float32)
    _check(lib().rt_camera_make(_p(a), _p(b), _p(c), float(vfov), float(aspect), _p(out)), "rt_camera_make")
    return out


class Scene:
    """Device-resident scene (triangles, materials, lights, BVH) on the current HIP device."""

    def __init__(self, arrays: SceneArrays, library=None, device_bvh: bool = False):
        """`library`: the loaded library that owns the scene -- the product (default) or `tools_lib()`, whose private copy of
        the product's entry points is what rt_split_probe works on.  `device_bvh`: build the BVH on the device
        (RT_SCENE_DEVICE_BVH, the PLOC builder) instead of the host SAH builder; the image is the same."""
        L = self.L = library or lib()
        self.arrays = arrays
        tris = np.ascontiguousarray(arrays.tris, np.float32)
        tm = np.ascontiguousarray(arrays.tri_material, np.int32)
        tl = np.ascontiguousarray(arrays.tri_light, np.int32)
        mats = np.ascontiguousarray(arrays.materials)
        lights = np.ascontiguousarray(arrays.lights)
        assert mats.dtype.itemsize == 20 and lights.dtype.itemsize == 32
        h = ctypes.c_void_p()
        _check(L.rt_scene_create_flags(_p(tris), tris.shape[0], _p(tm), _p(tl), _p(mats), mats.shape[0], _p(lights),
                                       lights.shape[0], SCENE_DEVICE_BVH if device_bvh else 0, ctypes.byref(h)),
               "rt_scene_create", L)
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.rt_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        out = np.zeros(4, np.int64)
        _check(self.L.rt_scene_info(self.h, _p(out)), "rt_scene_info", self.L)
        b, sec = ctypes.c_int(0), ctypes.c_double(0.0)
        _check(self.L.rt_scene_build_info(self.h, ctypes.byref(b), ctypes.byref(sec)), "rt_scene_build_info", self.L)
        return {"pairs": int(out[0]), "tris": int(out[1]), "max_depth": int(out[2]), "leaves": int(out[3]),
                "builder": {0: "sah", 2: "ploc"}.get(b.value, str(b.value)), "build_seconds": sec.value}

    def n_tris(self) -> int:
        """The scene's current triangle count, from the library (rt_scene_info): it follows set_triangles*()."""
        out = np.zeros(4, np.int64)
        _check(self.L.rt_scene_info(self.h, _p(out)), "rt_scene_info", self.L)
        return int(out[1])

    # ---- editing in place: materials, lights, a new triangle set (rt_scene_set_*).  Renders and queries afterwards are
    # bit-equal to those of a scene created from the same arrays; an RtError leaves the scene as it was.
    @staticmethod
    def _tables(materials, lights):
        mats = np.ascontiguousarray(materials)
        lights = np.ascontiguousarray(lights)
        if mats.dtype.itemsize != 20 or lights.dtype.itemsize != 32:
            raise RtError("materials / lights must be arrays of scenes.MATERIAL_DTYPE / scenes.LIGHT_DTYPE records (20 / 32 bytes)")
        return mats, lights

    def set_materials(self, materials) -> None:
        """A new material table (records as in SceneArrays.materials; any count that covers the triangles' indices).  The tree
        and everything in leaf order stay: the cost is a table upload and one small launch."""
        mats, _ = self._tables(materials, self.arrays.lights if self.arrays is not None else np.zeros(0, "V32"))
        _check(self.L.rt_scene_set_materials(self.h, _p(mats), mats.shape[0]), "rt_scene_set_materials", self.L)
        if self.arrays is not None:
            self.arrays = dataclasses.replace(self.arrays, materials=mats)

    def set_lights(self, lights, tri_light=None) -> None:
        """New lights and, unless tri_light is None, a new light assignment of the triangles ((n,) int32, -1 = none)."""
        _, lights = self._tables(np.zeros(0, "V20"), lights)
        tl = None if tri_light is None else np.ascontiguousarray(tri_light, np.int32)
        if tl is not None and tl.shape != (self.n_tris(),):
            raise RtError(f"set_lights: tri_light must have shape ({self.n_tris()},), it has {tl.shape}")
        _check(self.L.rt_scene_set_lights(self.h, _p(lights), lights.shape[0], _p(tl)), "rt_scene_set_lights", self.L)
        if self.arrays is not None:
            self.arrays = dataclasses.replace(self.arrays, lights=lights, **({} if tl is None else {"tri_light": tl}))

    def set_triangles(self, arrays: SceneArrays) -> None:
        """A whole new scene description in place (any triangle count >= 1): the tree is built on the device."""
        tris = np.ascontiguousarray(arrays.tris, np.float32).reshape(-1, 9)
        tm = np.ascontiguousarray(arrays.tri_material, np.int32)
        tl = np.ascontiguousarray(arrays.tri_light, np.int32)
        mats, lights = self._tables(arrays.materials, arrays.lights)
        if tm.shape != (tris.shape[0],) or tl.shape != (tris.shape[0],):
            raise RtError(f"set_triangles: {tris.shape[0]} triangles, tri_material {tm.shape}, tri_light {tl.shape}")
        _check(self.L.rt_scene_set_triangles(self.h, _p(tris), tris.shape[0], _p(tm), _p(tl), _p(mats), mats.shape[0], _p(lights),
                                             lights.shape[0]), "rt_scene_set_triangles", self.L)
        self.arrays = arrays

    @staticmethod
    def _triangle_tensors(what, tris, tri_material, tri_light):
        """The checks of set_triangles_tensors / from_tensors, in the manner of _query_rays: contiguous CUDA tensors on one
        GPU, (n, 9) or (n, 3, 3) float32 and (n,) int32 (tri_light may be None).  Nothing is converted or copied."""
        import torch
        n, device = None, None
        for name, x, dtype in (("tris", tris, torch.float32), ("tri_material", tri_material, torch.int32),
                               ("tri_light", tri_light, torch.int32)):
            if x is None and name == "tri_light":
                continue  # (optional: no area lights)
            if not isinstance(x, torch.Tensor):
                raise RtError(f"{what}: {name} must be a torch tensor, it is a {type(x).__name__}")
            if not x.is_cuda:
                raise RtError(f"{what}: {name} must be on the scene's GPU, it is on {x.device}")
            if x.dtype != dtype:
                raise RtError(f"{what}: {name} must be {dtype}, it is {x.dtype}")
            if name == "tris":
                if x.dim() not in (2, 3) or tuple(x.shape[1:]) not in ((9,), (3, 3)):
                    raise RtError(f"{what}: tris must have shape (n, 9) or (n, 3, 3), it has {tuple(x.shape)}")
                n = x.shape[0]
            elif tuple(x.shape) != (n,):
                raise RtError(f"{what}: {name} must have shape ({n},), it has {tuple(x.shape)}")
            if not x.is_contiguous():
                raise RtError(f"{what}: {name} must be contiguous")
            device = x.device if device is None else device
            if x.device != device:
                raise RtError(f"{what}: {name} is on {x.device}, tris are on {device}")
        return n, device

    def set_triangles_tensors(self, tris, tri_material, tri_light, materials, lights) -> None:
        """set_triangles() from torch tensors on the scene's device (tris (n, 9) or (n, 3, 3) float32; tri_material and
        tri_light (n,) int32, tri_light may be None), ordered on ``torch.cuda.current_stream()``; materials and lights are
        host record arrays.  The index ranges are checked on the device.  ``self.arrays`` no longer describes the scene
        afterwards and is set to None."""
        import torch
        n, device = self._triangle_tensors("set_triangles_tensors", tris, tri_material, tri_light)
        mats, lights = self._tables(materials, lights)
        c = ctypes.c_void_p
        _check(self.L.rt_scene_set_triangles_device(self.h, c(tris.data_ptr()), n, c(tri_material.data_ptr()),
                                                    c(None if tri_light is None else tri_light.data_ptr()), _p(mats), mats.shape[0],
                                                    _p(lights), lights.shape[0], c(torch.cuda.current_stream(device).cuda_stream or None)),
               "rt_scene_set_triangles_device", self.L)
        self.arrays = None

    @classmethod
    def from_tensors(cls, tris, tri_material, tri_light, materials, lights, library=None) -> "Scene":
        """A scene made from torch tensors on the current device without a host copy of the triangles
        (rt_scene_create_device: the device BVH builder); arguments as set_triangles_tensors()."""
        import torch
        n, device = cls._triangle_tensors("from_tensors", tris, tri_material, tri_light)
        mats, lights = cls._tables(materials, lights)
        self = cls.__new__(cls)
        L = self.L = library or lib()
        self.arrays = None
        self.h = None
        c, h = ctypes.c_void_p, ctypes.c_void_p()
        with torch.cuda.device(device):
            _check(L.rt_scene_create_device(c(tris.data_ptr()), n, c(tri_material.data_ptr()),
                                            c(None if tri_light is None else tri_light.data_ptr()), _p(mats), mats.shape[0], _p(lights),
                                            lights.shape[0], c(torch.cuda.current_stream(device).cuda_stream or None), ctypes.byref(h)),
                   "rt_scene_create_device", L)
        self.h = h
        return self

    # ---- moving geometry: new vertex positions, same triangles, materials and lights (rt_scene_update)
    def update(self, tris) -> None:
        """New positions for every triangle ((n, 9) float32 p0 p1 p2, the creation order and count): the BVH is refit on the
        device.  Renders afterwards are bit-equal to those of a scene created from the same vertices."""
        tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
        _check(self.L.rt_scene_update(self.h, _p(tris), tris.shape[0]), "rt_scene_update", self.L)

    def update_device(self, ptr: int, stream: int = 0, n_tris: int = None) -> None:
        """The same from a DEVICE buffer of n_tris x 9 float32 on the scene's device (e.g. ``tensor.data_ptr()``), ordered
        on ``stream`` (0 = default stream; synchronous on return).  n_tris defaults to the scene's count."""
        n = self.n_tris() if n_tris is None else int(n_tris)
        _check(self.L.rt_scene_update_device(self.h, ctypes.c_void_p(ptr), n, ctypes.c_void_p(stream)),
               "rt_scene_update_device", self.L)

    # ---- a new tree on the device when the refit one has degraded (rt_scene_rebuild)
    def rebuild(self, tris=None) -> None:
        """A new BVH built on the device (the PLOC builder) from the current vertices (tris None) or from new ones (as
        update() takes them).  Call it when refit_info()["sah_ratio"] has grown.  Renders afterwards are bit-equal to those
        of a scene created from the same vertices."""
        if tris is None:
            _check(self.L.rt_scene_rebuild(self.h, None, self.n_tris()), "rt_scene_rebuild", self.L)
            return
        tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
        _check(self.L.rt_scene_rebuild(self.h, _p(tris), tris.shape[0]), "rt_scene_rebuild", self.L)

    def rebuild_device(self, ptr: int, stream: int = 0, n_tris: int = None) -> None:
        """The same from a DEVICE buffer of n_tris x 9 float32 on the scene's device (e.g. ``tensor.data_ptr()``; 0 = the
        current vertices), ordered on ``stream`` (0 = default stream; synchronous on return)."""
        n = self.n_tris() if n_tris is None else int(n_tris)
        _check(self.L.rt_scene_rebuild_device(self.h, ctypes.c_void_p(ptr or None), n, ctypes.c_void_p(stream or None)),
               "rt_scene_rebuild_device", self.L)

    def refit_info(self) -> dict:
        """Refits since creation, device seconds of the last one, and the tree's surface-area cost relative to build time."""
        refits, sec, ratio = ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        _check(self.L.rt_scene_refit_info(self.h, ctypes.byref(refits), ctypes.byref(sec), ctypes.byref(ratio)),
               "rt_scene_refit_info", self.L)
        return {"refits": refits.value, "seconds_last": sec.value, "sah_ratio": ratio.value}

    # ---- render(): the drop-in entry point
    def render(self, camera: np.ndarray, width: int, height: int, spp: int, max_bounces: int = 10,
               seed: int = 1, flags: int = 0):
        """Whole frame on the current device -> (image (h, w, 3) float32 post-processed, stats)."""
        cam = np.ascontiguousarray(camera, np.float32)
        out = np.zeros((height, width, 3), np.float32)
        st = RtStats()
        _check(self.L.rt_render(self.h, _p(cam), width, height, spp, max_bounces, seed, flags, _p(out),
                               ctypes.byref(st)), "rt_render", self.L)
        return out, st.as_dict()

    def render_multi(self, camera: np.ndarray, width: int, height: int, spp: int, devices, max_bounces: int = 10,
                     seed: int = 1, flags: int = 0):
        """Whole frame over the listed devices in this one process (rt_render_multi) -> (image, stats)."""
        cam = np.ascontiguousarray(camera, np.float32)
        dev = np.ascontiguousarray(devices, np.int32)
        out = np.zeros((height, width, 3), np.float32)
        st = RtStats()
        _check(self.L.rt_render_multi(self.h, _p(cam), width, height, spp, max_bounces, seed, flags, _p(dev), int(dev.shape[0]),
                                     _p(out), ctypes.byref(st)), "rt_render_multi", self.L)
        d = st.as_dict()
        d["device_shards"] = int(st.reserved[3])
        return out, d

    def render_shard(self, camera: np.ndarray, width: int, height: int, spp: int, shard_index: int,
                     shard_count: int, d_sum_ptr: int, max_bounces: int = 10, seed: int = 1, flags: int = 0,
                     stream: int = 0) -> dict:
        """Adds this shard's raw sums into the DEVICE buffer at ``d_sum_ptr`` (w*h*3 floats)."""
        cam = np.ascontiguousarray(camera, np.float32)
        st = RtStats()
        _check(self.L.rt_render_shard(self.h, _p(cam), width, height, spp, max_bounces, seed, shard_index,
                                     shard_count, flags, ctypes.c_void_p(d_sum_ptr), ctypes.c_void_p(stream),
                                     ctypes.byref(st)), "rt_render_shard", self.L)
        return st.as_dict()

    def render_shard_fixed(self, camera: np.ndarray, width: int, height: int, spp: int, shard_index: int,
                           shard_count: int, d_sum_fixed_ptr: int, max_bounces: int = 10, seed: int = 1, flags: int = 0,
                           stream: int = 0) -> dict:
        """Order-independent accumulation: adds int64 fixed-point sums (2^-30) into the DEVICE buffer."""
        cam = np.ascontiguousarray(camera, np.float32)
        st = RtStats()
        _check(self.L.rt_render_shard_fixed(self.h, _p(cam), width, height, spp, max_bounces, seed, shard_index,
                                           shard_count, flags, ctypes.c_void_p(d_sum_fixed_ptr), ctypes.c_void_p(stream),
                                           ctypes.byref(st)), "rt_render_shard_fixed", self.L)
        return st.as_dict()

    # ---- radiance along the caller's camera rays (rt_render_rays_device / rt_render_rays_fixed_device)
    def render_rays_device(self, o_ptr: int, d_ptr: int, pixel_ptr: int, n_rays: int, n_pixels: int, d_sum_ptr: int,
                           rays_per_pixel: int = 1, max_bounces: int = 10, seed: int = 1, flags: int = 0, fixed: bool = False,
                           stream: int = 0) -> dict:
        """A frame of n_rays camera rays from DEVICE buffers on the scene's device (origins and directions n_rays x 3 float32;
        pixel n_rays int32, or 0: ray c lands on pixel c // rays_per_pixel).  Raw sums are ADDED into the DEVICE buffer at
        ``d_sum_ptr``: n_pixels x 3 float32, or with ``fixed`` int64 in units of 2^-30.  Ordered on ``stream`` (0 = default
        stream), synchronous on return."""
        c = ctypes.c_void_p
        name = "rt_render_rays_fixed_device" if fixed else "rt_render_rays_device"
        st = RtStats()
        _check(getattr(self.L, name)(self.h, int(n_rays), c(o_ptr or None), c(d_ptr or None), c(pixel_ptr or None), int(rays_per_pixel),
                                     int(n_pixels), int(max_bounces), seed, flags, c(d_sum_ptr or None), c(stream or None),
                                     ctypes.byref(st)), name, self.L)
        return st.as_dict()

    def render_rays(self, origins, dirs, n_pixels: int, pixel=None, rays_per_pixel: int = 1, max_bounces: int = 10, seed: int = 1,
                    flags: int = 0, fixed: bool = False, out=None):
        """Radiance along torch rays: origins, dirs (n, 3) float32 and pixel (n,) int32 or None (ray c lands on pixel
        c // rays_per_pixel), contiguous, on the scene's device -> (sums, stats): an (n_pixels, 3) tensor of raw sums there --
        float32, or with ``fixed`` int64 in units of 2^-30 -- ordered on ``torch.cuda.current_stream()``.  ``out``: such a
        tensor to ADD into instead of a new zeroed one."""
        import torch
        n, device = self._query_rays("render_rays", origins, dirs, None)
        if pixel is not None:
            self._query_rays("render_rays", origins, dirs, None, pixel, "pixel")
        dtype = torch.int64 if fixed else torch.float32
        if out is None:
            if not isinstance(n_pixels, int) or n_pixels < 1:
                raise RtError(f"render_rays: n_pixels must be a positive int, it is {n_pixels!r}")
            out = torch.zeros((n_pixels, 3), dtype=dtype, device=device)
        else:
            if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != device:
                raise RtError("render_rays: out must be a torch tensor on the rays' GPU")
            if out.dtype != dtype or tuple(out.shape) != (n_pixels, 3) or not out.is_contiguous():
                raise RtError(f"render_rays: out must be a contiguous ({n_pixels}, 3) {dtype} tensor, it is {tuple(out.shape)} {out.dtype}")
        st = self.render_rays_device(origins.data_ptr(), dirs.data_ptr(), 0 if pixel is None else pixel.data_ptr(), n, n_pixels,
                                     out.data_ptr(), rays_per_pixel, max_bounces, seed, flags, fixed,
                                     torch.cuda.current_stream(device).cuda_stream)
        return out, st

    # ---- the same with a per-sample stream per ray (rt_render_rays_keyed_device / rt_render_rays_keyed_fixed_device)
    def render_rays_keyed_device(self, o_ptr: int, d_ptr: int, pixel_ptr: int, n_rays: int, n_pixels: int, d_sum_ptr: int,
                                 rays_per_pixel: int = 1, key_first: int = 0, key_stride: int = 1, max_bounces: int = 10, seed: int = 1,
                                 flags: int = 0, fixed: bool = False, stream: int = 0) -> dict:
        """A keyed frame of n_rays camera rays from DEVICE buffers (as render_rays_device): row c has the 64-bit key
        K = key_first + c * key_stride, the random numbers of camera ray K of a FLAG_RNG_PER_SAMPLE frame, and lands on pixel
        pixel[c] or, with pixel_ptr 0, K // rays_per_pixel.  Raw sums are ADDED into the DEVICE buffer at ``d_sum_ptr``; with
        ``fixed`` any split of a table by key range or stride adds up to exactly the whole frame's sums."""
        c = ctypes.c_void_p
        name = "rt_render_rays_keyed_fixed_device" if fixed else "rt_render_rays_keyed_device"
        for what, v, top in (("key_first", key_first, 1 << 64), ("key_stride", key_stride, 1 << 32), ("seed", seed, 1 << 64)):
            if not isinstance(v, int) or not 0 <= v < top:  # (ctypes would wrap it silently)
                raise RtError(f"{name}: {what} must be an int in 0 .. 2^{top.bit_length() - 1} - 1, it is {v!r}")
        st = RtStats()
        _check(getattr(self.L, name)(self.h, int(n_rays), c(o_ptr or None), c(d_ptr or None), c(pixel_ptr or None), int(rays_per_pixel),
                                     int(n_pixels), int(max_bounces), seed, key_first, key_stride, flags, c(d_sum_ptr or None),
                                     c(stream or None), ctypes.byref(st)), name, self.L)
        return st.as_dict()

    def render_rays_keyed(self, origins, dirs, n_pixels: int, pixel=None, rays_per_pixel: int = 1, key_first: int = 0, key_stride: int = 1,
                          max_bounces: int = 10, seed: int = 1, fixed: bool = False, out=None, stream=None):
        """Radiance along torch rays with a stream per ray (render_rays' tensors and checks; see render_rays_keyed_device for
        the keys) -> (sums, stats).  ``out``: an (n_pixels, 3) tensor to ADD into -- chunks of one table, rendered with
        key_first = the chunk's first row, accumulate into one buffer.  ``stream``: a torch stream (default: the current one)."""
        import torch
        n, device = self._query_rays("render_rays_keyed", origins, dirs, None)
        if pixel is not None:
            self._query_rays("render_rays_keyed", origins, dirs, None, pixel, "pixel")
        dtype = torch.int64 if fixed else torch.float32
        if out is None:
            if not isinstance(n_pixels, int) or n_pixels < 1:
                raise RtError(f"render_rays_keyed: n_pixels must be a positive int, it is {n_pixels!r}")
            out = torch.zeros((n_pixels, 3), dtype=dtype, device=device)
        else:
            if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != device:
                raise RtError("render_rays_keyed: out must be a torch tensor on the rays' GPU")
            if out.dtype != dtype or tuple(out.shape) != (n_pixels, 3) or not out.is_contiguous():
                raise RtError(f"render_rays_keyed: out must be a contiguous ({n_pixels}, 3) {dtype} tensor, it is {tuple(out.shape)} {out.dtype}")
        s = torch.cuda.current_stream(device) if stream is None else stream
        st = self.render_rays_keyed_device(origins.data_ptr(), dirs.data_ptr(), 0 if pixel is None else pixel.data_ptr(), n, n_pixels,
                                           out.data_ptr(), rays_per_pixel, key_first, key_stride, max_bounces, seed, 0, fixed, s.cuda_stream)
        return out, st

    # ---- a sample count per pixel (rt_render_counts_fixed)
    def render_counts(self, camera: np.ndarray, width: int, height: int, sample_stride: int, count, first=None, samples=None,
                      max_bounces: int = 10, seed: int = 1, flags: int = 0, out=None, stream=None):
        """The samples first[p] .. first[p] + count[p] - 1 of every pixel p of the FLAG_RNG_PER_SAMPLE frame (width, height,
        sample_stride, seed) -> (sums, stats): sample k of pixel p is camera ray p * sample_stride + k of that frame.  ``count``
        and ``first`` (None: all 0) are (width * height,) int32 tensors on one GPU; the (width * height, 3) int64 fixed-point sums
        (units of 2^-30) are ADDED into ``out`` when one is given, and ``samples`` (a (width * height,) int32 tensor) gets the
        counts ADDED: the divisor for normalize_counts / post_process_counts.  Calls whose ranges tile [0, sample_stride) add up
        to exactly the whole frame's sums, in any order.  ``stream``: a torch stream (default: the current one)."""
        import torch
        me = "render_counts"
        for name, v in (("width", width), ("height", height), ("sample_stride", sample_stride)):
            if not isinstance(v, int) or isinstance(v, bool) or v < 1:
                raise RtError(f"{me}: {name} must be a positive int, it is {v!r}")
        if not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise RtError(f"{me}: seed must be an int in 0 .. 2^64 - 1, it is {seed!r}")
        cam = np.ascontiguousarray(camera, np.float32)
        if cam.shape != (12,):
            raise RtError(f"{me}: camera must be the 12 floats of make_camera(), it has shape {cam.shape}")
        n = width * height
        if not isinstance(count, torch.Tensor) or not count.is_cuda:
            raise RtError(f"{me}: count must be a torch tensor on a GPU")
        device = count.device
        for name, t in (("count", count), ("first", first), ("samples", samples)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
                raise RtError(f"{me}: {name} must be a torch tensor on the GPU of count")
            if t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous():
                raise RtError(f"{me}: {name} must be a contiguous ({n},) torch.int32 tensor, it is {tuple(t.shape)} {t.dtype}")
        if out is None:
            out = torch.zeros((n, 3), dtype=torch.int64, device=device)
        else:
            if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != device:
                raise RtError(f"{me}: out must be a torch tensor on the GPU of count")
            if out.dtype != torch.int64 or tuple(out.shape) != (n, 3) or not out.is_contiguous():
                raise RtError(f"{me}: out must be a contiguous ({n}, 3) torch.int64 tensor, it is {tuple(out.shape)} {out.dtype}")
        s = torch.cuda.current_stream(device) if stream is None else stream
        c = ctypes.c_void_p
        st = RtStats()
        _check(self.L.rt_render_counts_fixed(self.h, _p(cam), width, height, sample_stride, c(None if first is None else first.data_ptr()),
                                             c(count.data_ptr()), int(max_bounces), seed, flags, c(out.data_ptr()),
                                             c(None if samples is None else samples.data_ptr()), c(s.cuda_stream or None), ctypes.byref(st)),
               "rt_render_counts_fixed", self.L)
        return out, st.as_dict()

    # ---- first-hit feature buffers (rt_render_aov_fixed / rt_render_aov_rays_fixed_device)
    @staticmethod
    def _aov_buffers(what, n_pixels, ids, out, device):
        """The sum buffer (a new zeroed one, or `out` checked) and the id buffer (or None) of an AOV call."""
        import torch
        if not isinstance(n_pixels, int) or n_pixels < 1:
            raise RtError(f"{what}: n_pixels must be a positive int, it is {n_pixels!r}")
        if out is None:
            out = torch.zeros((n_pixels, AOV_CHANNELS), dtype=torch.int64, device=device)
        else:
            if not isinstance(out, torch.Tensor) or not out.is_cuda or (device is not None and out.device != device):
                raise RtError(f"{what}: out must be a torch tensor on the scene's GPU")
            if out.dtype != torch.int64 or tuple(out.shape) != (n_pixels, AOV_CHANNELS) or not out.is_contiguous():
                raise RtError(f"{what}: out must be a contiguous ({n_pixels}, {AOV_CHANNELS}) torch.int64 tensor, it is {tuple(out.shape)} {out.dtype}")
        if ids is None or ids is False:
            return out, None
        if ids is True:
            return out, torch.full((n_pixels, 2), -1, dtype=torch.int32, device=out.device)
        if not isinstance(ids, torch.Tensor) or not ids.is_cuda or ids.device != out.device:
            raise RtError(f"{what}: ids must be a bool or a torch tensor on the scene's GPU")
        if ids.dtype != torch.int32 or tuple(ids.shape) != (n_pixels, 2) or not ids.is_contiguous():
            raise RtError(f"{what}: ids must be a contiguous ({n_pixels}, 2) torch.int32 tensor, it is {tuple(ids.shape)} {ids.dtype}")
        return out, ids

    def render_aov(self, camera: np.ndarray, width: int, height: int, spp: int, seed: int = 1, flags: int = 0, shard=(0, 1),
                   ids=False, out=None, stream=None):
        """First-hit features of the camera's per-sample frame -> (sums, ids or None, stats): an (width * height, 11) int64
        tensor of fixed-point sums (units of 2^-30; channels AOV_ALBEDO, AOV_NORMAL, AOV_EMISSION, AOV_DEPTH, AOV_HITS) on the
        current device, ADDED into ``out`` when one is given; with ``ids`` (True, or a (width * height, 2) int32 tensor to
        write into) {triangle, material} of every pixel's first sample, -1 on a miss.  ``shard=(r, R)``: the samples G with
        G % R == r (spp % R == 0); the shards' sums add up to the whole frame's.  Sample G is camera ray G of a
        FLAG_RNG_PER_SAMPLE frame of the same seed.  ``flags``: 0, FLAG_REFERENCE_WALK or FLAG_WATERTIGHT."""
        return self._render_aov("render_aov", None, camera, width, height, spp, seed, flags, shard, ids, out, stream)

    def render_aov_follow(self, camera: np.ndarray, width: int, height: int, spp: int, max_specular: int, seed: int = 1, flags: int = 0,
                          shard=(0, 1), ids=False, out=None, stream=None):
        """render_aov with mirror and glass followed to the first non-specular vertex (rt_render_aov_follow_fixed): a sample whose
        hit is specular goes on as sample G of the FLAG_RNG_PER_SAMPLE beauty frame does, for up to ``max_specular`` (0 ..
        AOV_FOLLOW_MAX) vertices, and deposits beta * albedo, the faced normal and the path length of the vertex its chain ends
        on; emission and ``ids`` stay the first hit's.  max_specular = 0 is render_aov, bit for bit.  stats["closest_rays"]
        counts the chain rays too."""
        return self._render_aov("render_aov_follow", max_specular, camera, width, height, spp, seed, flags, shard, ids, out, stream)

    def _render_aov(self, what, max_specular, camera, width, height, spp, seed, flags, shard, ids, out, stream):
        import torch
        for name, v in (("width", width), ("height", height), ("spp", spp)):
            if not isinstance(v, int) or v < 1:
                raise RtError(f"{what}: {name} must be a positive int, it is {v!r}")
        if not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise RtError(f"{what}: seed must be an int in 0 .. 2^64 - 1, it is {seed!r}")
        r, R = shard
        cam = np.ascontiguousarray(camera, np.float32)
        if cam.shape != (12,):
            raise RtError(f"{what}: camera must be the 12 floats of make_camera(), it has shape {cam.shape}")
        out, ids = self._aov_buffers(what, width * height, ids, out, None if out is not None else torch.device("cuda", torch.cuda.current_device()))
        s = torch.cuda.current_stream(out.device) if stream is None else stream
        c = ctypes.c_void_p
        st = RtStats()
        tail = (c(out.data_ptr()), c(None if ids is None else ids.data_ptr()), c(s.cuda_stream or None), ctypes.byref(st))
        if max_specular is None:
            _check(self.L.rt_render_aov_fixed(self.h, _p(cam), width, height, spp, seed, int(r), int(R), flags, *tail), "rt_render_aov_fixed", self.L)
        else:
            if not isinstance(max_specular, int) or isinstance(max_specular, bool):
                raise RtError(f"{what}: max_specular must be an int, it is {max_specular!r}")
            _check(self.L.rt_render_aov_follow_fixed(self.h, _p(cam), width, height, spp, seed, int(r), int(R), flags, max_specular, *tail),
                   "rt_render_aov_follow_fixed", self.L)
        return out, ids, st.as_dict()

    def render_aov_rays(self, origins, dirs, n_pixels: int, pixel=None, rays_per_pixel: int = 1, key_first: int = 0, key_stride: int = 1,
                        flags: int = 0, ids=False, out=None, stream=None):
        """First-hit features along torch rays (render_rays_keyed's tensors and checks): row c has the key
        key_first + c * key_stride and lands on pixel[c] or, without a pixel tensor, key // rays_per_pixel -> (sums, ids or
        None, stats) as render_aov.  ``ids`` needs pixel=None.  Chunks of one table, each with key_first = its first row,
        accumulate into one ``out``."""
        return self._render_aov_rays("render_aov_rays", None, 0, origins, dirs, n_pixels, pixel, rays_per_pixel, key_first, key_stride, flags,
                                     ids, out, stream)

    def render_aov_follow_rays(self, origins, dirs, n_pixels: int, max_specular: int, seed: int = 1, pixel=None, rays_per_pixel: int = 1,
                               key_first: int = 0, key_stride: int = 1, flags: int = 0, ids=False, out=None, stream=None):
        """render_aov_rays with mirror and glass followed as render_aov_follow follows them
        (rt_render_aov_follow_rays_fixed_device): row c continues on the stream of (seed, key_first + c * key_stride) behind its
        first two draws, as render_rays_keyed's row does."""
        if not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise RtError(f"render_aov_follow_rays: seed must be an int in 0 .. 2^64 - 1, it is {seed!r}")
        return self._render_aov_rays("render_aov_follow_rays", max_specular, seed, origins, dirs, n_pixels, pixel, rays_per_pixel, key_first,
                                     key_stride, flags, ids, out, stream)

    def _render_aov_rays(self, what, max_specular, seed, origins, dirs, n_pixels, pixel, rays_per_pixel, key_first, key_stride, flags, ids,
                         out, stream):
        n, device = self._query_rays(what, origins, dirs, None)
        if pixel is not None:
            self._query_rays(what, origins, dirs, None, pixel, "pixel")
        for name, v, top in (("key_first", key_first, 1 << 64), ("key_stride", key_stride, 1 << 32)):
            if not isinstance(v, int) or not 0 <= v < top:  # (ctypes would wrap it silently)
                raise RtError(f"{what}: {name} must be an int in 0 .. 2^{top.bit_length() - 1} - 1, it is {v!r}")
        if pixel is not None and ids is not None and ids is not False:
            raise RtError(f"{what}: ids together with a pixel tensor (ids belong to the pixels of the key rule)")
        out, ids = self._aov_buffers(what, n_pixels, ids, out, device)
        import torch
        s = torch.cuda.current_stream(device) if stream is None else stream
        c = ctypes.c_void_p
        st = RtStats()
        head = (self.h, n, c(origins.data_ptr()), c(dirs.data_ptr()), c(None if pixel is None else pixel.data_ptr()), int(rays_per_pixel), n_pixels)
        tail = (c(out.data_ptr()), c(None if ids is None else ids.data_ptr()), c(s.cuda_stream or None), ctypes.byref(st))
        if max_specular is None:
            _check(self.L.rt_render_aov_rays_fixed_device(*head, key_first, key_stride, flags, *tail), "rt_render_aov_rays_fixed_device", self.L)
        else:
            if not isinstance(max_specular, int) or isinstance(max_specular, bool):
                raise RtError(f"{what}: max_specular must be an int, it is {max_specular!r}")
            _check(self.L.rt_render_aov_follow_rays_fixed_device(*head, seed, key_first, key_stride, flags, max_specular, *tail),
                   "rt_render_aov_follow_rays_fixed_device", self.L)
        return out, ids, st.as_dict()

    # ---- where every pixel's first hit was one frame ago (rt_render_motion)
    def render_motion(self, camera: np.ndarray, width: int, height: int, prev_camera: np.ndarray, prev_tris=None, flags: int = 0,
                      out=None, stream=None):
        """The motion buffer of the camera's frame -> (records, stats): a (width * height, 4) float32 tensor on the current
        device, per pixel {sx, sy, dist, bits of the hit triangle}: where the first hit of the ray through the pixel centre lay
        in ``prev_camera``'s image (continuous pixel coordinates; -1, -1 when it was behind that camera), its distance from
        that camera, and the triangle in the caller's order (``records[:, 3].view(torch.int32)``; -1 and zeros on a miss).
        ``prev_tris``: the vertices of one frame ago, an (n_tris, 9) or (n_tris, 3, 3) float32 tensor on the scene's device, or
        None when they did not move.  ``flags``: 0, FLAG_REFERENCE_WALK or FLAG_WATERTIGHT.  ``out``: the tensor to fill."""
        import torch
        what = "render_motion"
        for name, v in (("width", width), ("height", height)):
            if not isinstance(v, int) or isinstance(v, bool) or v < 1:
                raise RtError(f"{what}: {name} must be a positive int, it is {v!r}")
        cams = []
        for name, c in (("camera", camera), ("prev_camera", prev_camera)):
            c = np.ascontiguousarray(c, np.float32)
            if c.shape != (12,):
                raise RtError(f"{what}: {name} must be the 12 floats of make_camera(), it has shape {c.shape}")
            cams.append(c)
        n = width * height
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
        elif not isinstance(out, torch.Tensor) or not out.is_cuda:
            raise RtError(f"{what}: out must be a torch tensor on the scene's GPU")
        elif out.dtype != torch.float32 or tuple(out.shape) != (n, 4) or not out.is_contiguous():
            raise RtError(f"{what}: out must be a contiguous ({n}, 4) torch.float32 tensor, it is {tuple(out.shape)} {out.dtype}")
        if prev_tris is not None:
            if not isinstance(prev_tris, torch.Tensor) or not prev_tris.is_cuda or prev_tris.device != out.device:
                raise RtError(f"{what}: prev_tris must be a torch tensor on the scene's GPU")
            nt = self.n_tris()
            if prev_tris.dtype != torch.float32 or tuple(prev_tris.shape) not in ((nt, 9), (nt, 3, 3)) or not prev_tris.is_contiguous():
                raise RtError(f"{what}: prev_tris must be a contiguous ({nt}, 9) or ({nt}, 3, 3) torch.float32 tensor, it is "
                              f"{tuple(prev_tris.shape)} {prev_tris.dtype}")
        s = torch.cuda.current_stream(out.device) if stream is None else stream
        c = ctypes.c_void_p
        st = RtStats()
        _check(self.L.rt_render_motion(self.h, _p(cams[0]), width, height, _p(cams[1]), c(None if prev_tris is None else prev_tris.data_ptr()),
                                       flags, c(out.data_ptr()), c(s.cuda_stream or None), ctypes.byref(st)), "rt_render_motion", self.L)
        return out, st.as_dict()

    # ---- ray queries on device buffers (rt_query_*_device)
    def query_closest_device(self, o_ptr: int, d_ptr: int, tmax_ptr: int, n: int, hit_ptr: int, t_ptr: int = 0, u_ptr: int = 0,
                             v_ptr: int = 0, flags: int = 0, stream: int = 0) -> None:
        """Closest hit of n rays from DEVICE buffers on the scene's device (e.g. ``tensor.data_ptr()``; origins and
        directions n x 3 float32, tmax n float32 or 0 = FLT_MAX) into DEVICE buffers: hit triangle (int32, the caller's
        order or -1) and t, u, v (float32, zero on a miss; 0 = not wanted).  Ordered on ``stream`` (0 = default stream),
        synchronous on return."""
        c = ctypes.c_void_p
        _check(self.L.rt_query_closest_device(self.h, flags, int(n), c(o_ptr or None), c(d_ptr or None), c(tmax_ptr or None),
                                              c(hit_ptr or None), c(t_ptr or None), c(u_ptr or None), c(v_ptr or None),
                                              c(stream or None)), "rt_query_closest_device", self.L)

    def query_any_device(self, o_ptr: int, d_ptr: int, tmax_ptr: int, excluded_ptr: int, n: int, occluded_ptr: int,
                         flags: int = 0, stream: int = 0) -> None:
        """Occlusion of n rays from DEVICE buffers: occluded (int32, 0 / 1) <- is there an accepted hit within tmax on a
        triangle other than excluded[i] (int32, the caller's order; 0 = nothing excluded)."""
        c = ctypes.c_void_p
        _check(self.L.rt_query_any_device(self.h, flags, int(n), c(o_ptr or None), c(d_ptr or None), c(tmax_ptr or None),
                                          c(excluded_ptr or None), c(occluded_ptr or None), c(stream or None)),
               "rt_query_any_device", self.L)

    def query_counters(self) -> dict:
        """The rare path of the last query on this scene (rt_query_last_counters)."""
        out = np.zeros(3, np.int64)
        _check(self.L.rt_query_last_counters(self.h, _p(out)), "rt_query_last_counters", self.L)
        return {"retraced": int(out[0]), "lost": int(out[1]), "tied": int(out[2])}

    @staticmethod
    def _query_rays(what, origins, dirs, tmax, excluded=None, excluded_name="excluded"):
        """The checks of query_closest / query_any: torch tensors on one GPU (the scene's), float32 (excluded: int32),
        contiguous, (n, 3) / (n,).  Nothing is converted or copied: a million rays are not silently duplicated."""
        import torch
        n, device = None, None
        for name, x, dtype, cols in (("origins", origins, torch.float32, 3), ("dirs", dirs, torch.float32, 3),
                                     ("tmax", tmax, torch.float32, 0), (excluded_name, excluded, torch.int32, 0)):
            if x is None and not cols:
                continue  # (optional)
            if not isinstance(x, torch.Tensor):
                raise RtError(f"{what}: {name} must be a torch tensor, it is a {type(x).__name__}")
            if not x.is_cuda:
                raise RtError(f"{what}: {name} must be on the scene's GPU, it is on {x.device}")
            if x.dtype != dtype:
                raise RtError(f"{what}: {name} must be {dtype}, it is {x.dtype}")
            if n is None and x.dim() == 2:
                n = x.shape[0]
            if tuple(x.shape) != ((n, 3) if cols else (n,)):
                raise RtError(f"{what}: {name} must have shape {'(n, 3)' if cols else '(n,)'}, it has {tuple(x.shape)}")
            if not x.is_contiguous():
                raise RtError(f"{what}: {name} must be contiguous")
            device = x.device if device is None else device
            if x.device != device:
                raise RtError(f"{what}: {name} is on {x.device}, origins are on {device}")
        return n, device

    def query_closest(self, origins, dirs, tmax=None, flags: int = 0):
        """Closest hits of torch rays: origins, dirs (n, 3) float32 and tmax (n,) float32 or None (no limit), contiguous, on
        the scene's device -> (hit_tri int32, t, u, v float32) tensors there, ordered on ``torch.cuda.current_stream()``."""
        import torch
        n, device = self._query_rays("query_closest", origins, dirs, tmax)
        hit = torch.empty(n, dtype=torch.int32, device=device)
        t, u, v = (torch.empty(n, dtype=torch.float32, device=device) for _ in range(3))
        self.query_closest_device(origins.data_ptr(), dirs.data_ptr(), 0 if tmax is None else tmax.data_ptr(), n, hit.data_ptr(),
                                  t.data_ptr(), u.data_ptr(), v.data_ptr(), flags, torch.cuda.current_stream(device).cuda_stream)
        return hit, t, u, v

    def query_any(self, origins, dirs, tmax=None, excluded=None, flags: int = 0):
        """Occlusion of torch rays (as query_closest; excluded (n,) int32 or None) -> occluded int32 tensor (0 / 1)."""
        import torch
        n, device = self._query_rays("query_any", origins, dirs, tmax, excluded)
        occ = torch.empty(n, dtype=torch.int32, device=device)
        self.query_any_device(origins.data_ptr(), dirs.data_ptr(), 0 if tmax is None else tmax.data_ptr(),
                              0 if excluded is None else excluded.data_ptr(), n, occ.data_ptr(), flags,
                              torch.cuda.current_stream(device).cuda_stream)
        return occ

    # ---- stage-level entry points (parity tests)
    def trace_closest(self, o3, d3, tmax, flags: int = 0):
        """``flags=FLAG_REFERENCE_WALK``: through the reference's own tree and walk (rt_trace_closest_flags)."""
        o3 = np.ascontiguousarray(o3, np.float32)
        d3 = np.ascontiguousarray(d3, np.float32)
        tmax = np.ascontiguousarray(tmax, np.float32)
        n = o3.shape[0]
        tri = np.zeros(n, np.int32)
        t, u, v = (np.zeros(n, np.float32) for _ in range(3))
        if flags:
            _check(self.L.rt_trace_closest_flags(self.h, flags, n, _p(o3), _p(d3), _p(tmax), _p(tri), _p(t), _p(u), _p(v)),
                   "rt_trace_closest_flags", self.L)
        else:
            _check(self.L.rt_trace_closest(self.h, n, _p(o3), _p(d3), _p(tmax), _p(tri), _p(t), _p(u), _p(v)),
                   "rt_trace_closest", self.L)
        return tri, t, u, v

    def trace_any(self, o3, d3, tmax, excluded, flags: int = 0):
        o3 = np.ascontiguousarray(o3, np.float32)
        d3 = np.ascontiguousarray(d3, np.float32)
        tmax = np.ascontiguousarray(tmax, np.float32)
        excluded = np.ascontiguousarray(excluded, np.int32)
        n = o3.shape[0]
        occ = np.zeros(n, np.int32)
        if flags:
            _check(self.L.rt_trace_any_flags(self.h, flags, n, _p(o3), _p(d3), _p(tmax), _p(excluded), _p(occ)),
                   "rt_trace_any_flags", self.L)
        else:
            _check(self.L.rt_trace_any(self.h, n, _p(o3), _p(d3), _p(tmax), _p(excluded), _p(occ)), "rt_trace_any", self.L)
        return occ


def post_process(d_ptr: int, num_pixels: int, spp: int, stream: int = 0) -> None:
    _check(lib().rt_post_process(ctypes.c_void_p(d_ptr), num_pixels, spp, ctypes.c_void_p(stream)),
           "rt_post_process")


def post_process_fixed(d_fixed_ptr: int, d_out_ptr: int, num_pixels: int, spp: int, stream: int = 0) -> None:
    _check(lib().rt_post_process_fixed(ctypes.c_void_p(d_fixed_ptr), ctypes.c_void_p(d_out_ptr), num_pixels, spp,
                                       ctypes.c_void_p(stream)), "rt_post_process_fixed")


def _counts_tensors(me: str, sums, samples):
    """The checks of an (n, 3) int64 sums tensor and its (n,) int32 divisor, both on one GPU -> n."""
    import torch
    if not isinstance(sums, torch.Tensor) or not sums.is_cuda:
        raise RtError(f"{me}: sums must be a torch tensor on a GPU")
    if sums.dtype != torch.int64 or sums.dim() != 2 or sums.shape[1] != 3 or sums.shape[0] < 1 or not sums.is_contiguous():
        raise RtError(f"{me}: sums must be a contiguous (n_pixels, 3) torch.int64 tensor, it is {tuple(sums.shape)} {sums.dtype}")
    n = int(sums.shape[0])
    if not isinstance(samples, torch.Tensor) or not samples.is_cuda or samples.device != sums.device:
        raise RtError(f"{me}: samples must be a torch tensor on the GPU of the sums")
    if samples.dtype != torch.int32 or tuple(samples.shape) != (n,) or not samples.is_contiguous():
        raise RtError(f"{me}: samples must be a contiguous ({n},) torch.int32 tensor, it is {tuple(samples.shape)} {samples.dtype}")
    return n


def normalize_counts(sums, samples, out=None, stream=None):
    """Sums with a per-pixel divisor -> int64 sums of ONE sample of the mean (rt_normalize_counts_fixed): per channel
    sign(s) * ((|s| + (n >> 1)) // n) with n = samples[p], 0 where n == 0.  ``out``: a tensor like ``sums`` to write into
    (``sums`` itself: in place).  The result feeds denoise(out, 1, ...), denoise_variance and the temporal accumulators."""
    import torch
    me = "normalize_counts"
    n = _counts_tensors(me, sums, samples)
    if out is None:
        out = torch.empty_like(sums)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != sums.device:
        raise RtError(f"{me}: out must be a torch tensor on the GPU of the sums")
    elif out.dtype != torch.int64 or tuple(out.shape) != (n, 3) or not out.is_contiguous():
        raise RtError(f"{me}: out must be a contiguous ({n}, 3) torch.int64 tensor, it is {tuple(out.shape)} {out.dtype}")
    s = torch.cuda.current_stream(sums.device) if stream is None else stream
    with torch.cuda.device(sums.device):
        _check(lib().rt_normalize_counts_fixed(ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(samples.data_ptr()), n,
                                               ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(s.cuda_stream or None)), "rt_normalize_counts_fixed")
    return out


def post_process_counts(sums, samples, out=None, stream=None):
    """post_process_fixed with the pixel's own count (rt_post_process_counts_fixed) -> (n_pixels, 3) float32 tensor; 0 where the
    count is 0."""
    import torch
    me = "post_process_counts"
    n = _counts_tensors(me, sums, samples)
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=sums.device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != sums.device:
        raise RtError(f"{me}: out must be a torch tensor on the GPU of the sums")
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, 3) or not out.is_contiguous():
        raise RtError(f"{me}: out must be a contiguous ({n}, 3) torch.float32 tensor, it is {tuple(out.shape)} {out.dtype}")
    s = torch.cuda.current_stream(sums.device) if stream is None else stream
    with torch.cuda.device(sums.device):
        _check(lib().rt_post_process_counts_fixed(ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(samples.data_ptr()), n,
                                                  ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(s.cuda_stream or None)),
               "rt_post_process_counts_fixed")
    return out


def sample_allocate(weight, min_count: int, max_count: int, budget: int, out=None, stream=None):
    """From a weight map to counts under a budget, in exact integers (rt_sample_allocate) -> (counts, total): ``weight`` is an
    (n_pixels,) float32 tensor on a GPU; count[p] = min(max_count, min_count + extra * q[p] // T) with q the weight quantised
    to 2^-20 (0 for NaN, zero and negatives; capped at 4096), T its sum and extra = budget - n_pixels * min_count (an even
    split where T == 0).  ``total`` = the sum of the counts <= budget: what flooring and the cap leave over is not
    redistributed."""
    import torch
    me = "sample_allocate"
    if not isinstance(weight, torch.Tensor) or not weight.is_cuda:
        raise RtError(f"{me}: weight must be a torch tensor on a GPU")
    if weight.dtype != torch.float32 or weight.dim() != 1 or weight.shape[0] < 1 or not weight.is_contiguous():
        raise RtError(f"{me}: weight must be a contiguous (n_pixels,) torch.float32 tensor, it is {tuple(weight.shape)} {weight.dtype}")
    n = int(weight.shape[0])
    for name, v, top in (("min_count", min_count, 1 << 31), ("max_count", max_count, 1 << 31), ("budget", budget, 1 << 63)):
        if not isinstance(v, int) or isinstance(v, bool) or not -top <= v < top:  # (ctypes would wrap it silently)
            raise RtError(f"{me}: {name} must be an int of the C type's range, it is {v!r}")
    if out is None:
        out = torch.empty((n,), dtype=torch.int32, device=weight.device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != weight.device:
        raise RtError(f"{me}: out must be a torch tensor on the GPU of the weights")
    elif out.dtype != torch.int32 or tuple(out.shape) != (n,) or not out.is_contiguous():
        raise RtError(f"{me}: out must be a contiguous ({n},) torch.int32 tensor, it is {tuple(out.shape)} {out.dtype}")
    s = torch.cuda.current_stream(weight.device) if stream is None else stream
    total = ctypes.c_int64(0)
    with torch.cuda.device(weight.device):
        _check(lib().rt_sample_allocate(ctypes.c_void_p(weight.data_ptr()), n, min_count, max_count, budget, ctypes.c_void_p(out.data_ptr()),
                                        ctypes.byref(total), ctypes.c_void_p(s.cuda_stream or None)), "rt_sample_allocate")
    return out, int(total.value)


def aov_resolve(sums, spp: int, stream=None):
    """The float features of AOV sums ((n_pixels, 11) int64 tensor on a GPU; rt_aov_resolve) -> (n_pixels, 11) float32 tensor:
    albedo, normal and emission as means over the ``spp`` samples, depth as the mean over the hits (0 where nothing was hit),
    channel AOV_HITS as coverage."""
    import torch
    if not isinstance(sums, torch.Tensor) or not sums.is_cuda:
        raise RtError("aov_resolve: sums must be a torch tensor on a GPU")
    if sums.dtype != torch.int64 or sums.dim() != 2 or sums.shape[1] != AOV_CHANNELS or not sums.is_contiguous():
        raise RtError(f"aov_resolve: sums must be a contiguous (n_pixels, {AOV_CHANNELS}) torch.int64 tensor, it is {tuple(sums.shape)} {sums.dtype}")
    if not isinstance(spp, int) or spp < 1:
        raise RtError(f"aov_resolve: spp must be a positive int, it is {spp!r}")
    out = torch.empty(tuple(sums.shape), dtype=torch.float32, device=sums.device)
    s = torch.cuda.current_stream(sums.device) if stream is None else stream
    with torch.cuda.device(sums.device):
        _check(lib().rt_aov_resolve(ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(out.data_ptr()), int(sums.shape[0]), spp,
                                    ctypes.c_void_p(s.cuda_stream or None)), "rt_aov_resolve")
    return out


def _dn_default_params(me: str, params, sigma: str) -> dict:
    _check(getattr(lib(), f"rt_{me}_default_params")(ctypes.byref(params)), f"rt_{me}_default_params")
    return {"passes": int(params.passes), sigma: float(getattr(params, sigma)), "sigma_depth": float(params.sigma_depth),
            "normal_power_log2": int(params.normal_power_log2)}


def _dn_scratch_bytes(me: str, width, height) -> int:
    if not isinstance(width, int) or not isinstance(height, int):
        raise RtError(f"{me}_scratch_bytes: width and height must be ints, they are {width!r}, {height!r}")
    n = int(getattr(lib(), f"rt_{me}_scratch_bytes")(width, height))
    if n < 0:
        raise RtError(f"{me}_scratch_bytes: bad frame size {width} x {height}")
    return n


def _dn_positive_ints(me: str, named) -> None:
    for name, v in named:
        if not isinstance(v, int) or isinstance(v, bool) or v < 1:
            raise RtError(f"{me}: {name} must be a positive int, it is {v!r}")


def _dn_sums(me: str, n: int, named):
    """The checks of the sums tensors ((name, tensor, channels), the first names the GPU of the call) -> that GPU."""
    import torch
    for name, t, ch in named:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RtError(f"{me}: {name} must be a torch tensor on a GPU")
        if t.dtype != torch.int64 or tuple(t.shape) != (n, ch) or not t.is_contiguous():
            raise RtError(f"{me}: {name} must be a contiguous ({n}, {ch}) torch.int64 tensor, it is {tuple(t.shape)} {t.dtype}")
    first, device = named[0][0], named[0][1].device
    for name, t, _ in named[1:]:
        if t.device != device:
            raise RtError(f"{me}: {name} is on {t.device}, {first} on {device}")
    return device


def _dn_params(me: str, prm, ints, sigmas, defaults_of=None):
    """``prm`` (a ctypes parameter struct) as the library's defaults (``defaults_of``: the entry point whose defaults they are, if
    not ``me``'s own), overwritten by the (name, value) pairs that are not None."""
    owner = defaults_of or me
    _check(getattr(lib(), f"rt_{owner}_default_params")(ctypes.byref(prm)), f"rt_{owner}_default_params")
    for name, v in ints:
        if v is not None:
            if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= 8:
                raise RtError(f"{me}: {name} must be an int in 0 .. 8, it is {v!r}")
            setattr(prm, name, v)
    for name, v in sigmas:
        if v is not None:
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating)) or not (np.isfinite(v) and v > 0):
                raise RtError(f"{me}: {name} must be a finite positive number, it is {v!r}")
            setattr(prm, name, float(v))
    return prm


def _dn_buffers(me: str, need: int, n: int, device, scratch, out, stream):
    """``scratch`` and ``out`` checked, or made on ``device``, and the stream of the call."""
    import torch
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=device)
    elif not isinstance(scratch, torch.Tensor) or not scratch.is_cuda or scratch.device != device:
        raise RtError(f"{me}: scratch must be a torch tensor on the GPU of the sums")
    elif scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.numel() < need:
        raise RtError(f"{me}: scratch must be a contiguous torch.uint8 tensor of at least {need} bytes, it is {tuple(scratch.shape)} {scratch.dtype}")
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != device:
        raise RtError(f"{me}: out must be a torch tensor on the GPU of the sums")
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, 3) or not out.is_contiguous():
        raise RtError(f"{me}: out must be a contiguous ({n}, 3) torch.float32 tensor, it is {tuple(out.shape)} {out.dtype}")
    return scratch, out, torch.cuda.current_stream(device) if stream is None else stream


def denoise_default_params() -> dict:
    """The parameters rt_denoise_fixed uses when it is given none (rt_denoise_default_params)."""
    return _dn_default_params("denoise", RtDenoiseParams(), "sigma_color")


def denoise_scratch_bytes(width: int, height: int) -> int:
    """Bytes of scratch rt_denoise_fixed needs for a width x height frame (rt_denoise_scratch_bytes)."""
    return _dn_scratch_bytes("denoise", width, height)


def denoise(beauty_sums, spp: int, aov_sums, aov_spp: int, width: int, height: int, *, passes=None, sigma_color=None,
            sigma_depth=None, normal_power_log2=None, scratch=None, out=None, stream=None):
    """The denoised frame (rt_denoise_fixed: an a-trous filter on albedo-demodulated radiance, guided by first-hit normal and depth)
    of fixed-point beauty sums ((h * w, 3) int64, as Scene.render_*_fixed leave them, ``spp`` samples) and AOV sums ((h * w, 11)
    int64, as Scene.render_aov leaves them, ``aov_spp`` samples), both on one GPU -> (h * w, 3) float32 tensor of LINEAR mean
    radiance.  Parameters left at None are the library's defaults (denoise_default_params).  ``scratch``: a contiguous
    torch.uint8 tensor of at least denoise_scratch_bytes(width, height) bytes to reuse between calls (made here otherwise);
    ``out``: the result tensor to fill; ``stream``: a torch.cuda.Stream (the current one otherwise)."""
    import torch
    me = "denoise"
    _dn_positive_ints(me, (("width", width), ("height", height), ("spp", spp), ("aov_spp", aov_spp)))
    n = width * height
    device = _dn_sums(me, n, (("beauty_sums", beauty_sums, 3), ("aov_sums", aov_sums, AOV_CHANNELS)))
    prm = _dn_params(me, RtDenoiseParams(), (("passes", passes), ("normal_power_log2", normal_power_log2)),
                     (("sigma_color", sigma_color), ("sigma_depth", sigma_depth)))
    scratch, out, s = _dn_buffers(me, denoise_scratch_bytes(width, height), n, device, scratch, out, stream)
    with torch.cuda.device(device):
        _check(lib().rt_denoise_fixed(ctypes.c_void_p(beauty_sums.data_ptr()), spp, ctypes.c_void_p(aov_sums.data_ptr()), aov_spp,
                                      width, height, ctypes.byref(prm), ctypes.c_void_p(scratch.data_ptr()),
                                      ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(s.cuda_stream or None)), "rt_denoise_fixed")
    return out


def denoise_dual_default_params() -> dict:
    """The parameters rt_denoise_dual_fixed uses when it is given none (rt_denoise_dual_default_params)."""
    return _dn_default_params("denoise_dual", RtDenoiseDualParams(), "sigma_variance")


def denoise_dual_scratch_bytes(width: int, height: int) -> int:
    """Bytes of scratch rt_denoise_dual_fixed needs for a width x height frame (rt_denoise_dual_scratch_bytes)."""
    return _dn_scratch_bytes("denoise_dual", width, height)


def denoise_dual(beauty_a, spp_a: int, beauty_b, spp_b: int, aov_sums, aov_spp: int, width: int, height: int, *, passes=None,
                 sigma_variance=None, sigma_depth=None, normal_power_log2=None, scratch=None, out=None, stream=None):
    """The denoised frame of TWO HALF FRAMES of one view (rt_denoise_dual_fixed: the a-trous filter of ``denoise`` with its colour
    stop measured in standard deviations of a per-pixel variance estimate, which the difference of the halves supplies).
    ``beauty_a`` / ``beauty_b``: (h * w, 3) int64 fixed-point sums of ``spp_a`` / ``spp_b`` samples, as
    Scene.render_shard_fixed(..., rank 0 / 1, 2, ..., flags=FLAG_RNG_PER_SAMPLE) leaves them in two zeroed buffers (their sum is
    the whole frame); they may be the same tensor (the variance is then 0).  ``aov_sums``: (h * w, 11) int64, as Scene.render_aov
    leaves them.  All on one GPU -> (h * w, 3) float32 tensor of LINEAR mean radiance.  Parameters left at None are the library's
    defaults (denoise_dual_default_params).  ``scratch``: a contiguous torch.uint8 tensor of at least
    denoise_dual_scratch_bytes(width, height) bytes to reuse between calls (made here otherwise); ``out``: the result tensor to
    fill; ``stream``: a torch.cuda.Stream (the current one otherwise)."""
    import torch
    me = "denoise_dual"
    _dn_positive_ints(me, (("width", width), ("height", height), ("spp_a", spp_a), ("spp_b", spp_b), ("aov_spp", aov_spp)))
    if spp_a + spp_b > 0x7FFFFFFF:
        raise RtError(f"denoise_dual: spp_a + spp_b must fit an int32, they are {spp_a} + {spp_b}")
    n = width * height
    device = _dn_sums(me, n, (("beauty_a", beauty_a, 3), ("beauty_b", beauty_b, 3), ("aov_sums", aov_sums, AOV_CHANNELS)))
    prm = _dn_params(me, RtDenoiseDualParams(), (("passes", passes), ("normal_power_log2", normal_power_log2)),
                     (("sigma_variance", sigma_variance), ("sigma_depth", sigma_depth)))
    scratch, out, s = _dn_buffers(me, denoise_dual_scratch_bytes(width, height), n, device, scratch, out, stream)
    with torch.cuda.device(device):
        _check(lib().rt_denoise_dual_fixed(ctypes.c_void_p(beauty_a.data_ptr()), spp_a, ctypes.c_void_p(beauty_b.data_ptr()), spp_b,
                                           ctypes.c_void_p(aov_sums.data_ptr()), aov_spp, width, height, ctypes.byref(prm),
                                           ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                           ctypes.c_void_p(s.cuda_stream or None)), "rt_denoise_dual_fixed")
    return out


def _temporal(me, prm, defaults, entry, history_names, n_out, out_names, beauty_a, spp_a, beauty_b, spp_b, aov_sums, aov_spp, motion, history, width,
              height, moments, ints, floats, emission_tolerance, out, stream):
    """What temporal_accumulate and temporal_accumulate_moments do: the checks, the parameters (``prm``: the entry point's struct,
    which ``defaults`` fills; ``ints`` / ``floats``: (name, value or None) of the caller's), the outputs and the call of ``entry``.
    The older entry point has no previous motion, no moments (a history of ``n_out`` + 2 items, ``n_out`` results) and no
    emission_tolerance."""
    import torch
    two = beauty_b is not None
    _dn_positive_ints(me, (("width", width), ("height", height), ("spp_a", spp_a), ("aov_spp", aov_spp)) + ((("spp_b", spp_b),) if two else ()))
    n = width * height
    named = [("beauty_a", beauty_a, 3)] + ([("beauty_b", beauty_b, 3)] if two else []) + [("aov_sums", aov_sums, AOV_CHANNELS)]
    hist_a = hist_b = length = prev_aov = prev_motion = prev_moments = None
    prev_spp = 1
    if history is not None:
        if not isinstance(history, (tuple, list)) or len(history) != n_out + 2:
            raise RtError(f"{me}: history must be None or {history_names}")
        hist_a, hist_b, length, prev_aov, prev_spp, prev_motion, prev_moments = tuple(history) + (None,) * (5 - n_out)
        if (hist_b is not None) != two:
            raise RtError(f"{me}: history's hist_b and beauty_b must be None together")
        if prev_moments is not None and not moments:
            raise RtError(f"{me}: history's prev_moments needs moments=True")
        _dn_positive_ints(me, (("prev_aov_spp", prev_spp),))
        named += [("history hist_a", hist_a, 3)] + ([("history hist_b", hist_b, 3)] if two else []) + [("history prev_aov_sums", prev_aov, AOV_CHANNELS)]
    device = _dn_sums(me, n, tuple(named))

    def plain(name, t, dtype, shape):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
            raise RtError(f"{me}: {name} must be a torch tensor on the GPU of the sums")
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise RtError(f"{me}: {name} must be a contiguous {shape} {dtype} tensor, it is {tuple(t.shape)} {t.dtype}")

    plain("motion", motion, torch.float32, (n, 4))
    if history is not None:
        plain("history length", length, torch.int32, (n,))
        if prev_motion is not None:
            plain("history prev_motion", prev_motion, torch.float32, (n, 4))
        if prev_moments is not None:
            plain("history prev_moments", prev_moments, torch.float32, (n, 4))
    _check(getattr(lib(), defaults)(ctypes.byref(prm)), defaults)
    for name, v in ints:
        if v is not None:
            if not isinstance(v, int) or isinstance(v, bool) or not 1 <= v <= 0x7FFFFFFF:
                raise RtError(f"{me}: {name} must be an int in 1 .. 2^31 - 1, it is {v!r}")
            setattr(prm, name, v)
    for name, v in floats:
        if v is not None:
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating)) or not np.isfinite(v):
                raise RtError(f"{me}: {name} must be a finite number, it is {v!r}")
            setattr(prm, name, float(v))
    if emission_tolerance is not None:
        if isinstance(emission_tolerance, bool) or not isinstance(emission_tolerance, (int, float, np.floating)):
            raise RtError(f"{me}: emission_tolerance must be a number, it is {emission_tolerance!r}")
        prm.emission_tolerance = float(emission_tolerance)  # (a NaN or a negative one is the library's to refuse)
    if out is None:
        out = (torch.empty((n, 3), dtype=torch.int64, device=device), torch.empty((n, 3), dtype=torch.int64, device=device) if two else None,
               torch.empty(n, dtype=torch.int32, device=device), torch.empty((n, 4), dtype=torch.float32, device=device) if moments else None,
               torch.empty(n, dtype=torch.float32, device=device) if moments else None)[:n_out]
    else:
        if not isinstance(out, (tuple, list)) or len(out) != n_out or (out[1] is not None) != two or any((t is not None) != moments for t in out[3:]):
            raise RtError(f"{me}: out must be {out_names}")
        _dn_sums(me, n, tuple([("out hist_a", out[0], 3)] + ([("out hist_b", out[1], 3)] if two else [])))
        plain("out length", out[2], torch.int32, (n,))
        if moments:
            plain("out moments", out[3], torch.float32, (n, 4))
            plain("out variance", out[4], torch.float32, (n,))
        if out[0].device != device:
            raise RtError(f"{me}: out is on {out[0].device}, beauty_a on {device}")
    s = torch.cuda.current_stream(device) if stream is None else stream
    c = ctypes.c_void_p

    def ptr(t):
        return c(None if t is None else t.data_ptr())

    with torch.cuda.device(device):
        _check(getattr(lib(), entry)(ptr(beauty_a), spp_a, ptr(beauty_b), spp_b if two else 0, ptr(aov_sums), aov_spp, ptr(motion), ptr(hist_a),
                                     ptr(hist_b), ptr(length), ptr(prev_aov), prev_spp, *((ptr(prev_motion), ptr(prev_moments)) if n_out == 5 else ()),
                                     width, height, ctypes.byref(prm), *map(ptr, out), c(s.cuda_stream or None)), entry)
    return tuple(out)


def temporal_default_params() -> dict:
    """The parameters rt_temporal_accumulate_fixed uses when it is given none (rt_temporal_default_params)."""
    prm = RtTemporalParams()
    _check(lib().rt_temporal_default_params(ctypes.byref(prm)), "rt_temporal_default_params")
    return {"max_history": int(prm.max_history), "alpha_min": float(prm.alpha_min), "depth_tolerance": float(prm.depth_tolerance),
            "normal_cos_min": float(prm.normal_cos_min)}


def temporal_accumulate(beauty_a, spp_a: int, beauty_b, spp_b: int, aov_sums, aov_spp: int, motion, history, width: int, height: int, *,
                        max_history=None, alpha_min=None, depth_tolerance=None, normal_cos_min=None, out=None, stream=None):
    """This frame blended into the reprojected history (rt_temporal_accumulate_fixed) -> (hist_a, hist_b or None, length).
    ``beauty_a`` / ``beauty_b``: (h * w, 3) int64 fixed-point sums of ``spp_a`` / ``spp_b`` samples (``beauty_b`` may be None: one
    buffer); ``aov_sums``: (h * w, 11) int64 of this frame, ``aov_spp`` samples; ``motion``: (h * w, 4) float32, as
    Scene.render_motion leaves it.  ``history``: None on the first frame, else the tuple (hist_a, hist_b or None, length,
    prev_aov_sums, prev_aov_spp) of the previous call's results and the previous frame's AOV sums.  The results are (h * w, 3)
    int64 sums that stand for ONE sample of the accumulated mean -- denoise(hist_a, 1, ...) and denoise_dual(hist_a, 1, hist_b, 1,
    ...) take them as they are -- and the (h * w,) int32 history length per pixel.  ``out``: a tuple (hist_a, hist_b or None,
    length) of tensors to fill, none of which may be an input (ping-pong two sets).  Parameters left at None are the library's
    defaults (temporal_default_params)."""
    return _temporal("temporal_accumulate", RtTemporalParams(), "rt_temporal_default_params", "rt_temporal_accumulate_fixed",
                     "(hist_a, hist_b or None, length, prev_aov_sums, prev_aov_spp)", 3, "(hist_a, hist_b or None as beauty_b, length)", beauty_a, spp_a, beauty_b, spp_b, aov_sums, aov_spp, motion, history, width,
                     height, False, (("max_history", max_history),),
                     (("alpha_min", alpha_min), ("depth_tolerance", depth_tolerance), ("normal_cos_min", normal_cos_min)), None, out, stream)


def temporal_moments_default_params() -> dict:
    """The parameters rt_temporal_accumulate_moments_fixed uses when it is given none (rt_temporal_moments_default_params)."""
    prm = RtTemporalMomentsParams()
    _check(lib().rt_temporal_moments_default_params(ctypes.byref(prm)), "rt_temporal_moments_default_params")
    return {"max_history": int(prm.max_history), "alpha_min": float(prm.alpha_min), "depth_tolerance": float(prm.depth_tolerance),
            "normal_cos_min": float(prm.normal_cos_min), "emission_tolerance": float(prm.emission_tolerance),
            "variance_min_history": int(prm.variance_min_history)}


def temporal_accumulate_moments(beauty_a, spp_a: int, beauty_b, spp_b: int, aov_sums, aov_spp: int, motion, history, width: int, height: int, *,
                                moments: bool = True, max_history=None, alpha_min=None, depth_tolerance=None, normal_cos_min=None,
                                emission_tolerance=None, variance_min_history=None, out=None, stream=None):
    """``temporal_accumulate`` with an emission stop, a triangle stop and temporally accumulated moments
    (rt_temporal_accumulate_moments_fixed) -> (hist_a, hist_b or None, length, moments or None, variance or None).
    The arguments are temporal_accumulate's; ``history`` is None on the first frame, else (hist_a, hist_b or None, length,
    prev_aov_sums, prev_aov_spp, prev_motion or None, prev_moments or None): the previous call's results, the previous frame's
    AOV sums and MOTION buffer ((h * w, 4) float32; None: no triangle stop) and the previous call's moments ((h * w, 4) float32;
    None: the moments start again).  With ``moments`` (the default) the call also returns the moments, for the next frame, and
    the (h * w,) float32 variance of the mean of demodulated radiance, which ``denoise_variance`` takes.  ``emission_tolerance``
    may be float('inf') (the stop passes every tap).  ``out``: a tuple of the five results' tensors to fill (None where a result
    is None), none of which may be an input.  Parameters left at None are the library's defaults
    (temporal_moments_default_params)."""
    return _temporal("temporal_accumulate_moments", RtTemporalMomentsParams(), "rt_temporal_moments_default_params",
                     "rt_temporal_accumulate_moments_fixed",
                     "(hist_a, hist_b or None, length, prev_aov_sums, prev_aov_spp, prev_motion or None, prev_moments or None)", 5,
                     "(hist_a, hist_b or None as beauty_b, length, moments and variance or None as ``moments``)", beauty_a, spp_a, beauty_b, spp_b,
                     aov_sums, aov_spp, motion, history, width, height, moments, (("max_history", max_history), ("variance_min_history", variance_min_history)),
                     (("alpha_min", alpha_min), ("depth_tolerance", depth_tolerance), ("normal_cos_min", normal_cos_min)), emission_tolerance, out, stream)


def denoise_variance(beauty_sums, spp: int, variance, aov_sums, aov_spp: int, width: int, height: int, *, passes=None, sigma_variance=None,
                     sigma_depth=None, normal_power_log2=None, scratch=None, out=None, stream=None):
    """``denoise_dual``'s filter on ONE frame and a variance buffer (rt_denoise_variance_fixed).  ``beauty_sums``: (h * w, 3) int64
    sums of ``spp`` samples -- hist_a of temporal_accumulate_moments with spp = 1; ``variance``: (h * w,) float32 on the same
    GPU, the variance of the mean of demodulated radiance summed over the channels, as temporal_accumulate_moments returns it (a
    NaN or a negative value counts as 0, the top is 2^87); ``aov_sums``: (h * w, 11) int64 -> (h * w, 3) float32 tensor of LINEAR
    mean radiance.  Parameters, defaults and scratch are denoise_dual's (denoise_dual_default_params,
    denoise_dual_scratch_bytes)."""
    import torch
    me = "denoise_variance"
    _dn_positive_ints(me, (("width", width), ("height", height), ("spp", spp), ("aov_spp", aov_spp)))
    n = width * height
    device = _dn_sums(me, n, (("beauty_sums", beauty_sums, 3), ("aov_sums", aov_sums, AOV_CHANNELS)))
    if not isinstance(variance, torch.Tensor) or not variance.is_cuda or variance.device != device:
        raise RtError(f"{me}: variance must be a torch tensor on the GPU of the sums")
    if variance.dtype != torch.float32 or tuple(variance.shape) != (n,) or not variance.is_contiguous():
        raise RtError(f"{me}: variance must be a contiguous ({n},) torch.float32 tensor, it is {tuple(variance.shape)} {variance.dtype}")
    prm = _dn_params(me, RtDenoiseDualParams(), (("passes", passes), ("normal_power_log2", normal_power_log2)),
                     (("sigma_variance", sigma_variance), ("sigma_depth", sigma_depth)), defaults_of="denoise_dual")
    scratch, out, s = _dn_buffers(me, denoise_dual_scratch_bytes(width, height), n, device, scratch, out, stream)
    with torch.cuda.device(device):
        _check(lib().rt_denoise_variance_fixed(ctypes.c_void_p(beauty_sums.data_ptr()), spp, ctypes.c_void_p(variance.data_ptr()),
                                               ctypes.c_void_p(aov_sums.data_ptr()), aov_spp, width, height, ctypes.byref(prm),
                                               ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                               ctypes.c_void_p(s.cuda_stream or None)), "rt_denoise_variance_fixed")
    return out


def upsample_default_params() -> dict:
    """The parameters rt_upsample_fixed and rt_upsample_rgb use when they are given none (rt_upsample_default_params)."""
    prm = RtUpsampleParams()
    _check(lib().rt_upsample_default_params(ctypes.byref(prm)), "rt_upsample_default_params")
    return {"sigma_depth": float(prm.sigma_depth), "normal_power_log2": int(prm.normal_power_log2)}


def _upsample(me: str, entry: str, low, low_channels_dtype, spp, aov_lo, aov_spp_lo: int, low_width: int, low_height: int, factor: int, aov_hi,
              aov_spp_hi: int, sigma_depth, normal_power_log2, out, out_fixed, want_rgb: bool, want_fixed: bool, stream):
    """What upsample and upsample_rgb share: the checks of the tensors, the parameters, the outputs made or checked, the call."""
    import torch
    _dn_positive_ints(me, (("low_width", low_width), ("low_height", low_height), ("aov_spp_lo", aov_spp_lo), ("aov_spp_hi", aov_spp_hi)) +
                      ((("spp", spp),) if spp is not None else ()))
    if not isinstance(factor, int) or isinstance(factor, bool) or not 2 <= factor <= 4:
        raise RtError(f"{me}: factor must be 2, 3 or 4, it is {factor!r}")
    n_lo, n = low_width * low_height, factor * factor * low_width * low_height
    low_name, low_dtype = low_channels_dtype
    if low_dtype == torch.int64:
        device = _dn_sums(me, n_lo, ((low_name, low, 3), ("aov_lo", aov_lo, AOV_CHANNELS)))
    else:
        if not isinstance(low, torch.Tensor) or not low.is_cuda:
            raise RtError(f"{me}: {low_name} must be a torch tensor on a GPU")
        if low.dtype != torch.float32 or tuple(low.shape) != (n_lo, 3) or not low.is_contiguous():
            raise RtError(f"{me}: {low_name} must be a contiguous ({n_lo}, 3) torch.float32 tensor, it is {tuple(low.shape)} {low.dtype}")
        device = _dn_sums(me, n_lo, (("aov_lo", aov_lo, AOV_CHANNELS),))
        if low.device != device:
            raise RtError(f"{me}: {low_name} is on {low.device}, aov_lo on {device}")
    if _dn_sums(me, n, (("aov_hi", aov_hi, AOV_CHANNELS),)) != device:
        raise RtError(f"{me}: aov_hi is on {aov_hi.device}, aov_lo on {device}")
    prm = _dn_params(me, RtUpsampleParams(), (("normal_power_log2", normal_power_log2),), (("sigma_depth", sigma_depth),), defaults_of="upsample")
    if not (want_rgb or want_fixed or out is not None or out_fixed is not None):
        raise RtError(f"{me}: at least one of the two outputs must be asked for")
    for name, t, dtype, want in (("out", out, torch.float32, want_rgb), ("out_fixed", out_fixed, torch.int64, want_fixed)):
        if t is not None:
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
                raise RtError(f"{me}: {name} must be a torch tensor on the GPU of the inputs")
            if t.dtype != dtype or tuple(t.shape) != (n, 3) or not t.is_contiguous():
                raise RtError(f"{me}: {name} must be a contiguous ({n}, 3) {dtype} tensor, it is {tuple(t.shape)} {t.dtype}")
    if out is None and want_rgb:
        out = torch.empty((n, 3), dtype=torch.float32, device=device)
    if out_fixed is None and want_fixed:
        out_fixed = torch.empty((n, 3), dtype=torch.int64, device=device)
    s = torch.cuda.current_stream(device) if stream is None else stream
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    head = (ptr(low),) + ((spp,) if spp is not None else ())
    with torch.cuda.device(device):
        _check(getattr(lib(), entry)(*head, ptr(aov_lo), aov_spp_lo, low_width, low_height, factor, ptr(aov_hi), aov_spp_hi, ctypes.byref(prm),
                                     ptr(out), ptr(out_fixed), ctypes.c_void_p(s.cuda_stream or None)), entry)
    return out, out_fixed


def upsample(beauty_lo, spp: int, aov_lo, aov_spp_lo: int, low_width: int, low_height: int, factor: int, aov_hi, aov_spp_hi: int, *,
             sigma_depth=None, normal_power_log2=None, out=None, out_fixed=None, rgb=True, fixed=True, stream=None):
    """A full-resolution frame from a LOW-RESOLUTION beauty frame and FULL-RESOLUTION features (rt_upsample_fixed: joint bilateral
    upsampling of albedo-demodulated radiance, guided by first-hit normal and depth).  ``beauty_lo``: (low_height * low_width, 3)
    int64 sums of ``spp`` samples; ``aov_lo``: the (low_height * low_width, 11) int64 AOV sums of the same view at the low size;
    ``aov_hi``: those at ``factor`` (2, 3 or 4) times the width and the height, same camera.  Returns ``(out, out_fixed)``: the
    (n, 3) float32 LINEAR mean radiance and the (n, 3) int64 sums of ONE sample of it, which denoise(out_fixed, 1, aov_hi, ...),
    denoise_variance and the temporal accumulators take; ``rgb=False`` / ``fixed=False`` leaves one of them out (None in its
    place), ``out`` / ``out_fixed`` are tensors to fill.  Parameters left at None are the library's defaults
    (upsample_default_params); ``stream``: a torch.cuda.Stream (the current one otherwise)."""
    import torch
    return _upsample("upsample", "rt_upsample_fixed", beauty_lo, ("beauty_lo", torch.int64), spp, aov_lo, aov_spp_lo, low_width, low_height, factor,
                     aov_hi, aov_spp_hi, sigma_depth, normal_power_log2, out, out_fixed, rgb, fixed, stream)


def upsample_rgb(rgb_lo, aov_lo, aov_spp_lo: int, low_width: int, low_height: int, factor: int, aov_hi, aov_spp_hi: int, *, sigma_depth=None,
                 normal_power_log2=None, out=None, out_fixed=None, rgb=True, fixed=True, stream=None):
    """``upsample`` of a FLOAT frame (rt_upsample_rgb): ``rgb_lo`` is (low_height * low_width, 3) float32 linear mean radiance, a
    denoiser's output at the low size for example; a value that is NaN or infinite counts as 0.  Everything else is upsample's."""
    import torch
    return _upsample("upsample_rgb", "rt_upsample_rgb", rgb_lo, ("rgb_lo", torch.float32), None, aov_lo, aov_spp_lo, low_width, low_height, factor,
                     aov_hi, aov_spp_hi, sigma_depth, normal_power_log2, out, out_fixed, rgb, fixed, stream)


def xorwow_states(seed: int, first: int, count: int, draws: int = 0):
    st = np.zeros((count, 6), np.uint32)
    uni = np.zeros((count, max(draws, 1)), np.float32)
    _check(lib().rt_xorwow_states(seed, first, count, draws, _p(st), _p(uni)), "rt_xorwow_states")
    return st, uni[:, :draws]


def measure_copy_bandwidth(nbytes: int = 1 << 30, reps: int = 5) -> float:
    out = ctypes.c_double(0.0)
    _check(tools_lib().rt_measure_copy_bandwidth(nbytes, reps, ctypes.byref(out)), "rt_measure_copy_bandwidth", tools_lib())
    return out.value


def calibrate_valu(waves_per_simd: int = 4, iters: int = 20000):
    """(lane-operations/s the vector ALUs sustain on independent v_fma_f32, wave-instructions per launch)."""
    rate, winstr = ctypes.c_double(0.0), ctypes.c_double(0.0)
    _check(tools_lib().rt_calibrate_valu(waves_per_simd, iters, ctypes.byref(rate), ctypes.byref(winstr)), "rt_calibrate_valu", tools_lib())
    return rate.value, winstr.value


def calibrate_valu_packed(waves_per_simd: int = 4, iters: int = 20000, kind: int = 1) -> float:
    """Lane-operations/s of a packed-fp32 stream (kind 1 v_pk_fma_f32, 2 v_pk_mul_f32, 3 v_pk_add_f32; 2 per lane and instruction)."""
    rate = ctypes.c_double(0.0)
    _check(tools_lib().rt_calibrate_valu_packed(waves_per_simd, iters, kind, ctypes.byref(rate)), "rt_calibrate_valu_packed", tools_lib())
    return rate.value


PROBE_ISSUE_KINDS = ["v_fma_f32", "v_fmac_f32", "v_mul_f32", "v_add_f32", "v_mov_b32", "v_xor_b32", "v_lshlrev_b32", "v_max_f32",
                     "v_rcp_f32", "v_sqrt_f32", "v_cndmask_b32", "v_mul_f32 -> v_add_f32 (dependent pair)", "v_fma_f32, one dependent chain",
                     "v_mul_f32, one dependent chain", "v_mul_f32 literal", "v_mul_f32 sgpr", "v_fma_f32 2 sgprs",
                     "v_cndmask_b32 sgpr-pair mask", "v_cmp_lt_f32 -> vcc", "v_cmp_lt_f32 -> v_cndmask_b32 (dependent pair)", "v_bfi_b32",
                     "v_and_b32", "mix 3 v_mul + 1 v_cndmask", "mix 3 v_mul + 1 v_max", "mix 4 v_mul", "mix 3 v_mul + 1 v_mov"]


def probe_issue(kind: int, waves_per_simd: int, iters: int = 20000):
    """(seconds of the best launch, instructions every wave issued) of the issue probe (rt_probe_issue)."""
    sec, n = ctypes.c_double(0.0), ctypes.c_double(0.0)
    _check(tools_lib().rt_probe_issue(kind, waves_per_simd, iters, ctypes.byref(sec), ctypes.byref(n)), "rt_probe_issue", tools_lib())
    return sec.value, n.value


# rt_split_probe's out[] layout (the RT_PROBE_* enum of include/rtcuda_amd.h)
PROBE_FIELDS = (["rounds", "closest_rays", "any_rays", "s_advance_round0", "s_advance", "s_trace_pool"]
                + [f"s_trace_closest_w{w}" for w in (8, 6, 5, 4)] + [f"s_trace_any_w{w}" for w in (8, 6, 5, 4)]
                + [f"trace_blocks_per_cu_w{w}" for w in (8, 6, 5, 4)]
                + [f"shades_{k}" for k in ("matte", "mirror", "glass")] + [f"s_shade_{k}" for k in ("matte", "mirror", "glass")])


def split_probe(scene: "Scene", camera: np.ndarray, width: int, height: int, spp: int, target_rays: int,
                max_bounces: int = 10, seed: int = 1) -> dict:
    """Trace-only and shade-only rates on rays / shading records dumped from the round pipeline (rt_split_probe)."""
    cam = np.ascontiguousarray(camera, np.float32)
    out = np.zeros(len(PROBE_FIELDS), np.float64)
    if scene.L is not tools_lib():
        raise RtError("split_probe: the scene must be created with library=tools_lib()")
    _check(tools_lib().rt_split_probe(scene.h, _p(cam), width, height, spp, max_bounces, seed, target_rays, _p(out), len(out)),
           "rt_split_probe", tools_lib())
    return dict(zip(PROBE_FIELDS, out.tolist()))


# rt_shade_table: words per row in / out, by function id (include/rtcuda_amd_tools.h: the reference pins' layouts, with the
# two uniforms of sample_f and uniform_sample_sphere replaced by the six words of an XORWOW state, and again_draws added)
SHADE_TABLE_WORDS_IN = {1: 17, 2: 14, 6: 16, 7: 6, 8: 2, 9: 9, 10: 6, 11: 8, 12: 6, 13: 14}
SHADE_TABLE_WORDS_OUT = {1: 12, 2: 5, 6: 4, 7: 3, 8: 1, 9: 1, 10: 3, 11: 3, 12: 4, 13: 6}
SHADE_RECORD_IN, SHADE_RECORD_OUT, SHADE_UNWRITTEN = 22, 30, 0xFFFFFFFF


def shade_table(func: int, rows: np.ndarray, fill: int = 0) -> np.ndarray:
    """The product's shading function `func` on every row of `rows` ((n, words in) uint32), one lane per row (rt_shade_table)
    -> (n, words out) uint32.  Words no lane writes come back as `fill`."""
    rows = np.ascontiguousarray(rows, np.uint32)
    if func in SHADE_TABLE_WORDS_IN and (rows.ndim != 2 or rows.shape[1] != SHADE_TABLE_WORDS_IN[func]):
        raise RtError(f"shade_table: function {func} takes rows of {SHADE_TABLE_WORDS_IN[func]} words, got {rows.shape}")
    out = np.full((rows.shape[0], SHADE_TABLE_WORDS_OUT.get(func, 1)), fill, np.uint32)
    _check(tools_lib().rt_shade_table(int(func), rows.shape[0], _p(rows), _p(out)), "rt_shade_table", tools_lib())
    return out


def shade_records(scene: "Scene", records: np.ndarray, max_bounces: int, lds_tables: bool) -> np.ndarray:
    """The product's init() + mat() on path states ((n, 22) uint32; rt_shade_records) -> (n, 30) uint32."""
    if scene.L is not tools_lib():
        raise RtError("shade_records: the scene must be created with library=tools_lib()")
    records = np.ascontiguousarray(records, np.uint32)
    if records.ndim != 2 or records.shape[1] != SHADE_RECORD_IN:
        raise RtError(f"shade_records: records must have shape (n, {SHADE_RECORD_IN}), got {records.shape}")
    out = np.zeros((records.shape[0], SHADE_RECORD_OUT), np.uint32)
    _check(tools_lib().rt_shade_records(scene.h, int(max_bounces), int(bool(lds_tables)), records.shape[0], _p(records), _p(out)),
           "rt_shade_records", tools_lib())
    return out


def render(width: int, height: int, num_samples: int, max_bounces: int, camera: np.ndarray, scene: Scene,
           seed: int = 1):
    """Same argument order as the reference's ``render()`` (render.cuh:366-367); returns the framebuffer."""
    img, _ = scene.render(camera, width, height, num_samples, max_bounces, seed)
    return img
