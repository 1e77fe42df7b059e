#!/usr/bin/env python3
"""What a device BVH build (PLOC: rt_scene_rebuild, RT_SCENE_DEVICE_BVH) costs and gives against the host SAH build, one JSON
line per scene.

  device_build_ms   device time of the build (HIP events, rt_scene_build_info), warm, median of 5 rebuilds
  rebuild_wall_ms   wall time of one rt_scene_rebuild (build + re-emitting the scene for the new leaf order)
  host_build_s      rt_scene_build_info's seconds of the host SAH build of the same scene
  iterations        clustering iterations of the build (the host twin's count: the device makes the same ones)
  sah_ratio         the device tree's surface-area cost over the host tree's
  Msamples_s        1920 x 1080 frame at REBUILD_SPP spp on the device-built tree and on the host-built one, in turns
"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rtcuda_amd import api, scenes  # noqa: E402


def twin(tris):
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    L.rt_ploc_check.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                ctypes.c_void_p]
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    out = np.zeros(8, np.int64)
    assert L.rt_ploc_check(t.ctypes.data, t.shape[0], 0, None, None, 1, out.ctypes.data) == 0
    return {"iterations": int(out[6]), "sah_ratio": round(float(out[4] / out[5]), 4)}


def rate(sc, cam, w, h, spp):
    _, st = sc.render(cam, w, h, spp)
    return st["camera_rays"] / st["seconds_render"] / 1e6


def main():
    w, h, spp = 1920, 1080, int(os.environ.get("REBUILD_SPP", "64"))
    for variant, tag in (("full_bsdf", "c2"), ("four_bunnies", "c4")):
        arrays = scenes.cornell_bunny(variant)
        a = api.Scene(arrays, device_bvh=True)
        b = api.Scene(arrays)
        times = []
        for _ in range(6):
            a.rebuild()
            times.append(a.info()["build_seconds"])
        t0 = time.perf_counter()
        a.rebuild()
        wall = time.perf_counter() - t0
        line = {"scene": variant, "tris": arrays.n_tris, "device_build_ms": round(1e3 * statistics.median(times[1:]), 3),
                "rebuild_wall_ms": round(1e3 * wall, 2), "host_build_s": round(b.info()["build_seconds"], 4),
                "depth_device": a.info()["max_depth"], "depth_host": b.info()["max_depth"]}
        line.update(twin(arrays.tris))
        cam = api.make_camera(aspect=w / h)
        rate(a, cam, 256, 144, 4)  # (warm-up: contexts, RNG states, the reference's tree)
        rate(b, cam, 256, 144, 4)
        ra, rb = [], []
        for _ in range(3):  # alternating, one process
            ra.append(rate(a, cam, w, h, spp))
            rb.append(rate(b, cam, w, h, spp))
        line[f"{tag}_spp"] = spp
        line[f"{tag}_device_tree_Msamples_s"] = round(statistics.median(ra), 1)
        line[f"{tag}_host_tree_Msamples_s"] = round(statistics.median(rb), 1)
        line[f"{tag}_frame_time_ratio"] = round(statistics.median(rb) / statistics.median(ra), 4)
        print(json.dumps(line), flush=True)
        a.close()
        b.close()


if __name__ == "__main__":
    main()
