#!/usr/bin/env python3
"""What a vertex update costs against building the scene anew (rt_scene_update vs rt_scene_create), one JSON line per scene.

  refit_ms     device time of rt_scene_update (HIP events, rt_scene_refit_info), warm, median of 7 updates
  build_s      rt_scene_build_info's build seconds of a fresh scene with the same vertices
  sah_ratio    the refit tree's surface-area cost relative to build time
  c2           (full_bsdf only) Msamples/s of a 1920x1080 frame at reduced spp on the refit scene and on the fresh one
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import dataclasses  # noqa: E402

import numpy as np  # noqa: E402

from rtcuda_amd import api, scenes  # noqa: E402
from test_scene_update_host import deform  # noqa: E402


def rate(sc, cam, w, h, spp, reps=3):
    out = []
    for _ in range(reps):
        _, st = sc.render(cam, w, h, spp)
        out.append(st["camera_rays"] / st["seconds_render"] / 1e6)
    return statistics.median(out)


def main():
    w, h, spp = 1920, 1080, int(os.environ.get("REFIT_SPP", "64"))
    for variant in ("full_bsdf", "four_bunnies"):
        arrays = scenes.cornell_bunny(variant)
        new = deform(arrays.tris, amp=0.005)
        a = api.Scene(arrays)
        times = []
        for k in range(8):
            a.update(new if k % 2 == 0 else arrays.tris)
            times.append(a.refit_info()["seconds_last"])
        a.update(new)
        t0 = time.perf_counter()
        a.update(new)
        wall = time.perf_counter() - t0
        info = a.refit_info()
        b = api.Scene(dataclasses.replace(arrays, tris=new))
        line = {"scene": variant, "tris": arrays.n_tris, "refit_ms": round(1e3 * statistics.median(times[1:]), 4),
                "refit_wall_ms": round(1e3 * wall, 3), "build_s": round(b.info()["build_seconds"], 4),
                "sah_ratio": round(info["sah_ratio"], 5)}
        if variant == "full_bsdf":
            cam = api.make_camera(aspect=w / h)
            rate(a, cam, 256, 144, 4, reps=1)  # (warm-up: contexts, RNG states, the reference's tree of the new vertices)
            rate(b, cam, 256, 144, 4, reps=1)
            line["c2_spp"] = spp
            line["c2_refit_Msamples_s"] = round(rate(a, cam, w, h, spp), 1)
            line["c2_fresh_Msamples_s"] = round(rate(b, cam, w, h, spp), 1)
        print(json.dumps(line), flush=True)
        a.close()
        b.close()


if __name__ == "__main__":
    main()
