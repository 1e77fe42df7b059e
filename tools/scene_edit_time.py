#!/usr/bin/env python3
"""What an in-place scene edit costs next to destroying the scene and creating it again -> profiles/scene_edit_time.json.

For the bunny (full-BSDF) and the four-bunnies scene, host wall clock around the synchronous calls, one process, medians of
REPS runs after a warm-up run, min and max beside them (the spread).  Every run is the edit FOLLOWED by one small default-mode
render (64 x 48 x 2), so that the rebuild of the reference's tree on the host is counted where it occurs; `*_call_ms` is the
edit alone.

  set_materials / set_lights       rt_scene_set_materials / rt_scene_set_lights with changed values
  set_triangles_device             rt_scene_set_triangles_device from tensors already on the device (deformed vertices)
  set_triangles_host               rt_scene_set_triangles from host arrays
  rebuild_device                   rt_scene_rebuild_device with the same vertices (what a count-preserving change cost before)
  recreate                         rt_scene_destroy + rt_scene_create_flags(RT_SCENE_DEVICE_BVH) from host arrays: what the
                                   library offered for any of these changes before the edit entry points
"""
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rtcuda_amd import api, scenes  # noqa: E402

REPS = int(os.environ.get("EDIT_REPS", "7"))


def deform(tris, amp):
    v = np.asarray(tris, np.float64).reshape(-1, 3)
    d = amp * np.stack([np.sin(7.0 * v[:, 1] + 1.0), np.sin(5.0 * v[:, 2] + 2.0), np.sin(6.0 * v[:, 0] + 3.0)], axis=1)
    return (v + d).astype(np.float32).reshape(-1, 9)


def timed(edit, scene_of, cam):
    """[(edit ms, edit + render ms)] of REPS runs after one warm-up run; edit(k) returns nothing or the scene to render."""
    rows = []
    for k in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        edit(k)
        t1 = time.perf_counter()
        scene_of().render(cam, 64, 48, 2)
        t2 = time.perf_counter()
        rows.append((1e3 * (t1 - t0), 1e3 * (t2 - t0)))
    return rows[1:]


def summary(name, rows):
    call, total = [r[0] for r in rows], [r[1] for r in rows]
    return {f"{name}_call_ms": round(statistics.median(call), 3), f"{name}_ms": round(statistics.median(total), 3),
            f"{name}_ms_min_max": [round(min(total), 3), round(max(total), 3)]}


def main():
    cam = api.make_camera(aspect=64 / 48)
    result = {"build_id": api.build_id(), "reps": REPS, "frame_after_each_edit": "64x48x2 default mode", "scenes": []}
    for variant in ("full_bsdf", "four_bunnies"):
        arrays = scenes.cornell_bunny(variant)
        versions = [dataclasses.replace(arrays, tris=deform(arrays.tris, 0.002 * (k + 1))) for k in range(2)]
        dev = [(torch.from_numpy(v.tris).cuda(), torch.from_numpy(np.ascontiguousarray(v.tri_material)).cuda(),
                torch.from_numpy(np.ascontiguousarray(v.tri_light)).cuda()) for v in versions]
        box = {"sc": api.Scene(arrays, device_bvh=True)}
        box["sc"].render(cam, 64, 48, 2)
        line = {"scene": variant, "tris": arrays.n_tris, "materials": len(arrays.materials), "lights": len(arrays.lights)}

        def set_materials(k):
            m = arrays.materials.copy()
            m["albedo"] *= np.float32(0.9 + 0.01 * k)
            box["sc"].set_materials(m)

        def set_lights(k):
            l = arrays.lights.copy()
            l["L"] *= np.float32(0.9 + 0.01 * k)
            box["sc"].set_lights(l)

        def set_triangles_device(k):
            t, m, l = dev[k % 2]
            box["sc"].set_triangles_tensors(t, m, l, arrays.materials, arrays.lights)

        def set_triangles_host(k):
            box["sc"].set_triangles(versions[k % 2])

        def rebuild_device(k):
            box["sc"].rebuild_device(dev[k % 2][0].data_ptr())

        def recreate(k):
            box["sc"].close()
            box["sc"] = api.Scene(versions[k % 2], device_bvh=True)

        for name, edit in (("set_materials", set_materials), ("set_lights", set_lights), ("set_triangles_device", set_triangles_device),
                           ("set_triangles_host", set_triangles_host), ("rebuild_device", rebuild_device), ("recreate", recreate)):
            line.update(summary(name, timed(edit, lambda: box["sc"], cam)))
        line["recreate_over_set_triangles_device"] = round(line["recreate_ms"] / line["set_triangles_device_ms"], 3)
        result["scenes"].append(line)
        print(json.dumps(line), flush=True)
        box["sc"].close()
    out = os.path.join(ROOT, "profiles", "scene_edit_time.json")
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
