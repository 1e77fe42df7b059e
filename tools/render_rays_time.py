#!/usr/bin/env python3
"""What rendering along a ray table costs (rt_render_rays_fixed_device) next to the camera path (rt_render_shard_fixed).

1920 x 1080 x 16 pinhole rays of the default view, made with torch on the device (0.8 GB of table: 24 B per camera ray,
d_pixel = NULL), on full_bsdf (C2); the camera path renders the same scene / size / spp in the same process.  One warm-up of
each, then REPS repetitions in turn (table, camera, table, ...); wall time around the synchronous call.

  Msamples_s           median over the repetitions, of both paths; `ratio` = table / camera; `spread` = (max - min) / median
  --variant-lib NAME   the same table measurement in a child process that loads rtcuda_amd/NAME instead (a build of
                       `make variant`, e.g. DEFS=-DRT_RAYS_NONTEMPORAL=0: the table read with ordinary loads), recorded under
                       "variant" -- the non-temporal A/B

  python tools/render_rays_time.py --variant-lib librtcuda_amd_raystemporal.so --out profiles/render_rays_time.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W_PX, H_PX, SPP, REPS = 1920, 1080, 16, 5


def pinhole_rays(torch, cam12, w, h, spp, seed):
    """Jittered pinhole rays in camera-ray order (ray c on pixel c // spp), float32 on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    cam = torch.from_numpy(cam12).cuda()
    lf, ul, hz, vt = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    n = w * h * spp
    pixel = torch.arange(n, device="cuda") // spp
    x = ((pixel % w).float() + torch.rand(n, generator=g, device="cuda")) / w
    y = ((pixel // w).float() + torch.rand(n, generator=g, device="cuda")) / h
    d = ul + x[:, None] * hz + y[:, None] * vt - lf
    d = (d / d.norm(dim=1, keepdim=True)).contiguous()
    return lf.expand(n, 3).contiguous(), d


def measure():
    import torch
    from rtcuda_amd import api, scenes
    sc = api.Scene(scenes.cornell_bunny("full_bsdf"))
    cam = api.make_camera(aspect=W_PX / H_PX)
    o, d = pinhole_rays(torch, cam, W_PX, H_PX, SPP, 1)
    n, npix = o.shape[0], W_PX * H_PX
    acc = torch.zeros((npix, 3), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def table():
        return sc.render_rays_device(o.data_ptr(), d.data_ptr(), 0, n, npix, acc.data_ptr(), rays_per_pixel=SPP, fixed=True, stream=stream)

    def camera():
        return sc.render_shard_fixed(cam, W_PX, H_PX, SPP, 0, 1, acc.data_ptr(), stream=stream)

    times = {"table": [], "camera": []}
    stats = {}
    for rep in range(REPS + 1):
        for name, call in (("table", table), ("camera", camera)):
            acc.zero_()
            torch.cuda.synchronize()
            t = time.perf_counter()
            stats[name] = call()
            torch.cuda.synchronize()
            if rep > 0:
                times[name].append(time.perf_counter() - t)
    out = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "frame": f"full_bsdf {W_PX}x{H_PX}x{SPP}",
           "camera_rays": n, "table_bytes": 24 * n, "reps": REPS}
    for name in times:
        med = statistics.median(times[name])
        out[name] = {"ms": [round(1e3 * t, 3) for t in times[name]], "Msamples_s": round(n / med / 1e6, 1),
                     "spread": round((max(times[name]) - min(times[name])) / med, 4),
                     "kernel_ms": round(1e3 * stats[name]["seconds_trace"], 3), "shade_events": stats[name]["shade_events"]}
    out["ratio_table_over_camera"] = round(out["table"]["Msamples_s"] / out["camera"]["Msamples_s"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant-lib")
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    res = measure()
    if a.child:
        print("RESULT " + json.dumps(res), flush=True)
        return
    if a.variant_lib:
        env = dict(os.environ, RT_LIB_NAME=a.variant_lib)
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=600)
        line = [l for l in child.stdout.splitlines() if l.startswith("RESULT ")]
        res["variant"] = dict(json.loads(line[0][7:]), lib=a.variant_lib) if line else {"error": child.stderr[-500:]}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
