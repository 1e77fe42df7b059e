#!/usr/bin/env python3
"""What a keyed ray-table frame costs (rt_render_rays_keyed_fixed_device) next to the paths it joins.

1920 x 1080 x 16 pinhole rays of the default view, made with torch on the device (0.8 GB of table: 24 B per camera ray,
d_pixel = NULL), on full_bsdf (C2), all in one process.  One warm-up of each, then REPS repetitions in turn; wall time around
the synchronous call(s), the sum buffer zeroed outside the timed region.

  a  keyed            rt_render_rays_keyed_fixed_device, the table in one call
  b  keyed_8_chunks   the same table in 8 contiguous chunk calls (dist.ray_chunk; key_first = the chunk's first row) into ONE
                      buffer -- what streaming a table through a smaller buffer, or a progressive render, pays per call
  c  camera_per_sample  rt_render_shard_fixed(RT_FLAG_RNG_PER_SAMPLE) on the same frame: the camera path of the same streams
  d  table            rt_render_rays_fixed_device on the same table: the slot-stream table path

  median ms and Msamples/s over the repetitions; `spread` = (max - min) / median; ratios a/c, b/a, a/d of Msamples/s.

  python tools/render_rays_keyed_time.py --out profiles/render_rays_keyed_time.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from render_rays_time import pinhole_rays  # noqa: E402  (tools/, the script's own directory)

W_PX, H_PX, SPP, REPS, CHUNKS = 1920, 1080, 16, 7, 8


def measure():
    import torch
    from rtcuda_amd import api, dist, scenes
    sc = api.Scene(scenes.cornell_bunny("full_bsdf"))
    cam = api.make_camera(aspect=W_PX / H_PX)
    o, d = pinhole_rays(torch, cam, W_PX, H_PX, SPP, 1)
    n, npix = o.shape[0], W_PX * H_PX
    acc = torch.zeros((npix, 3), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    chunks = [dist.ray_chunk(r, CHUNKS, n) for r in range(CHUNKS)]

    def keyed():
        return sc.render_rays_keyed_device(o.data_ptr(), d.data_ptr(), 0, n, npix, acc.data_ptr(), rays_per_pixel=SPP, fixed=True, stream=stream)

    def keyed_chunks():
        tot = None
        for first, count in chunks:
            st = sc.render_rays_keyed_device(o.data_ptr() + 12 * first, d.data_ptr() + 12 * first, 0, count, npix, acc.data_ptr(),
                                             rays_per_pixel=SPP, key_first=first, fixed=True, stream=stream)
            if tot is None:
                tot = dict(st)
            else:
                for k in ("camera_rays", "shade_events", "seconds_trace"):
                    tot[k] += st[k]
        return tot

    def camera():
        return sc.render_shard_fixed(cam, W_PX, H_PX, SPP, 0, 1, acc.data_ptr(), flags=api.FLAG_RNG_PER_SAMPLE, stream=stream)

    def table():
        return sc.render_rays_device(o.data_ptr(), d.data_ptr(), 0, n, npix, acc.data_ptr(), rays_per_pixel=SPP, fixed=True, stream=stream)

    calls = (("keyed", keyed), ("keyed_8_chunks", keyed_chunks), ("camera_per_sample", camera), ("table", table))
    times = {name: [] for name, _ in calls}
    stats, sums = {}, {}
    for rep in range(REPS + 1):
        for name, call in calls:
            acc.zero_()
            torch.cuda.synchronize()
            t = time.perf_counter()
            stats[name] = call()
            torch.cuda.synchronize()
            if rep > 0:
                times[name].append(time.perf_counter() - t)
            elif name.startswith("keyed"):
                sums[name] = acc.clone()
    out = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "frame": f"full_bsdf {W_PX}x{H_PX}x{SPP}",
           "camera_rays": n, "table_bytes": 24 * n, "reps": REPS, "chunks": CHUNKS,
           "chunked_sums_equal_one_call": bool(torch.equal(sums["keyed"], sums["keyed_8_chunks"]))}
    for name in times:
        med = statistics.median(times[name])
        out[name] = {"ms": [round(1e3 * t, 3) for t in times[name]], "median_ms": round(1e3 * med, 3), "Msamples_s": round(n / med / 1e6, 1),
                     "spread": round((max(times[name]) - min(times[name])) / med, 4),
                     "kernel_ms": round(1e3 * stats[name]["seconds_trace"], 3), "shade_events": stats[name]["shade_events"]}
    rate = {k: out[k]["Msamples_s"] for k in times}
    out["ratio_a_over_c_keyed_over_camera_per_sample"] = round(rate["keyed"] / rate["camera_per_sample"], 4)
    out["ratio_b_over_a_8_chunks_over_one_call"] = round(rate["keyed_8_chunks"] / rate["keyed"], 4)
    out["ratio_a_over_d_keyed_over_table"] = round(rate["keyed"] / rate["table"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    res = measure()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
