#!/usr/bin/env python3
"""What a counted frame costs (rt_render_counts_fixed) next to the paths it joins.

full_bsdf (C2) at 1920 x 1080, the default view, all in one process.  One warm-up of each, then REPS repetitions in turn; wall
time around the synchronous call, the sum buffer zeroed outside the timed region.

 at sample_stride 16:
  a  counts_uniform      rt_render_counts_fixed with every count 16 (d_first NULL, d_samples given)
  b  camera_per_sample   rt_render_shard_fixed(RT_FLAG_RNG_PER_SAMPLE) on the same frame: the camera path of the same samples
  c  keyed               rt_render_rays_keyed_fixed_device on the table of the same rays (24 B per camera ray, made with torch)
  d  counts_allocated    counts from rt_sample_allocate (min_count 1, max_count 16, budget 8 * pixels) on the two-half variance
                         of a rendered 4 + 4 spp frame: weight = sqrt(|mean_a - mean_b|^2 / 4) / (mean + 0.05) + 0.1 on luminance,
                         composed in torch
  e  camera_8spp         rt_render_shard_fixed(RT_FLAG_RNG_PER_SAMPLE) at 8 spp: as many samples as d places, evenly
 at 1 spp (what the prepass weighs against):
  f  counts_1spp         rt_render_counts_fixed, every count 1, sample_stride 1
  g  camera_1spp         rt_render_shard_fixed(RT_FLAG_RNG_PER_SAMPLE) at 1 spp
  h  counts_zero         rt_render_counts_fixed with every count 0: the call returns after the prepass's first two kernels and the
                         read-back of the total (it leaves out the third kernel, which writes the prefix sum)

  median ms and Msamples/s over the repetitions; `spread` = (max - min) / median; ratios of Msamples/s a/b, c/b, a/c, d/e, and
  h's median over g's.

  python tools/render_counts_time.py --out profiles/render_counts_time.json
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

W_PX, H_PX, SPP, REPS = 1920, 1080, 16, 7


def measure():
    import torch
    from rtcuda_amd import api, scenes
    sc = api.Scene(scenes.cornell_bunny("full_bsdf"))
    cam = api.make_camera(aspect=W_PX / H_PX)
    npix = W_PX * H_PX
    acc = torch.zeros((npix, 3), dtype=torch.int64, device="cuda")
    samples = torch.zeros((npix,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def counts_of(value):
        return torch.full((npix,), value, dtype=torch.int32, device="cuda")

    def camera(spp):
        return lambda: sc.render_shard_fixed(cam, W_PX, H_PX, spp, 0, 1, acc.data_ptr(), flags=api.FLAG_RNG_PER_SAMPLE, stream=stream)

    def counted(count, stride):
        return lambda: sc.render_counts(cam, W_PX, H_PX, stride, count, samples=samples, out=acc)[1]

    # the allocated map: two 4-spp halves of the same per-sample frame (samples 0 .. 3 and 4 .. 7), their two-half variance
    half = [sc.render_counts(cam, W_PX, H_PX, SPP, counts_of(4), first=counts_of(f))[0] for f in (0, 4)]
    lum = [(h.to(torch.float64) * (2.0 ** -30 / 4)) @ torch.tensor([0.2126, 0.7152, 0.0722], dtype=torch.float64, device="cuda") for h in half]
    weight = (torch.sqrt((lum[0] - lum[1]) ** 2 / 4) / ((lum[0] + lum[1]) / 2 + 0.05) + 0.1).to(torch.float32).contiguous()
    allocated, placed = api.sample_allocate(weight, 1, SPP, 8 * npix)
    del half, lum

    o, d = pinhole_rays(torch, cam, W_PX, H_PX, SPP, 1)
    n16 = o.shape[0]

    def keyed():
        return sc.render_rays_keyed_device(o.data_ptr(), d.data_ptr(), 0, n16, npix, acc.data_ptr(), rays_per_pixel=SPP, fixed=True, stream=stream)

    calls = (("counts_uniform", counted(counts_of(SPP), SPP), n16), ("camera_per_sample", camera(SPP), n16), ("keyed", keyed, n16),
             ("counts_allocated", counted(allocated, SPP), placed), ("camera_8spp", camera(8), 8 * npix),
             ("counts_1spp", counted(counts_of(1), 1), npix), ("camera_1spp", camera(1), npix), ("counts_zero", counted(counts_of(0), SPP), 0))
    times = {name: [] for name, _, _ in calls}
    stats, sums = {}, {}
    for rep in range(REPS + 1):
        for name, call, _ in calls:
            acc.zero_()
            torch.cuda.synchronize()
            t = time.perf_counter()
            stats[name] = call()
            torch.cuda.synchronize()
            if rep > 0:
                times[name].append(time.perf_counter() - t)
            elif name in ("counts_uniform", "camera_per_sample"):
                sums[name] = acc.clone()
    hist = torch.bincount(allocated.to(torch.int64), minlength=SPP + 1).tolist()
    out = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "frame": f"full_bsdf {W_PX}x{H_PX}", "sample_stride": SPP, "reps": REPS,
           "uniform_sums_equal_camera_path": bool(torch.equal(sums["counts_uniform"], sums["camera_per_sample"])),
           "allocated": {"budget": 8 * npix, "placed": placed, "min_count": 1, "max_count": SPP, "pixels_per_count": hist}}
    for name, _, n in calls:
        med = statistics.median(times[name])
        out[name] = {"ms": [round(1e3 * t, 3) for t in times[name]], "median_ms": round(1e3 * med, 3), "camera_rays": n,
                     "Msamples_s": round(n / med / 1e6, 1), "spread": round((max(times[name]) - min(times[name])) / med, 4),
                     "kernel_ms": round(1e3 * stats[name]["seconds_trace"], 3), "shade_events": stats[name]["shade_events"]}
    rate = {k: out[k]["Msamples_s"] for k in times}
    out["ratio_a_over_b_counts_over_camera_per_sample"] = round(rate["counts_uniform"] / rate["camera_per_sample"], 4)
    out["ratio_c_over_b_keyed_over_camera_per_sample"] = round(rate["keyed"] / rate["camera_per_sample"], 4)
    out["ratio_a_over_c_counts_over_keyed"] = round(rate["counts_uniform"] / rate["keyed"], 4)
    out["ratio_d_over_e_allocated_over_uniform_8spp"] = round(rate["counts_allocated"] / rate["camera_8spp"], 4)
    out["ratio_f_over_g_counts_over_camera_1spp"] = round(rate["counts_1spp"] / rate["camera_1spp"], 4)
    out["prepass_h_ms_over_1spp_frame_g_ms"] = round(out["counts_zero"]["median_ms"] / out["camera_1spp"]["median_ms"], 4)
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
