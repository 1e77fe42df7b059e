#!/usr/bin/env python3
"""What the denoiser costs (rt_denoise_fixed), against the frame it cleans and against what a caller could do before it existed.

C2 (full_bsdf) at 1920 x 1080, 16 spp, warm, medians of 7 with min and max, HIP events on the current stream, one process:

  call            api.denoise with the default parameters, scratch and output allocated before the clock
  by_passes       the same call with passes = 0 .. 8 (the other parameters the defaults'): passes = 0 is k_dn_prepare + k_dn_finish
  pass_kernel_ms  THE PASS KERNELS THEMSELVES, per stride and per form: rt_denoise_pass_time of the lab library launches one
                  pass (direct = k_atrous, lds = k_atrous_lds) on the prepared frame and times every launch with HIP events;
                  the two forms alternate launch blocks within one process, 7 timed launches each after a warm-up.  `kept` is
                  the faster form per stride -- what dn_lds_wins in rt_host_denoise.inc must say
  bytes           per pass, from the shapes: what HBM must move (one {u, z} and one {n} record read, one {u, z} written per
                  pixel) and what the 25 taps ask of the caches (two 16-byte records each, less the image edge), with the
                  rates the direct kernel's time makes of them
  torch           the same filter composed from torch ops alone in float32 (resolve, shifted slices, torch.exp): it calls no
                  entry point of this library, so it is what a user of the parent commit's library can write; `max_abs_diff`
                  against the call
  beauty          the per-sample beauty frame of the same size (rt_render_shard_fixed, RT_FLAG_RNG_PER_SAMPLE, 10 bounces),
                  re-measured here: rt_stats.seconds_render

  python tools/denoise_time.py [--out profiles/denoise_time.json]
  python tools/denoise_time.py --once FORM   two calls with passes = 8 in one form (1 direct, 2 lds; the RT_DENOISE_FORM knob)
      and nothing else -- what a counter run profiles:
      rocprofv3 --pmc <counters> --output-format csv -d DIR -- python tools/denoise_time.py --once 1     (no tracing with it)
  python tools/denoise_time.py --merge-pmc DIR/**/counter_collection.csv ... [--out ...]
      no GPU: adds the counters of such runs to the result file as `pmc`, per kernel and per stride (the n-th dispatch of a pass
      kernel in a call is stride 2^n), with what follows from them and from pass_kernel_ms: T_lane_ops_per_s = SQ_INSTS_VALU *
      64 / time, its fraction of the 78.6 T lane-op/s fp32 vector peak and of the 62.9 T the chip sustained on independent
      v_fma_f32 (profiles/r02_valu_calibration.json, 8 waves per SIMD); l2_hit_rate = TCC_HIT_sum / (TCC_HIT_sum + TCC_MISS_sum)
"""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

W, H, SPP, SEED = 1920, 1080, 16, 1
REPS = 7
KERNEL = (0.0625, 0.25, 0.375, 0.25, 0.0625)


def _summary(ms):
    return {"ms": round(statistics.median(ms), 4), "min_max": [round(min(ms), 4), round(max(ms), 4)]}


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def _median_of(torch, fn):
    ms = []
    for rep in range(REPS + 1):  # (the first repetition warms up and is dropped)
        t, r = _timed(torch, fn)
        if rep:
            ms.append(t)
    return ms, r


def torch_denoise(torch, api, beauty, spp, aov, aov_spp, w, h, prm):
    """The filter of rt_denoise_fixed from torch ops alone, float32 (not bit-exact: torch.exp, fused kernels)."""
    sa = (aov.double() * (1.0 / 1073741824.0)).float()
    hits = aov[:, 10]
    f = sa * np.float32(1.0 / aov_spp)
    c = (beauty.double() * (1.0 / 1073741824.0)).float() * np.float32(1.0 / spp)
    a, n, e = f[:, 0:3], f[:, 3:6].reshape(h, w, 3), f[:, 6:9]
    z = torch.where(hits > 0, sa[:, 9] / hits.clamp(min=1).float(), torch.zeros_like(sa[:, 9])).reshape(h, w)
    d = torch.clamp(a, min=2.0 ** -10)
    u = (torch.clamp(c - e, min=0) / d).reshape(h, w, 3)
    kz = 1.0 / (prm["sigma_depth"] ** 2)
    for i in range(prm["passes"]):
        s, kc = 1 << i, 4.0 ** i / (prm["sigma_color"] ** 2)
        sw = torch.zeros((h, w), dtype=torch.float32, device=u.device)
        su = torch.zeros_like(u)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = s * dy, s * dx
                y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                hk = KERNEL[dx + 2] * KERNEL[dy + 2]
                if dx == 0 and dy == 0:
                    wt = torch.full_like(sw[P], hk)
                else:
                    x = ((u[Q] - u[P]) ** 2).sum(2) * kc + (z[Q] - z[P]) ** 2 * kz
                    wn = torch.clamp((n[P] * n[Q]).sum(2), 0, 1)
                    for _ in range(prm["normal_power_log2"]):
                        wn = wn * wn
                    wt = hk * torch.exp(-x) * wn
                sw[P] += wt
                su[P] += wt[..., None] * u[Q]
        u = su / sw[..., None]
    return u.reshape(-1, 3) * d + e


def pass_bytes(w, h, stride):
    taps = sum(max(0, w - abs(stride * dx)) * max(0, h - abs(stride * dy)) for dy in range(-2, 3) for dx in range(-2, 3))
    return {"hbm": w * h * 48, "taps": taps * 32}


def pmc_rows(paths, res):
    """{kernel: {stride: {counter: mean per dispatch, ..., derived}}} of rocprofv3 counter_collection.csv files of --once runs."""
    acc = {}
    for path in paths:
        seen = {}
        with open(path) as fh:
            rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Dispatch_Id"]))
        for row in rows:
            name = row.get("Kernel_Name", "").split("(")[0]
            if not name.startswith("k_atrous"):
                continue
            order = seen.setdefault(name, {})
            k = order.setdefault(row["Dispatch_Id"], len(order))  # (the n-th dispatch of this kernel in the run)
            acc.setdefault(name, {}).setdefault(1 << (k % 8), {}).setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
    out = {}
    for name, per_stride in acc.items():
        form = "lds" if name.endswith("_lds") else "direct"
        for stride, ctr in sorted(per_stride.items()):
            m = {k: round(sum(v) / len(v), 1) for k, v in sorted(ctr.items())}
            d = dict(m, dispatches=len(next(iter(ctr.values()))))
            ms = res["pass_kernel_ms"][form][stride.bit_length() - 1]["ms"]
            if "SQ_INSTS_VALU" in m and "SQ_WAVES" in m:
                rate = m["SQ_INSTS_VALU"] * 64 / (ms * 1e-3) / 1e12
                d.update(kernel_ms=ms, valu_instructions_per_wave=round(m["SQ_INSTS_VALU"] / m["SQ_WAVES"], 1), T_lane_ops_per_s=round(rate, 2),
                         of_fp32_vector_peak=round(rate / 78.6, 3), of_calibrated_rate=round(rate / 62.9, 3))
            if "TCC_HIT_sum" in m and "TCC_MISS_sum" in m:
                d["l2_hit_rate"] = round(m["TCC_HIT_sum"] / (m["TCC_HIT_sum"] + m["TCC_MISS_sum"]), 4)
            out.setdefault(form, {})[str(stride)] = d
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_time.json"))
    ap.add_argument("--merge-pmc", nargs="+")
    ap.add_argument("--once", type=int, choices=[1, 2], metavar="FORM")
    ap.add_argument("--size", nargs=2, type=int, default=[W, H], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.merge_pmc:
        res = json.load(open(a.out))
        res["pmc"] = dict(pmc_rows(a.merge_pmc, res), note="%d x %d calls with passes = 8 in one form, two calls per run" % tuple(res["frame"][:2]))
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        return
    if a.once:
        os.environ["RTCUDA_EXPERIMENTAL"], os.environ["RT_DENOISE_FORM"] = "1", str(a.once)
    import torch
    from rtcuda_amd import api, scenes
    assert torch.cuda.is_available(), "denoise_time.py measures on a GPU"
    w, h = a.size
    scene = api.Scene(scenes.cornell_bunny("full_bsdf"))
    cam = api.make_camera(aspect=w / h)
    beauty = torch.zeros((w * h, 3), dtype=torch.int64, device="cuda")
    beauty_ms = []
    for rep in range(1 if a.once else REPS + 1):
        beauty.zero_()
        st = scene.render_shard_fixed(cam, w, h, SPP, 0, 1, beauty.data_ptr(), seed=SEED, flags=api.FLAG_RNG_PER_SAMPLE)
        if rep:
            beauty_ms.append(st["seconds_render"] * 1e3)
    aov, _, _ = scene.render_aov(cam, w, h, SPP, seed=SEED, flags=api.FLAG_WATERTIGHT)
    scratch = torch.empty(api.denoise_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    out = torch.empty((w * h, 3), dtype=torch.float32, device="cuda")
    prm = api.denoise_default_params()
    if a.once:
        for _ in range(2):
            api.denoise(beauty, SPP, aov, SPP, w, h, passes=8, scratch=scratch, out=out)
        torch.cuda.synchronize()
        print("once ok", float(out.mean()), flush=True)
        return
    res = {"scene": "full_bsdf", "frame": [w, h, SPP], "reps": REPS, "build_id": api.build_id(), "device": torch.cuda.get_device_name(0),
           "params": prm, "forms": ["direct", "lds"], "tile": [32, 8]}
    ms, _ = _median_of(torch, lambda: api.denoise(beauty, SPP, aov, SPP, w, h, scratch=scratch, out=out))
    res["call"] = _summary(ms)
    ours = out.clone()
    by = []
    for p in range(9):
        ms, _ = _median_of(torch, lambda: api.denoise(beauty, SPP, aov, SPP, w, h, passes=p, scratch=scratch, out=out))
        by.append(_summary(ms))
    res["by_passes"] = by
    # the pass kernels themselves: the scratch of a passes = 0 call holds the prepared frame
    api.denoise(beauty, SPP, aov, SPP, w, h, passes=0, scratch=scratch, out=out)
    T = api.tools_lib()
    per = {"direct": [[] for _ in range(8)], "lds": [[] for _ in range(8)]}
    buf = (ctypes.c_float * 4)()
    for rnd in range(4):  # (rounds of 4 launches per form and stride, the forms taking turns; the first round warms up)
        for i in range(8):
            for form, name in ((1, "direct"), (2, "lds")):
                rc = T.rt_denoise_pass_time(ctypes.c_void_p(scratch.data_ptr()), w, h, 1 << i, form, prm["sigma_color"], prm["sigma_depth"],
                                            prm["normal_power_log2"], 4, buf)
                assert rc == 0, T.rt_last_error().decode()
                if rnd:
                    per[name][i] += list(buf)
    res["pass_kernel_ms"] = {k: [_summary(v[:REPS]) for v in per[k]] for k in per}
    res["kept"] = ["lds" if per["lds"][i] and statistics.median(per["lds"][i][:REPS]) < statistics.median(per["direct"][i][:REPS]) else "direct"
                   for i in range(8)]
    res["bytes"] = []
    for i in range(8):
        b = pass_bytes(w, h, 1 << i)
        sec = res["pass_kernel_ms"]["direct"][i]["ms"] * 1e-3
        res["bytes"].append(dict(b, stride=1 << i, hbm_TBps=round(b["hbm"] / sec / 1e12, 3), taps_TBps=round(b["taps"] / sec / 1e12, 3)))
    ms, theirs = _median_of(torch, lambda: torch_denoise(torch, api, beauty, SPP, aov, SPP, w, h, prm))
    res["torch"] = dict(_summary(ms), max_abs_diff=float((theirs - ours).abs().max()))
    res["torch_over_call"] = round(res["torch"]["ms"] / res["call"]["ms"], 2)
    res["beauty_per_sample_10_bounces"] = {"render": _summary(beauty_ms)}
    res["call_over_beauty"] = round(res["call"]["ms"] / res["beauty_per_sample_10_bounces"]["render"]["ms"], 4)
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
