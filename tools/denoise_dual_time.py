#!/usr/bin/env python3
"""What the dual-buffer denoiser costs (rt_denoise_dual_fixed), against rt_denoise_fixed and against the frame it cleans.

C2 (full_bsdf) at 1920 x 1080, 16 spp, warm, medians of 7 with min and max, HIP events on the current stream, one process:

  call            api.denoise_dual with the default parameters on the two 8-spp half frames, scratch and output allocated before
                  the clock
  fixed_call      api.denoise (rt_denoise_fixed, unchanged by this feature) on the summed frame with ITS other defaults and the
                  dual defaults' pass count: the comparison, in the same process, the two calls alternating
  by_passes       both calls with passes = 0 .. 8
  pass_kernel_ms  THE PASS KERNELS THEMSELVES per stride: rt_denoise_dual_pass_time of the lab library launches one pass in one
                  form (direct = k_atrous_var, lds = k_atrous_var_lds) with one placement of the 3 x 3 variance prefilter
                  (inline = in the pass, prepass = k_dn_var_blur before it, inside the timed interval) and times every launch
                  with HIP events; `fixed` holds rt_denoise_pass_time's k_atrous / k_atrous_lds of the same stride.  All take turns
                  in launch blocks within one process, 7 timed launches each after a warm-up.  `kept_g` is the placement kept
                  per form and stride (prepass where its median beats every inline launch, inline otherwise), `kept` the faster form per stride at its kept placement -- what dn_dual_inline_g_wins and
                  dn_dual_lds_wins in rt_host_denoise.inc must say.  `dual_over_fixed` is the kept dual pass over the faster
                  rt_denoise_fixed pass of that stride
  halves          what the dual input costs the renderer: two rt_render_shard_fixed calls of shard (r, 2) against the one
                  whole-frame call of the same 16 spp (RT_FLAG_RNG_PER_SAMPLE, rt_stats.seconds_render), alternating

  python tools/denoise_dual_time.py [--out profiles/denoise_dual_time.json]
  python tools/denoise_dual_time.py --once FORM G   two calls of each denoiser with passes = 8 and nothing else, the dual passes
      in one form and placement (0 0: the kept ones) -- what a counter run profiles:
      rocprofv3 --pmc <counters> --output-format csv -d DIR -- python tools/denoise_dual_time.py --once 0 0   (no tracing with it)
  python tools/denoise_dual_time.py --merge-pmc DIR/**/counter_collection.csv ... [--out ...]
      no GPU: adds the counters of such runs to the result file as `pmc`: per pass kernel and stride (the n-th dispatch of a
      kernel family in a call is stride 2^n) the mean of each counter per dispatch, and per wave where SQ_WAVES was collected
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, SPP, SEED = 1920, 1080, 16, 1
REPS = 7


def _summary(ms):
    return {"ms": round(statistics.median(ms), 4), "min_max": [round(min(ms), 4), round(max(ms), 4)]}


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _alternate(torch, fns):
    """Medians of REPS of each of `fns`, taking turns; the first round warms up and is dropped."""
    ms = [[] for _ in fns]
    for rep in range(REPS + 1):
        for k, fn in enumerate(fns):
            t = _timed(torch, fn)
            if rep:
                ms[k].append(t)
    return [_summary(m) for m in ms]


def pmc_rows(paths):
    """{kernel: {stride: {counter: mean per dispatch, "<counter>_per_wave": ...}}} of rocprofv3 counter_collection.csv files."""
    import csv
    acc = {}
    for path in paths:
        with open(path) as fh:
            rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Dispatch_Id"]))
        seen = {}
        for row in rows:
            name = row.get("Kernel_Name", "").split("(")[0].replace("void ", "")
            if not name.startswith("k_atrous"):
                continue
            family = "dual" if name.startswith("k_atrous_var") else "fixed"
            order = seen.setdefault(family, {})
            k = order.setdefault(row["Dispatch_Id"], len(order))  # (the n-th pass of this denoiser in the run)
            acc.setdefault(name, {}).setdefault(1 << (k % 8), {}).setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
    out = {}
    for name, per_stride in sorted(acc.items()):
        for stride, ctr in sorted(per_stride.items()):
            m = {k: round(sum(v) / len(v), 1) for k, v in sorted(ctr.items())}
            if m.get("SQ_WAVES"):
                m.update({k + "_per_wave": round(v / m["SQ_WAVES"], 1) for k, v in list(m.items()) if k != "SQ_WAVES"})
            out.setdefault(name, {})[str(stride)] = m
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_dual_time.json"))
    ap.add_argument("--once", nargs=2, type=int, metavar=("FORM", "G"))
    ap.add_argument("--merge-pmc", nargs="+")
    ap.add_argument("--size", nargs=2, type=int, default=[W, H], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.merge_pmc:
        res = json.load(open(a.out))
        res["pmc"] = pmc_rows(a.merge_pmc)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        return
    if a.once and a.once[0]:
        os.environ["RTCUDA_EXPERIMENTAL"] = "1"
        os.environ["RT_DENOISE_FORM"], os.environ["RT_DENOISE_DUAL_G"] = str(a.once[0]), str(a.once[1])
    import torch
    from rtcuda_amd import api, scenes
    assert torch.cuda.is_available(), "denoise_dual_time.py measures on a GPU"
    w, h = a.size
    scene = api.Scene(scenes.cornell_bunny("full_bsdf"))
    cam = api.make_camera(aspect=w / h)
    bufs = {k: torch.zeros((w * h, 3), dtype=torch.int64, device="cuda") for k in ("a", "b", "whole")}

    def shard(name, rank, of):
        bufs[name].zero_()
        return scene.render_shard_fixed(cam, w, h, SPP, rank, of, bufs[name].data_ptr(), seed=SEED, flags=api.FLAG_RNG_PER_SAMPLE)["seconds_render"] * 1e3

    whole_ms, halves_ms = [], []
    for rep in range(1 if a.once else REPS + 1):
        t_whole = shard("whole", 0, 1)
        t_halves = shard("a", 0, 2) + shard("b", 1, 2)
        if rep:
            whole_ms.append(t_whole)
            halves_ms.append(t_halves)
    assert torch.equal(bufs["a"] + bufs["b"], bufs["whole"]), "the half frames do not sum to the whole frame"
    aov, _, _ = scene.render_aov(cam, w, h, SPP, seed=SEED, flags=api.FLAG_WATERTIGHT)
    scratch = torch.empty(api.denoise_dual_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    scratch1 = torch.empty(api.denoise_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    out, out1 = (torch.empty((w * h, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    prm, prm1 = api.denoise_dual_default_params(), api.denoise_default_params()
    A, B, S = bufs["a"], bufs["b"], bufs["whole"]

    def dual(**kw):
        return api.denoise_dual(A, SPP // 2, B, SPP // 2, aov, SPP, w, h, scratch=scratch, out=out, **kw)

    def fixed(**kw):
        return api.denoise(S, SPP, aov, SPP, w, h, scratch=scratch1, out=out1, **kw)

    if a.once:
        for _ in range(2):
            dual(passes=8)
            fixed(passes=8)
        torch.cuda.synchronize()
        print("once ok", float(out.mean()), flush=True)
        return
    res = {"scene": "full_bsdf", "frame": [w, h, SPP], "reps": REPS, "build_id": api.build_id(), "device": torch.cuda.get_device_name(0),
           "params": prm, "fixed_params": dict(prm1, passes=prm["passes"]), "forms": ["direct", "lds"], "g_places": ["inline", "prepass"],
           "tile": [32, 8], "scratch_bytes_per_pixel": api.denoise_dual_scratch_bytes(1, 1)}
    res["call"], res["fixed_call"] = _alternate(torch, [dual, lambda: fixed(passes=prm["passes"])])
    res["call_over_fixed_call"] = round(res["call"]["ms"] / res["fixed_call"]["ms"], 3)
    by = [_alternate(torch, [lambda: dual(passes=p), lambda: fixed(passes=p)]) for p in range(9)]
    res["by_passes"] = {"dual": [b[0] for b in by], "fixed": [b[1] for b in by]}
    # the pass kernels themselves: the scratch of a passes = 0 call holds the prepared frame
    dual(passes=0)
    fixed(passes=0)
    T = api.tools_lib()
    names = [("direct", "inline"), ("direct", "prepass"), ("lds", "inline"), ("lds", "prepass")]
    per = {n: [[] for _ in range(8)] for n in names}
    per1 = {n: [[] for _ in range(8)] for n in ("direct", "lds")}
    buf = (ctypes.c_float * 4)()
    for rnd in range(4):  # (rounds of 4 launches per variant and stride, the variants taking turns; the first round warms up)
        for i in range(8):
            for form, g in names:
                rc = T.rt_denoise_dual_pass_time(ctypes.c_void_p(scratch.data_ptr()), w, h, 1 << i, 1 + (form == "lds"), 1 + (g == "prepass"),
                                                 prm["sigma_variance"], prm["sigma_depth"], prm["normal_power_log2"], 4, buf)
                assert rc == 0, T.rt_last_error().decode()
                if rnd:
                    per[(form, g)][i] += list(buf)
            for form in ("direct", "lds"):
                rc = T.rt_denoise_pass_time(ctypes.c_void_p(scratch1.data_ptr()), w, h, 1 << i, 1 + (form == "lds"), prm1["sigma_color"],
                                            prm1["sigma_depth"], prm1["normal_power_log2"], 4, buf)
                assert rc == 0, T.rt_last_error().decode()
                if rnd:
                    per1[form][i] += list(buf)

    def med(v):
        return statistics.median(v[:REPS])

    res["pass_kernel_ms"] = {form: {g: [_summary(per[(form, g)][i][:REPS]) for i in range(8)] for g in ("inline", "prepass")} for form in ("direct", "lds")}
    res["pass_kernel_ms"]["fixed"] = {form: [_summary(per1[form][i][:REPS]) for i in range(8)] for form in ("direct", "lds")}
    # inline needs no launch and no array of its own: prepass is kept only where its median beats EVERY inline launch
    res["kept_g"] = {form: ["prepass" if med(per[(form, "prepass")][i]) < min(per[(form, "inline")][i][:REPS]) else "inline" for i in range(8)]
                     for form in ("direct", "lds")}
    best = {form: [med(per[(form, res["kept_g"][form][i])][i]) for i in range(8)] for form in ("direct", "lds")}
    res["kept"] = ["lds" if best["lds"][i] < best["direct"][i] else "direct" for i in range(8)]
    res["dual_over_fixed"] = [round(min(best["direct"][i], best["lds"][i]) / min(med(per1["direct"][i]), med(per1["lds"][i])), 3) for i in range(8)]
    res["halves"] = {"whole_frame_render": _summary(whole_ms), "two_half_frame_renders": _summary(halves_ms)}
    res["halves_over_whole"] = round(res["halves"]["two_half_frame_renders"]["ms"] / res["halves"]["whole_frame_render"]["ms"], 4)
    res["call_over_whole_frame_render"] = round(res["call"]["ms"] / res["halves"]["whole_frame_render"]["ms"], 4)
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
