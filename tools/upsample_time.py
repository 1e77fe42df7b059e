#!/usr/bin/env python3
"""What AOV-guided upsampling costs (rt_upsample_fixed), and what a frame built with it costs against the frames it replaces.

C2 (full_bsdf), full size 1920 x 1080, from 960 x 540 (x 2) and from 480 x 270 (x 4); warm, medians of 7 with min and max, HIP
events on the current stream around calls that are synchronous on it, one process, the variants of a comparison taking turns:

  call            api.upsample with the default parameters, both outputs, allocated before the clock; `rgb_only` / `fixed_only`:
                  one output; `rgb_input`: api.upsample_rgb on the low frame's float mean, both outputs
  torch           the same filter composed from torch ops (gathers of the 16 taps, float32; not bit-exact: `max_abs_diff` against
                  the library's output is recorded) on the same tensors
  bytes           what the call must move: per full pixel the 88-byte AOV record and 12 + 24 bytes of output, per low pixel 24 + 88
                  bytes; `copy_ms` is that over the copy bandwidth rt_measure_copy_bandwidth measures in this process (a float4
                  copy, bytes read + bytes written per second), `call_over_copy` the call's median over it
  frame           the point of the feature, per factor: rt_render_shard_fixed at the low size with factor^2 * 4 spp + rt_render_aov_fixed
                  at the low size (the same spp) + rt_render_aov_fixed at the full size (4 spp) + the upsample call, each timed,
                  against rt_render_shard_fixed at the full size with 4 spp (the same sample budget) and with 16 spp
                  (RT_FLAG_RNG_PER_SAMPLE frames, as the AOVs are defined on them); every render and AOV time includes zeroing
                  the buffer the call adds into

  python tools/upsample_time.py [--out profiles/upsample_time.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, SEED = 1920, 1080, 1
FULL_SPP = 4
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


def torch_upsample(torch, beauty, spp, aov_lo, s_lo, lw, lh, f, aov_hi, s_hi, sigma_depth, npw):
    """rt_upsample_fixed's filter from torch ops -> (n, 3) float32."""
    w, h = f * lw, f * lh

    def features(aov, s):
        a = (aov.to(torch.float64) * 2.0 ** -30).to(torch.float32)
        hits = aov[:, 10]
        z = torch.where(hits > 0, a[:, 9] / hits.to(torch.float32).clamp_min(1.0), torch.zeros_like(a[:, 9]))
        return a[:, 0:3] / s, a[:, 3:6] / s, a[:, 6:9] / s, z, hits

    alb, n_lo, e_lo, z_lo, _ = features(aov_lo, s_lo)
    c = (beauty.to(torch.float64) * 2.0 ** -30).to(torch.float32) / spp
    u_lo = (c - e_lo).clamp_min(0.0) / alb.clamp_min(2.0 ** -10)
    alb_h, n_hi, e_hi, z_hi, hits_hi = features(aov_hi, s_hi)
    kz = 1.0 / (sigma_depth * sigma_depth)

    def axis(n):
        x = torch.arange(n, device=beauty.device)
        a = 2 * x + 1 - f
        x0 = torch.div(a, 2 * f, rounding_mode="floor")
        return x0, (a - 2 * f * x0).to(torch.float32) / (2 * f)

    x0, fx = axis(w)
    y0, fy = axis(h)
    sw, sh = (torch.zeros(h * w, device=beauty.device) for _ in range(2))
    su, sb = (torch.zeros((h * w, 3), device=beauty.device) for _ in range(2))
    for jy in range(-1, 3):
        qy, ky = y0 + jy, 1.0 - 0.5 * (jy - fy).abs()
        for jx in range(-1, 3):
            qx, kx = x0 + jx, 1.0 - 0.5 * (jx - fx).abs()
            inside = (((qy >= 0) & (qy < lh))[:, None] & ((qx >= 0) & (qx < lw))[None, :]).reshape(-1)
            q = (qy.clamp(0, lh - 1)[:, None] * lw + qx.clamp(0, lw - 1)[None, :]).reshape(-1)
            hk = (ky[:, None] * kx[None, :]).reshape(-1) * inside
            dz = z_lo[q] - z_hi
            wn = (n_lo[q] * n_hi).sum(1).clamp(0.0, 1.0)
            for _ in range(npw):
                wn = wn * wn
            wt = hk * torch.exp(-(dz * dz) * kz) * wn
            uq = u_lo[q]
            sw, sh = sw + wt, sh + hk
            su, sb = su + wt[:, None] * uq, sb + hk[:, None] * uq
    u = torch.where((sw > 0)[:, None], su / sw.clamp_min(1e-45)[:, None], sb / sh[:, None])
    u = torch.where((hits_hi > 0)[:, None], u, torch.zeros_like(u))
    return u * alb_h.clamp_min(2.0 ** -10) + e_hi


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_time.json"))
    ap.add_argument("--size", nargs=2, type=int, default=[W, H], help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    from rtcuda_amd import api, scenes
    assert torch.cuda.is_available(), "upsample_time.py measures on a GPU"
    w, h = a.size
    assert w % 4 == 0 and h % 4 == 0
    n = w * h
    scene = api.Scene(scenes.cornell_bunny("full_bsdf"))
    cam = api.make_camera(aspect=w / h)
    prm = api.upsample_default_params()
    res = {"scene": "full_bsdf", "full_frame": [w, h], "full_spp": FULL_SPP, "reps": REPS, "build_id": api.build_id(),
           "device": torch.cuda.get_device_name(0), "params": prm, "tile": [32, 8], "factors": {}}
    bw = api.measure_copy_bandwidth()
    res["copy_bandwidth_GBps"] = round(bw / 1e9, 1)

    def render(buf, ww, hh, spp):
        buf.zero_()
        return lambda: scene.render_shard_fixed(cam, ww, hh, spp, 0, 1, buf.data_ptr(), seed=SEED, flags=api.FLAG_RNG_PER_SAMPLE)

    full = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
    aov_hi = torch.zeros((n, api.AOV_CHANNELS), dtype=torch.int64, device="cuda")
    out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    out_fixed = torch.empty((n, 3), dtype=torch.int64, device="cuda")

    def aov(buf, ww, hh, spp):
        def run():
            buf.zero_()
            scene.render_aov(cam, ww, hh, spp, seed=SEED, flags=api.FLAG_WATERTIGHT, out=buf)
        return run

    def zeroed(buf, fn):
        def run():
            buf.zero_()
            fn()
        return run

    for f in (2, 4):
        lw, lh, spp = w // f, h // f, FULL_SPP * f * f
        low = torch.zeros((lw * lh, 3), dtype=torch.int64, device="cuda")
        aov_lo = torch.zeros((lw * lh, api.AOV_CHANNELS), dtype=torch.int64, device="cuda")
        render(low, lw, lh, spp)()
        aov(aov_lo, lw, lh, spp)()
        aov(aov_hi, w, h, FULL_SPP)()
        rgb_lo = ((low.to(torch.float64) * 2.0 ** -30).to(torch.float32) / spp).contiguous()
        args = (aov_lo, spp, lw, lh, f, aov_hi, FULL_SPP)

        def call(**kw):
            return api.upsample(low, spp, *args, **kw)

        entry = {"low_frame": [lw, lh, spp]}
        entry["call"], entry["rgb_only"], entry["fixed_only"], entry["rgb_input"] = _alternate(torch, [
            lambda: call(out=out, out_fixed=out_fixed), lambda: call(out=out, fixed=False), lambda: call(out_fixed=out_fixed, rgb=False),
            lambda: api.upsample_rgb(rgb_lo, *args, out=out, out_fixed=out_fixed)])
        call(out=out, out_fixed=out_fixed)
        composed = torch_upsample(torch, low, spp, aov_lo, spp, lw, lh, f, aov_hi, FULL_SPP, prm["sigma_depth"], prm["normal_power_log2"])
        entry["torch"] = _alternate(torch, [lambda: torch_upsample(torch, low, spp, aov_lo, spp, lw, lh, f, aov_hi, FULL_SPP, prm["sigma_depth"],
                                                                   prm["normal_power_log2"])])[0]
        entry["torch"]["max_abs_diff"] = float((composed - out).abs().max())
        entry["torch_over_call"] = round(entry["torch"]["ms"] / entry["call"]["ms"], 1)
        moved = n * (88 + 12 + 24) + lw * lh * (24 + 88)
        entry["bytes"] = {"moved": moved, "copy_ms": round(moved / bw * 1e3, 4)}
        entry["call_over_copy"] = round(entry["call"]["ms"] / entry["bytes"]["copy_ms"], 2)
        # the whole frame: its four calls one after the other, against the full-size frame at the same budget and at 16 spp
        parts = _alternate(torch, [zeroed(low, render(low, lw, lh, spp)), aov(aov_lo, lw, lh, spp), aov(aov_hi, w, h, FULL_SPP),
                                   lambda: call(out=out, out_fixed=out_fixed), zeroed(full, render(full, w, h, FULL_SPP)),
                                   zeroed(full, render(full, w, h, 16))])
        names = ("render_low", "aov_low", "aov_full", "upsample", "render_full_4spp", "render_full_16spp")
        entry["frame"] = dict(zip(names, parts))
        total = sum(parts[k]["ms"] for k in range(4))
        entry["frame"]["upsampled_total_ms"] = round(total, 4)
        entry["frame"]["full_4spp_plus_aov_ms"] = round(parts[4]["ms"] + parts[2]["ms"], 4)
        entry["frame"]["upsampled_over_full_4spp_plus_aov"] = round(total / (parts[4]["ms"] + parts[2]["ms"]), 3)
        entry["frame"]["upsampled_over_full_16spp_plus_aov"] = round(total / (parts[5]["ms"] + parts[2]["ms"]), 3)
        res["factors"]["x%d" % f] = entry
        print(json.dumps({"x%d" % f: entry}), flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
