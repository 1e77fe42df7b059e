#!/usr/bin/env python3
"""What temporal accumulation costs (rt_render_motion, rt_temporal_accumulate_fixed), against its neighbours and against the frame
it serves.  C2 (full_bsdf) at 1920 x 1080, warm, medians of 7 with min and max, one process, the compared calls taking turns:

  motion / aov_1spp   rt_render_motion against rt_render_aov_fixed at 1 spp (both RT_FLAG_WATERTIGHT): the device time of the
                      kernel (rt_stats.seconds_render) and the whole call between HIP events on the current stream.  The previous
                      camera is the current one orbited by 2 degrees; `motion_prev_tris` hands over previous vertices as well
  accumulate          api.temporal_accumulate at the default parameters on the second frame of such a pair (history given), with
                      two buffers and with one, outputs allocated before the clock, between HIP events
  torch_blend         the same blend composed from torch ops alone (reproject, four taps, the stops, the blend, to_fixed; float32
                      tensor arithmetic, not the stated sequence: its bits are not the library's) -- it calls no entry point of
                      this feature; the comparison a caller without the kernel has
  beauty_16spp        the frame the stage serves: the 16-spp per-sample beauty frame (rt_render_shard_fixed, seconds_render)
  bytes_per_pixel     what the accumulator must move: every input it uses and every output once (of an AOV pixel the 40 bytes of
                      normal, depth and hits); `lines` counts whole 88-byte AOV pixels instead.  rate = bytes / kernel call time,
                      against the lab's calibrated copy bandwidth (rt_measure_copy_bandwidth, read + write of a 1 GiB buffer)

  python tools/temporal_time.py [--out profiles/temporal_time.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, SPP, SEED = 1920, 1080, 16, 1
REPS = 7


def _summary(ms):
    return {"ms": round(statistics.median(ms), 4), "min_max": [round(min(ms), 4), round(max(ms), 4)]}


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def _alternate(torch, fns):
    """Per fn (call ms summary, list of what it returned), taking turns; the first round warms up and is dropped."""
    ms, ret = [[] for _ in fns], [[] for _ in fns]
    for rep in range(REPS + 1):
        for k, fn in enumerate(fns):
            t, r = _timed(torch, fn)
            if rep:
                ms[k].append(t)
                ret[k].append(r)
    return [(_summary(m), r) for m, r in zip(ms, ret)]


def torch_blend(torch, sums, spps, aov, aov_spp, motion, hist, length, prev_aov, prev_spp, w, h, prm):
    """The accumulator's blend from torch ops: -> ([hist_out per buffer], len_out)."""
    n = w * h
    scale = 2.0 ** -30
    c = [(s.double() * scale).float() * (1.0 / k) for s, k in zip(sums, spps)]
    n_p = (aov[:, 3:6].double() * scale).float() * (1.0 / aov_spp)
    hits_q = prev_aov[:, 10]
    n_q = (prev_aov[:, 3:6].double() * scale).float() * (1.0 / prev_spp)
    z_q = torch.where(hits_q > 0, (prev_aov[:, 9].double() * scale).float() / hits_q.float().clamp(min=1), torch.zeros((), device=aov.device))
    h_in = [(x.double() * scale).float() for x in hist]
    tri = motion[:, 3].view(torch.int32)
    fx, fy, dist = motion[:, 0] - 0.5, motion[:, 1] - 0.5, motion[:, 2]
    ok = (tri >= 0) & (fx >= -1) & (fx < w) & (fy >= -1) & (fy < h)
    fx, fy = torch.where(ok, fx, torch.zeros_like(fx)), torch.where(ok, fy, torch.zeros_like(fy))
    flx, fly = torch.floor(fx), torch.floor(fy)
    x0, y0 = flx.long(), fly.long()
    ax, ay = fx - flx, fy - fly
    sw = torch.zeros(n, device=aov.device)
    sh = [torch.zeros((n, 3), device=aov.device) for _ in sums]
    n_prev = torch.full((n,), 0x7fffffff, dtype=torch.int64, device=aov.device)
    for j in (0, 1):
        for i in (0, 1):
            xx, yy = x0 + i, y0 + j
            inside = ok & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            q = torch.where(inside, yy * w + xx, torch.zeros_like(xx))
            acc = inside & (length[q] >= 1) & (hits_q[q] > 0) & ((z_q[q] - dist).abs() <= prm["depth_tolerance"] * dist) & \
                ((n_p * n_q[q]).sum(1) >= prm["normal_cos_min"])
            b = (ax if i else 1 - ax) * (ay if j else 1 - ay)
            b = torch.where(acc, b, torch.zeros_like(b))
            sw = sw + b
            for k in range(len(sums)):
                sh[k] = sh[k] + b[:, None] * h_in[k][q]
            n_prev = torch.where(acc, torch.minimum(n_prev, length[q].long()), n_prev)
    blend = sw > 0
    N = torch.where(blend, torch.clamp(n_prev + 1, max=prm["max_history"]), torch.ones_like(n_prev))
    alpha = torch.clamp(1.0 / N.float(), min=prm["alpha_min"])[:, None]
    outs = []
    for k in range(len(sums)):
        hbar = sh[k] / sw.clamp(min=1e-30)[:, None]
        o = torch.where(blend[:, None], (c[k] - hbar) * alpha + hbar, c[k])
        outs.append(torch.round(o.clamp(-2147483648.0, 2147483648.0) * 1073741824.0).long())
    return outs, N.int()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_time.json"))
    ap.add_argument("--size", nargs=2, type=int, default=[W, H], help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    from rtcuda_amd import api, scenes
    assert torch.cuda.is_available(), "temporal_time.py measures on a GPU"
    w, h = a.size
    n = w * h
    arrays = scenes.cornell_bunny("full_bsdf")
    scene = api.Scene(arrays)

    def orbit(k):
        ang = np.deg2rad(2.0 * k)
        return api.make_camera((0.5 + 1.5 * np.sin(ang), 0.5, 1.5 * np.cos(ang)), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8, w / h)

    cams = [orbit(0), orbit(1)]
    prev_tris = torch.from_numpy(np.ascontiguousarray(arrays.tris, np.float32).reshape(-1, 9)).cuda()
    motion = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    aov1 = torch.zeros((n, api.AOV_CHANNELS), dtype=torch.int64, device="cuda")
    F = api.FLAG_WATERTIGHT

    def run_motion(prev=None):
        return scene.render_motion(cams[1], w, h, cams[0], prev_tris=prev, flags=F, out=motion)[1]["seconds_render"] * 1e3

    def run_aov1():
        aov1.zero_()
        return scene.render_aov(cams[1], w, h, 1, seed=SEED, flags=F, out=aov1)[2]["seconds_render"] * 1e3

    res = {"scene": "full_bsdf", "frame": [w, h], "reps": REPS, "build_id": api.build_id(), "device": torch.cuda.get_device_name(0),
           "params": api.temporal_default_params(), "orbit_degrees": 2.0}
    (m_call, m_k), (mp_call, mp_k), (a_call, a_k) = _alternate(torch, [run_motion, lambda: run_motion(prev_tris), run_aov1])
    res["motion"] = {"call": m_call, "kernel": _summary(m_k)}
    res["motion_prev_tris"] = {"call": mp_call, "kernel": _summary(mp_k)}
    res["aov_1spp"] = {"call": a_call, "kernel": _summary(a_k), "note": "the call includes zeroing its 88-byte-per-pixel sum buffer"}
    res["motion_over_aov_1spp_kernel"] = round(res["motion"]["kernel"]["ms"] / res["aov_1spp"]["kernel"]["ms"], 3)

    # two frames of the composition: halves, AOV, motion; frame 0 gives the history of frame 1
    frames = []
    beauty_ms = []
    for k in (0, 1):
        halves = []
        for r in (0, 1):
            t = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
            scene.render_shard_fixed(cams[k], w, h, SPP, r, 2, t.data_ptr(), seed=SEED + k, flags=api.FLAG_RNG_PER_SAMPLE)
            halves.append(t)
        aov, _, _ = scene.render_aov(cams[k], w, h, SPP, seed=SEED + k, flags=F)
        mo, _ = scene.render_motion(cams[k], w, h, cams[max(k - 1, 0)], flags=F)
        frames.append((halves, aov, mo))
    whole = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
    for rep in range(REPS + 1):
        whole.zero_()
        t = scene.render_shard_fixed(cams[1], w, h, SPP, 0, 1, whole.data_ptr(), seed=SEED + 1, flags=api.FLAG_RNG_PER_SAMPLE)["seconds_render"] * 1e3
        if rep:
            beauty_ms.append(t)
    res["beauty_16spp"] = _summary(beauty_ms)
    (h0, a0, m0), (h1, a1, m1) = frames
    first = api.temporal_accumulate(h0[0], SPP // 2, h0[1], SPP // 2, a0, SPP, m0, None, w, h)
    out2 = tuple(torch.empty_like(t) for t in first)
    out1 = (out2[0], None, out2[2])
    prm = api.temporal_default_params()

    def two():
        api.temporal_accumulate(h1[0], SPP // 2, h1[1], SPP // 2, a1, SPP, m1, (first[0], first[1], first[2], a0, SPP), w, h, out=out2)

    def one():
        api.temporal_accumulate(h1[0], SPP // 2, None, 0, a1, SPP, m1, (first[0], None, first[2], a0, SPP), w, h, out=out1)

    def blend(nbuf):
        return torch_blend(torch, h1[:nbuf], [SPP // 2] * nbuf, a1, SPP, m1, [first[0], first[1]][:nbuf], first[2], a0, SPP, w, h, prm)

    (t2, _), (t1, _), (b2, r2), (b1, _) = _alternate(torch, [two, one, lambda: blend(2), lambda: blend(1)])
    res["accumulate"] = {"two_buffers": t2, "one_buffer": t1}
    res["torch_blend"] = {"two_buffers": b2, "one_buffer": b1}
    two()
    same_len = float((r2[-1][1] == out2[2]).float().mean())
    close = float(((r2[-1][0][0] - out2[0]).abs() <= 64).float().mean())
    res["torch_blend"]["agreement_with_the_kernel"] = {"len_equal_share": round(same_len, 6), "hist_a_within_64_units_share": round(close, 6)}
    res["kept_history_share"] = round(float((out2[2] > 1).float().mean()), 4)
    res["torch_over_kernel"] = {"two_buffers": round(b2["ms"] / t2["ms"], 2), "one_buffer": round(b1["ms"] / t1["ms"], 2)}
    res["accumulate_over_beauty_16spp"] = {"two_buffers": round(t2["ms"] / res["beauty_16spp"]["ms"], 5), "one_buffer": round(t1["ms"] / res["beauty_16spp"]["ms"], 5)}
    used = {"two_buffers": 2 * 24 + 40 + 16 + 2 * 24 + 4 + 40 + 2 * 24 + 4, "one_buffer": 24 + 40 + 16 + 24 + 4 + 40 + 24 + 4}
    lines = {k: v + 2 * 48 for k, v in used.items()}
    bw = api.measure_copy_bandwidth()
    res["copy_bandwidth_GBps"] = round(bw / 1e9, 1)
    res["bytes_per_pixel"] = {"used": used, "lines": lines}
    res["rate_GBps"] = {k: round(used[k] * n / (res["accumulate"][k]["ms"] * 1e-3) / 1e9, 1) for k in used}
    res["rate_over_copy_bandwidth"] = {k: round(res["rate_GBps"][k] * 1e9 / bw, 3) for k in used}
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
