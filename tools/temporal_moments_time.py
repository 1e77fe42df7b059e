#!/usr/bin/env python3
"""What the single-buffer loop costs (rt_temporal_accumulate_moments_fixed, rt_denoise_variance_fixed) against the entry points it
stands beside.  C2 (full_bsdf) at 1920 x 1080, warm, medians of 7 with min and max, one process, the compared calls taking turns,
every call between HIP events on the current stream with its outputs allocated before the clock (tools/temporal_time.py's method):

  accumulate_off      the new entry point with everything off (emission_tolerance = +inf, no previous motion, no moments) against
                      rt_temporal_accumulate_fixed on the same buffers, two buffers and one: the same pixel body, the instantiation
                      with the features against the one without
  accumulate_on       the new entry point on the second frame of an orbit pair: two buffers with both stops; one buffer with both
                      stops and moments at variance_min_history = 1 (no pixel takes the spatial estimate) and at a
                      variance_min_history beyond every length (every pixel takes it)
  spatial_estimate    that one-buffer call by the share of pixels that owe a spatial estimate (a workgroup with such a pixel stages
                      its tile and a halo of 2 in LDS): none (variance_min_history = 1), the pixels that lost their history (2:
                      the second frame's lengths are 1 or 2), every pixel
  denoise             rt_denoise_variance_fixed against rt_denoise_dual_fixed at the defaults' passes on the accumulated frame
  loop                the whole frame: one 16-spp shard call + AOV + motion + new accumulator at its defaults (the emission stop,
                      moments, no previous motion buffer) + denoise_variance against two 8-spp shard calls + AOV + motion + old
                      accumulator + denoise_dual

  python tools/temporal_moments_time.py [--out profiles/temporal_moments_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from temporal_time import H, REPS, SEED, SPP, W, _alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_moments_time.json"))
    ap.add_argument("--size", nargs=2, type=int, default=[W, H], help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    from rtcuda_amd import api, scenes
    assert torch.cuda.is_available(), "temporal_moments_time.py measures on a GPU"
    w, h = a.size
    n = w * h
    scene = api.Scene(scenes.cornell_bunny("full_bsdf"))
    F, PS = api.FLAG_WATERTIGHT, api.FLAG_RNG_PER_SAMPLE

    def orbit(k):
        ang = np.deg2rad(2.0 * k)
        return api.make_camera((0.5 + 1.5 * np.sin(ang), 0.5, 1.5 * np.cos(ang)), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8, w / h)

    cams = [orbit(0), orbit(1)]
    i64 = lambda: torch.zeros((n, 3), dtype=torch.int64, device="cuda")  # noqa: E731
    frames = []
    for k in (0, 1):
        halves = [i64(), i64()]
        for r in (0, 1):
            scene.render_shard_fixed(cams[k], w, h, SPP, r, 2, halves[r].data_ptr(), seed=SEED + k, flags=PS)
        aov, _, _ = scene.render_aov(cams[k], w, h, SPP, seed=SEED + k, flags=F)
        mo, _ = scene.render_motion(cams[k], w, h, cams[max(k - 1, 0)], flags=F)
        frames.append((halves, halves[0] + halves[1], aov, mo))
    (h0, s0, a0, m0), (h1, s1, a1, m1) = frames
    old = api.temporal_default_params()
    new = api.temporal_moments_default_params()
    off = dict(old, emission_tolerance=float("inf"), variance_min_history=1)
    res = {"scene": "full_bsdf", "frame": [w, h], "reps": REPS, "build_id": api.build_id(), "device": torch.cuda.get_device_name(0),
           "old_params": old, "new_params": {k: (v if np.isfinite(v) else "inf") for k, v in new.items()}, "orbit_degrees": 2.0, "spp": SPP}

    # ---- the accumulators on frame 1, frame 0 being the history
    first2 = api.temporal_accumulate(h0[0], SPP // 2, h0[1], SPP // 2, a0, SPP, m0, None, w, h)
    first1 = api.temporal_accumulate_moments(s0, SPP, None, 0, a0, SPP, m0, None, w, h)
    o2 = tuple(torch.empty_like(t) for t in first2)
    o1 = (o2[0], None, o2[2])
    n2 = o2 + (None, None)
    n1 = (o2[0], None, o2[2], torch.empty_like(first1[3]), torch.empty_like(first1[4]))
    hist2, hist1 = (first2[0], first2[1], first2[2], a0, SPP), (first2[0], None, first2[2], a0, SPP)

    def old_two():
        api.temporal_accumulate(h1[0], SPP // 2, h1[1], SPP // 2, a1, SPP, m1, hist2, w, h, out=o2)

    def old_one():
        api.temporal_accumulate(h1[0], SPP // 2, None, 0, a1, SPP, m1, hist1, w, h, out=o1)

    def new_two(prm, prev_motion):
        api.temporal_accumulate_moments(h1[0], SPP // 2, h1[1], SPP // 2, a1, SPP, m1, hist2 + (prev_motion, None), w, h, moments=False, out=n2, **prm)

    def new_one_off():
        api.temporal_accumulate_moments(h1[0], SPP // 2, None, 0, a1, SPP, m1, hist1 + (None, None), w, h, moments=False, out=n1[:3] + (None, None), **off)

    def new_one(vmh):
        api.temporal_accumulate_moments(s1, SPP, None, 0, a1, SPP, m1, (first1[0], None, first1[2], a0, SPP, m0, first1[3]), w, h, out=n1,
                                        **dict(new, variance_min_history=vmh))

    far = 1 << 20
    (t_o2, _), (t_n2, _), (t_o1, _), (t_n1, _) = _alternate(torch, [old_two, lambda: new_two(off, None), old_one, new_one_off])
    res["accumulate_off"] = {"old_two_buffers": t_o2, "new_two_buffers": t_n2, "old_one_buffer": t_o1, "new_one_buffer": t_n1,
                             "new_over_old": {"two_buffers": round(t_n2["ms"] / t_o2["ms"], 3), "one_buffer": round(t_n1["ms"] / t_o1["ms"], 3)}}
    (t_s2, _), (t_m1, _), (t_sp, _), (t_o1b, _) = _alternate(torch, [lambda: new_two(new, m0), lambda: new_one(1), lambda: new_one(far), old_one])
    new_one(1)
    kept = float((n1[2] > 1).float().mean())
    res["accumulate_on"] = {"two_buffers_both_stops": t_s2, "one_buffer_stops_moments_temporal_variance": t_m1,
                            "one_buffer_stops_moments_spatial_variance_everywhere": t_sp, "old_one_buffer": t_o1b, "kept_history_share": round(kept, 4),
                            "over_old_one_buffer": {"temporal": round(t_m1["ms"] / t_o1b["ms"], 3), "spatial_everywhere": round(t_sp["ms"] / t_o1b["ms"], 3)}}

    # ---- what the spatial estimate costs by the share of pixels that owe one
    cases = (("none_owes", 1), ("lost_history_owes", 2), ("every_pixel_owes", far))
    timed = _alternate(torch, [lambda vmh=vmh: new_one(vmh) for _, vmh in cases])
    res["spatial_estimate"] = {}
    for (name, vmh), (t, _) in zip(cases, timed):
        new_one(vmh)
        res["spatial_estimate"][name] = dict(t, variance_min_history=vmh, owing_share=round(float((n1[2] < vmh).float().mean()), 4))

    # ---- the denoisers on the accumulated frame
    old_two()
    acc2 = (o2[0].clone(), o2[1].clone())
    new_one(new["variance_min_history"])
    acc1, var1 = n1[0].clone(), n1[4].clone()
    scratch = torch.empty(api.denoise_dual_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    (t_dd, _), (t_dv, _) = _alternate(torch, [lambda: api.denoise_dual(acc2[0], 1, acc2[1], 1, a1, SPP, w, h, scratch=scratch, out=rgb),
                                              lambda: api.denoise_variance(acc1, 1, var1, a1, SPP, w, h, scratch=scratch, out=rgb)])
    res["denoise"] = {"passes": api.denoise_dual_default_params()["passes"], "denoise_dual": t_dd, "denoise_variance": t_dv,
                      "variance_over_dual": round(t_dv["ms"] / t_dd["ms"], 3)}

    # ---- the whole frame
    aov_buf = torch.zeros((n, api.AOV_CHANNELS), dtype=torch.int64, device="cuda")
    mo_buf = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ha, hb, whole = i64(), i64(), i64()

    def common():
        aov_buf.zero_()
        scene.render_aov(cams[1], w, h, SPP, seed=SEED + 1, flags=F, out=aov_buf)
        scene.render_motion(cams[1], w, h, cams[0], flags=F, out=mo_buf)

    def loop_old():
        ha.zero_(), hb.zero_()
        scene.render_shard_fixed(cams[1], w, h, SPP, 0, 2, ha.data_ptr(), seed=SEED + 1, flags=PS)
        scene.render_shard_fixed(cams[1], w, h, SPP, 1, 2, hb.data_ptr(), seed=SEED + 1, flags=PS)
        common()
        api.temporal_accumulate(ha, SPP // 2, hb, SPP // 2, aov_buf, SPP, mo_buf, hist2, w, h, out=o2)
        api.denoise_dual(o2[0], 1, o2[1], 1, aov_buf, SPP, w, h, scratch=scratch, out=rgb)

    def loop_new():
        whole.zero_()
        scene.render_shard_fixed(cams[1], w, h, SPP, 0, 1, whole.data_ptr(), seed=SEED + 1, flags=PS)
        common()
        api.temporal_accumulate_moments(whole, SPP, None, 0, aov_buf, SPP, mo_buf, (first1[0], None, first1[2], a0, SPP, None, first1[3]), w, h, out=n1)
        api.denoise_variance(n1[0], 1, n1[4], aov_buf, SPP, w, h, scratch=scratch, out=rgb)

    (t_lo, _), (t_ln, _) = _alternate(torch, [loop_old, loop_new])
    res["loop"] = {"two_8spp_shards_old_accumulator_denoise_dual": t_lo, "one_16spp_shard_new_accumulator_denoise_variance": t_ln,
                   "new_over_old": round(t_ln["ms"] / t_lo["ms"], 3)}
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
