#!/usr/bin/env python3
"""What following mirror and glass costs (rt_render_aov_follow_fixed) against the first-hit buffers (rt_render_aov_fixed).

C2 (full_bsdf) at 1920 x 1080 x 16 = 33 177 600 samples, warm, medians of 7 with min and max.

  follow   one process, the calls taking turns repetition by repetition: rt_render_aov_fixed, then rt_render_aov_follow_fixed at
           max_specular 0, 1, 2 and 5.  Per call: `kernel` = rt_stats.seconds_render (HIP events around the kernel), its ratio to
           the first-hit call, closest_rays per sample, and its share of the 16-spp per-sample beauty frame of the same size
           (rt_render_shard_fixed, RT_FLAG_RNG_PER_SAMPLE, 10 bounces), timed in the same process.
  parent   (--parent-tree PATH: a built checkout of the parent commit) rt_render_aov_fixed on that build and on this one, taking
           turns as child processes, --turns each: did the first-hit kernel move?

  python tools/aov_follow_time.py [--parent-tree <built checkout of the parent>] --out profiles/aov_follow_time.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

# (AOV_FOLLOW_TREE: the checkout whose package a child process imports -- the parent commit's, for the `parent` leg)
ROOT = os.environ.get("AOV_FOLLOW_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, SPP, SEED = 1920, 1080, 16, 1
REPS = 7
CAPS = (0, 1, 2, 5)


def _summary(ms):
    return {"ms": round(statistics.median(ms), 4), "min_max": [round(min(ms), 4), round(max(ms), 4)]}


def leg_follow(width, height, spp):
    import torch
    from rtcuda_amd import api, scenes
    scene = api.Scene(scenes.cornell_bunny("full_bsdf"))
    cam = api.make_camera(aspect=width / height)
    n = width * height * spp
    sums = torch.zeros((width * height, api.AOV_CHANNELS), dtype=torch.int64, device="cuda")
    calls = [("first_hit", lambda: scene.render_aov(cam, width, height, spp, seed=SEED, out=sums))]
    for cap in CAPS:
        calls.append(("follow_%d" % cap, lambda cap=cap: scene.render_aov_follow(cam, width, height, spp, cap, seed=SEED, out=sums)))
    ms = {name: [] for name, _ in calls}
    rays, hits = {}, {}
    for rep in range(REPS + 1):  # (the first repetition warms up and is dropped)
        for name, call in calls:
            sums.zero_()
            _, _, st = call()
            if rep:
                ms[name].append(st["seconds_render"] * 1e3)
            rays[name], hits[name] = st["closest_rays"], int(sums[:, api.AOV_HITS].sum())
    fb = torch.zeros((width * height, 3), dtype=torch.int64, device="cuda")
    beauty = []
    for rep in range(REPS + 1):
        fb.zero_()
        st = scene.render_shard_fixed(cam, width, height, spp, 0, 1, fb.data_ptr(), seed=SEED, flags=api.FLAG_RNG_PER_SAMPLE)
        if rep:
            beauty.append(st["seconds_render"] * 1e3)
    out = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "frame": [width, height, spp],
           "beauty_per_sample_10_bounces": _summary(beauty)}
    base = statistics.median(ms["first_hit"])
    for name, _ in calls:
        out[name] = {"kernel": _summary(ms[name]), "ratio_to_first_hit": round(statistics.median(ms[name]) / base, 3),
                     "closest_rays_per_sample": round(rays[name] / n, 4), "hits": hits[name],
                     "share_of_beauty_frame": round(statistics.median(ms[name]) / statistics.median(beauty), 4)}
    print(json.dumps(out), flush=True)


def leg_first_hit(width, height, spp):
    """rt_render_aov_fixed alone, on the package of AOV_FOLLOW_TREE (default: this checkout)."""
    from rtcuda_amd import api, scenes
    scene = api.Scene(scenes.cornell_bunny("full_bsdf"))
    cam = api.make_camera(aspect=width / height)
    import torch
    sums = torch.zeros((width * height, api.AOV_CHANNELS), dtype=torch.int64, device="cuda")
    ms = []
    for rep in range(REPS + 1):
        sums.zero_()
        _, _, st = scene.render_aov(cam, width, height, spp, seed=SEED, out=sums)
        if rep:
            ms.append(st["seconds_render"] * 1e3)
    print(json.dumps({"build_id": api.build_id(), "kernel": _summary(ms), "reps": [round(x, 4) for x in ms]}), flush=True)


def _child(leg, env=None, size=(W, H, SPP)):
    e = dict(os.environ, **(env or {}))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--size", *map(str, size)], env=e, capture_output=True,
                         text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit("leg %s failed (%d):\n%s" % (leg, out.returncode, out.stderr[-2000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")
    ap.add_argument("--size", nargs=3, type=int, default=[W, H, SPP])
    ap.add_argument("--parent-tree")
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.leg == "follow":
        return leg_follow(*a.size)
    if a.leg == "first_hit":
        return leg_first_hit(*a.size)
    res = {"follow": _child("follow", size=a.size)}
    if a.parent_tree:
        turns = []
        for _ in range(a.turns):
            turns.append({"parent": _child("first_hit", {"AOV_FOLLOW_TREE": os.path.abspath(a.parent_tree)}, a.size),
                          "commit": _child("first_hit", size=a.size)})
        p = [x for t in turns for x in t["parent"]["reps"]]
        c = [x for t in turns for x in t["commit"]["reps"]]
        res["first_hit_parent_vs_commit"] = {"turns": turns, "parent": _summary(p), "commit": _summary(c),
                                             "commit_median_inside_parent_spread": min(p) <= statistics.median(c) <= max(p)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
