#!/usr/bin/env python3
"""What the first-hit feature buffers cost (rt_render_aov_fixed), against what a caller did before they existed.

C2 (full_bsdf) at 1920 x 1080 x 16 = 33 177 600 samples, warm, medians of 7 with min and max.  Every leg runs in a child
process of its own, on the library it names:

  aov          rt_render_aov_fixed at flags 0 and RT_FLAG_WATERTIGHT: `kernel_ms` = rt_stats.seconds_render (HIP events around
               k_aov), `call_ms` = events around the whole call on the current stream; and the per-sample beauty frame of the same
               size (rt_render_shard_fixed, RT_FLAG_RNG_PER_SAMPLE, 10 bounces) for scale
  today        (--parent-lib PATH: the parent commit's build; default: the product library) the route a caller took before:
               rt_query_closest_device on a prebuilt DEVICE table of the same rays, then the torch gather (material, albedo, the
               per-triangle shading normal faced to the viewer, emission, depth), the conversion to fixed point and index_add_
               into the same (n_pixels, 11) int64 sums.  The table (0.8 GB) and the per-triangle arrays are built before the
               clock starts.  `sums_equal_aov`: whether those sums are rt_render_aov_fixed's, integer for integer
  no_deposit   (--no-deposit-lib NAME: a library made by `make -C rtcuda_amd/csrc variant NAME=aov_nodeposit
               DEFS=-DRT_AOV_NO_DEPOSIT`, never the product) the aov leg with the deposit block -- the material and light reads,
               the conversions, the pre-reduction and the 64-bit atomics -- compiled out: `deposit_share` = 1 - kernel_ms(no
               deposit) / kernel_ms
  per_lane     (--per-lane-lib NAME: a variant made with DEFS=-DRT_AOV_PRE_REDUCE=0) the aov leg with the first version's deposit,
               one atomic per non-zero channel and hitting lane, without the wave-level pre-reduction

  python tools/aov_time.py --parent-lib <parent build>/librtcuda_amd.so --no-deposit-lib librtcuda_amd_aov_nodeposit.so \\
      --per-lane-lib librtcuda_amd_aov_perlane.so --out profiles/aov_time.json
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

W, H, SPP, SEED = 1920, 1080, 16, 1
REPS = 7
M64 = (1 << 64) - 1


def _summary(ms):
    return {"ms": round(statistics.median(ms), 4), "min_max": [round(min(ms), 4), round(max(ms), 4)]}


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def leg_aov(width, height, spp):
    """The product entry point (the library RT_LIB_NAME selects), and the beauty frame of the same size."""
    import torch
    from rtcuda_amd import api, scenes
    scene = api.Scene(scenes.cornell_bunny("full_bsdf"))
    cam = api.make_camera(aspect=width / height)
    out = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0)}
    sums = torch.zeros((width * height, api.AOV_CHANNELS), dtype=torch.int64, device="cuda")
    for name, flags in (("flags_0", 0), ("watertight", api.FLAG_WATERTIGHT)):
        kernel, call = [], []
        for rep in range(REPS + 1):  # (the first repetition warms up and is dropped)
            sums.zero_()
            ms, (_, _, st) = _timed(torch, lambda: scene.render_aov(cam, width, height, spp, seed=SEED, flags=flags, out=sums))
            if rep:
                kernel.append(st["seconds_render"] * 1e3)
                call.append(ms)
        out[name] = {"kernel": _summary(kernel), "call": _summary(call), "Msamples_s": round(width * height * spp / statistics.median(kernel) / 1e3, 1),
                     "hits": int(sums[:, api.AOV_HITS].sum()), "literal_retraces": st["literal_retraces"]}
    if os.environ.get("AOV_TIME_SUMS"):
        torch.save(sums.cpu(), os.environ["AOV_TIME_SUMS"])  # (the watertight frame: what the `today` leg compares its sums with)
    fb = torch.zeros((width * height, 3), dtype=torch.int64, device="cuda")
    beauty = []
    for rep in range(REPS + 1):
        fb.zero_()
        st = scene.render_shard_fixed(cam, width, height, spp, 0, 1, fb.data_ptr(), seed=SEED, flags=api.FLAG_RNG_PER_SAMPLE)
        if rep:
            beauty.append(st["seconds_render"] * 1e3)
    out["beauty_per_sample_10_bounces"] = {"render": _summary(beauty)}
    print(json.dumps(out), flush=True)


def _u64(x):
    """A Python int in 0 .. 2^64 - 1 as the int64 with the same bits."""
    return x - (1 << 64) if x >= 1 << 63 else x


def _lsr(torch, z, k):
    """Logical shift right of int64 words."""
    return (z >> k) & ((1 << (64 - k)) - 1)


def pinhole_rays(torch, cam12, width, height, spp, seed, first, count, device="cuda"):
    """Camera rays first .. first + count - 1 of the per-sample frame, in torch on the device: splitmix64 of (seed, G), the seed
    scramble, two XORWOW draws, camera.get_ray in float32 (the frame definition of DESIGN.md section 6; whether the rounding
    of every operation is the kernels' is what `sums_equal_aov` reports)."""
    g = torch.arange(first, first + count, dtype=torch.int64, device=device)
    z = (g + 1) * _u64(0x9E3779B97F4A7C15) + _u64(seed & M64)
    z = (z ^ _lsr(torch, z, 30)) * _u64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(torch, z, 27)) * _u64(0x94D049BB133111EB)
    z = z ^ _lsr(torch, z, 31)
    m = 0xFFFFFFFF
    s0, s1 = (z & m) ^ 0xAAD26B49, (_lsr(torch, z, 32) & m) ^ 0xF7DCEFDD
    t0, t1 = (s0 * 1099087573) & m, (s1 * 2591861531) & m
    d = (6615241 + t1 + t0) & m
    v = [(123456789 + t0) & m, 362436069 ^ t0, (521288629 + t1) & m, 88675123 ^ t1, (5783321 + t0) & m]

    def draw():
        nonlocal d, v
        t = v[0] ^ (v[0] >> 2)
        v4 = (v[4] ^ ((v[4] << 4) & m)) ^ (t ^ ((t << 1) & m))
        v = [v[1], v[2], v[3], v[4], v4]
        d = (d + 362437) & m
        u = ((v4 + d) & m).to(torch.float32)
        return u * np.float32(2.3283064e-10) + np.float32(2.3283064e-10 / 2.0)

    jx, jy = draw(), draw()
    pixel = g // spp
    px, py = (pixel % width).to(torch.float32), (pixel // width).to(torch.float32)
    x, y = ((px + jx) / np.float32(width))[:, None], ((py + jy) / np.float32(height))[:, None]
    c = torch.from_numpy(np.asarray(cam12, np.float32)).to(device)
    lf, ul, hz, vt = c[0:3], c[3:6], c[6:9], c[9:12]
    dr = ((ul + hz * x) + vt * y) - lf
    inv = 1.0 / torch.sqrt((dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1]) + dr[:, 2] * dr[:, 2])
    return lf.expand(count, 3), dr * inv[:, None]


def leg_today(width, height, spp, lib_path):
    """query_closest on a device table + the torch gather and index_add_, on the library at lib_path (or the product's)."""
    import torch
    from rtcuda_amd import api, scenes
    L = None
    if lib_path:
        api._preload_hip_runtime()
        L = ctypes.CDLL(lib_path)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.rt_last_error.restype = ctypes.c_char_p
        L.rt_build_id.restype = ctypes.c_char_p
        L.rt_scene_create_flags.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, ctypes.c_uint32, ctypes.POINTER(vp)]
        L.rt_scene_destroy.argtypes, L.rt_scene_destroy.restype = [vp], None
        L.rt_camera_make.argtypes = [vp, vp, vp, ctypes.c_float, ctypes.c_float, vp]
        L.rt_query_closest_device.argtypes = [vp, ctypes.c_uint32, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    arrays = scenes.cornell_bunny("full_bsdf")
    scene = api.Scene(arrays, library=L)
    cam = np.zeros(12, np.float32)
    a, b, c = (np.asarray(v, np.float32) for v in ((0.5, 0.5, 1.5), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0)))
    assert scene.L.rt_camera_make(a.ctypes.data, b.ctypes.data, c.ctypes.data, 37.8, width / height, cam.ctypes.data) == 0
    n, n_pixels = width * height * spp, width * height
    # ---- before the clock: the ray table, and what a caller keeps per triangle, material and light
    o = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    d = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    step = 1 << 22
    for first in range(0, n, step):
        cnt = min(step, n - first)
        o[first:first + cnt], d[first:first + cnt] = pinhole_rays(torch, cam, width, height, spp, SEED, first, cnt)
    pixel = torch.arange(n, dtype=torch.int64, device="cuda") // spp
    t9 = torch.from_numpy(np.asarray(arrays.tris, np.float32).reshape(-1, 3, 3)).cuda()
    e1, e2 = t9[:, 0] - t9[:, 1], t9[:, 2] - t9[:, 0]
    nrm = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    inv = 1.0 / torch.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
    shade_n = -(nrm * inv[:, None])
    tri_mat = torch.from_numpy(np.asarray(arrays.tri_material, np.int64)).cuda()
    albedo = torch.from_numpy(np.ascontiguousarray(arrays.materials["albedo"])).cuda()
    emission = np.zeros((arrays.n_tris, 3), np.float32)
    lit = np.asarray(arrays.tri_light) >= 0
    emission[lit] = arrays.lights["L"][np.asarray(arrays.tri_light)[lit]]
    emission = torch.from_numpy(emission).cuda()
    hit = torch.empty(n, dtype=torch.int32, device="cuda")
    t = torch.empty(n, dtype=torch.float32, device="cuda")
    sums = torch.zeros((n_pixels, 11), dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def route(flags):
        scene.query_closest_device(o.data_ptr(), d.data_ptr(), 0, n, hit.data_ptr(), t.data_ptr(), flags=flags, stream=st)
        idx = torch.nonzero(hit >= 0).squeeze(1)
        k = hit[idx].long()
        nn = shade_n[k]
        dd = d[idx]
        dot = (nn[:, 0] * dd[:, 0] + nn[:, 1] * dd[:, 1]) + nn[:, 2] * dd[:, 2]
        nn = torch.where((dot > 0)[:, None], -nn, nn)
        vals = torch.cat([albedo[tri_mat[k]], nn, emission[k], t[idx][:, None]], 1)
        fixed = torch.cat([torch.round(vals * 1073741824.0).long(), torch.ones((len(idx), 1), dtype=torch.int64, device="cuda")], 1)
        sums.index_add_(0, pixel[idx], fixed)

    out = {"library": os.path.basename(lib_path) if lib_path else "product", "build_id": scene.L.rt_build_id().decode(),
           "table_bytes": int(o.numel() + d.numel()) * 4}
    for name, flags in (("flags_0", 0), ("watertight", 16)):
        total, query = [], []
        for rep in range(REPS + 1):
            sums.zero_()
            ms_q, _ = _timed(torch, lambda: scene.query_closest_device(o.data_ptr(), d.data_ptr(), 0, n, hit.data_ptr(), t.data_ptr(),
                                                                       flags=flags, stream=st))
            sums.zero_()
            ms, _ = _timed(torch, lambda: route(flags))
            if rep:
                total.append(ms)
                query.append(ms_q)
        out[name] = {"route": _summary(total), "query_alone": _summary(query)}
    ref = os.environ.get("AOV_TIME_SUMS")
    if ref and os.path.exists(ref):  # (the watertight frame of the aov leg)
        out["sums_equal_aov"] = bool(torch.equal(sums.cpu(), torch.load(ref)))
    print(json.dumps(out), flush=True)


def run_child(leg, lib_name=None, lib_path=None, sums_path=None):
    env = dict(os.environ)
    if lib_name:
        env["RT_LIB_NAME"] = lib_name
    if sums_path:
        env["AOV_TIME_SUMS"] = sums_path
    cmd = [sys.executable, os.path.abspath(__file__), "--child", leg] + (["--parent-lib", lib_path] if lib_path else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="library of the parent commit: the `today` leg runs on it")
    ap.add_argument("--no-deposit-lib", help="file name (in rtcuda_amd/) of the variant build without the deposit block")
    ap.add_argument("--per-lane-lib", help="file name (in rtcuda_amd/) of the variant build with one atomic per lane and channel")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aov_time.json"))
    ap.add_argument("--child", choices=["aov", "today"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == "aov":
        return leg_aov(W, H, SPP)
    if a.child == "today":
        return leg_today(W, H, SPP, a.parent_lib)
    sums_path = a.out + ".sums.pt"
    try:
        res = {"scene": "full_bsdf", "frame": [W, H, SPP], "samples": W * H * SPP, "reps": REPS}
        res["aov"] = run_child("aov", sums_path=sums_path)
        res["today"] = run_child("today", lib_path=os.path.abspath(a.parent_lib) if a.parent_lib else None, sums_path=sums_path)
        for k in ("flags_0", "watertight"):
            res[f"today_over_aov_{k}"] = round(res["today"][k]["route"]["ms"] / res["aov"][k]["call"]["ms"], 2)
        if a.no_deposit_lib:
            res["no_deposit"] = run_child("aov", lib_name=a.no_deposit_lib)
            for k in ("flags_0", "watertight"):
                res[f"deposit_share_{k}"] = round(1.0 - res["no_deposit"][k]["kernel"]["ms"] / res["aov"][k]["kernel"]["ms"], 3)
        if a.per_lane_lib:
            res["per_lane_atomics"] = run_child("aov", lib_name=a.per_lane_lib)
            for k in ("flags_0", "watertight"):
                res[f"per_lane_over_product_{k}"] = round(res["per_lane_atomics"][k]["kernel"]["ms"] / res["aov"][k]["kernel"]["ms"], 2)
    finally:
        if os.path.exists(sums_path):
            os.remove(sums_path)
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
