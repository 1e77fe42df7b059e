#!/usr/bin/env python3
"""What a ray query costs (rt_query_closest_device / rt_query_any_device), one JSON line per scene and ray kind.

2^22 rays per call on full_bsdf (C2) and four_bunnies: coherent camera rays, their bounce rays (closest hit) and
shadow-style rays (any hit: bounce rays, tmax uniform in (0.05, 1.2), nothing excluded).  Warm, median of 7.

  device_ms    HIP events around the query with the rays already resident on the device; Mrays_s from it
  hook_ms      (--parent-lib PATH) wall time of rt_trace_*_flags on the same rays from HOST memory in the library at PATH (the
               parent commit's build), loaded in a child process of its own, one repetition at a time in turn with the
               device path: what the same answer cost before the query entry points existed
  kernel_ms    (--trace-dir DIR) duration of the k_query dispatches, and with --parent-lib of that library's k_trace test-mode
               dispatches, on the same rays: each from a rocprofv3 --kernel-trace run of its own (no counters), 7 repetitions
               after a warm-up; `kernel_spread_parent_ms` = max - min of the parent's 7, the margin k_query is held to

The hooks have since become the host-pointer form of the queries (upload, k_query, download) and k_trace walks pools only:
hook_ms, and the `k_trace<` dispatches kernel_parent_ms is made from, mean what is said above only with --parent-lib of a commit
up to 78db776, where the hooks still ran k_trace's dense-array modes.  A later library's hook launches k_query and no k_trace.

  python tools/query_time.py --parent-lib <parent build>/librtcuda_amd.so --trace-dir <dir> --out profiles/query_time.json
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

N = 1 << 22
REPS = 7
BATCHES = ("camera", "bounce", "any")
FLT_MAX = np.float32(3.4028234663852886e38)


def make_rays(scene, path):
    """The three batches of a scene, as float32 arrays in an .npz (the child processes trace the very same rays)."""
    import torch
    import raygen
    from rtcuda_amd import api
    o, d = raygen.camera_rays(api.make_camera(aspect=16 / 9), 1920, 1080, N, seed=11)
    hit, t, _, _ = scene.query_closest(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
    hit, t = hit.cpu().numpy(), t.cpu().numpy()
    o2, d2 = raygen.bounce_rays(o, d, t, hit >= 0, seed=12)
    idx = np.arange(N) % len(o2)  # (about half of the camera rays hit: tiled to the full count)
    o2, d2 = np.ascontiguousarray(o2[idx]), np.ascontiguousarray(d2[idx])
    tm = np.random.default_rng(13).uniform(0.05, 1.2, N).astype(np.float32)
    np.savez(path, camera_o=o, camera_d=d, bounce_o=o2, bounce_d=d2, any_o=o2, any_d=d2, any_tmax=tm,
             camera_hit_share=np.float64((hit >= 0).mean()))


class DevicePath:
    def __init__(self, scene, rays):
        import torch
        self.torch, self.scene = torch, scene
        self.r = {k: torch.from_numpy(rays[k]).cuda() for k in rays.files if rays[k].ndim > 0}
        self.hit = torch.empty(N, dtype=torch.int32, device="cuda")
        self.t, self.u, self.v = (torch.empty(N, dtype=torch.float32, device="cuda") for _ in range(3))

    def run(self, batch):
        """One query; device milliseconds between two events on the current stream."""
        torch, r = self.torch, self.r
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st = torch.cuda.current_stream().cuda_stream
        e0.record()
        if batch == "any":
            self.scene.query_any_device(r["any_o"].data_ptr(), r["any_d"].data_ptr(), r["any_tmax"].data_ptr(), 0, N, self.hit.data_ptr(),
                                        stream=st)
        else:
            self.scene.query_closest_device(r[batch + "_o"].data_ptr(), r[batch + "_d"].data_ptr(), 0, N, self.hit.data_ptr(),
                                            self.t.data_ptr(), self.u.data_ptr(), self.v.data_ptr(), stream=st)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)


class HookPath:
    def __init__(self, scene, rays):
        self.scene, self.r = scene, rays
        self.full = np.full(N, FLT_MAX, np.float32)
        self.none = np.full(N, -1, np.int32)

    def run(self, batch):
        """One call of the host-pointer hook; wall milliseconds."""
        r = self.r
        t0 = time.perf_counter()
        if batch == "any":
            self.scene.trace_any(r["any_o"], r["any_d"], r["any_tmax"], self.none)
        else:
            self.scene.trace_closest(r[batch + "_o"], r[batch + "_d"], self.full)
        return 1e3 * (time.perf_counter() - t0)


def hooks_library(path):
    """The library at `path` with the handful of entry points the hook path calls bound by hand: a build of the parent commit
    has no rt_query_* symbols, so api.lib()'s binding of the whole C-ABI does not apply to it.  None: the product library."""
    if not path:
        return None
    import ctypes
    from rtcuda_amd import api
    api._preload_hip_runtime()
    L = ctypes.CDLL(path)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.rt_last_error.restype = ctypes.c_char_p
    L.rt_scene_create_flags.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, ctypes.c_uint32, ctypes.POINTER(vp)]
    L.rt_scene_destroy.argtypes, L.rt_scene_destroy.restype = [vp], None
    L.rt_trace_closest.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
    L.rt_trace_any.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    return L


def child(variant, rays_path, path):
    """A process of its own, on the library QUERY_TIME_LIB names (the hook path) or the product library.  `serve`: one
    repetition of the named batch per line read, its milliseconds written back.  `replay`: warm-up + REPS of every batch in order (what a kernel trace is taken of)."""
    from rtcuda_amd import api, scenes
    scene = api.Scene(scenes.cornell_bunny(variant), library=hooks_library(os.environ.get("QUERY_TIME_LIB")))
    rays = np.load(rays_path)
    runner = (DevicePath if path.endswith("device") else HookPath)(scene, rays)
    if path.startswith("replay"):
        for batch in BATCHES:
            for _ in range(REPS + 1):
                runner.run(batch)
        return
    print("ready", flush=True)
    for line in sys.stdin:
        print(runner.run(line.strip()), flush=True)


def spawn(args, lib, **kw):
    env = dict(os.environ)
    if lib:
        env["QUERY_TIME_LIB"] = os.path.abspath(lib)
    return subprocess.Popen(args, env=env, text=True, **kw)


def kernel_times(trace_dir, tag, variant, rays_path, path, lib, pattern):
    """{batch: [ms of each of the REPS dispatches]} of the kernels whose name contains `pattern`, from a kernel trace of a
    replay child."""
    out_dir = os.path.join(trace_dir, f"{variant}_{tag}")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__),
           "--child", variant, rays_path, path]
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "rocprofv3.log"), "w") as log:
        p = spawn(cmd, lib, stdout=log, stderr=subprocess.STDOUT)
        try:
            rc = p.wait(timeout=400)
        except subprocess.TimeoutExpired:
            p.kill()
            raise
        if rc != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed: see {out_dir}/rocprofv3.log")
    rows = []
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f, newline="") as fh:
            rows += [r for r in csv.DictReader(fh) if pattern in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows]
    if len(ms) != len(BATCHES) * (REPS + 1):
        raise RuntimeError(f"{out_dir}: {len(ms)} dispatches of {pattern}, expected {len(BATCHES) * (REPS + 1)}")
    return {b: ms[k * (REPS + 1) + 1:(k + 1) * (REPS + 1)] for k, b in enumerate(BATCHES)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="library of the parent commit: hook_ms and the k_trace kernel times come from it")
    ap.add_argument("--trace-dir", help="directory for the rocprofv3 kernel traces (kernel_ms)")
    ap.add_argument("--out", help="also write all lines, with the build id, to this JSON file")
    ap.add_argument("--scenes", default="full_bsdf,four_bunnies")
    ap.add_argument("--child", nargs=3, metavar=("SCENE", "RAYS", "PATH"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    import torch
    from rtcuda_amd import api, scenes
    assert torch.cuda.is_available(), "query_time.py measures on a GPU"
    lines = []
    tmp = tempfile.mkdtemp(prefix="query_time_")
    for variant in a.scenes.split(","):
        arrays = scenes.cornell_bunny(variant)
        scene = api.Scene(arrays)
        rays_path = os.path.join(tmp, variant + ".npz")
        make_rays(scene, rays_path)
        rays = np.load(rays_path)
        dev = DevicePath(scene, rays)
        hook = None
        if a.parent_lib:
            hook = spawn([sys.executable, os.path.abspath(__file__), "--child", variant, rays_path, "serve-hook"], a.parent_lib,
                         stdin=subprocess.PIPE, stdout=subprocess.PIPE)
            assert hook.stdout.readline().strip() == "ready"
        device_ms = {b: [] for b in BATCHES}
        hook_ms = {b: [] for b in BATCHES}
        for rep in range(REPS + 1):  # (the first repetition warms both paths up and is dropped)
            for b in BATCHES:
                ms = dev.run(b)
                if rep:
                    device_ms[b].append(ms)
                if hook:
                    hook.stdin.write(b + "\n")
                    hook.stdin.flush()
                    ms = float(hook.stdout.readline())
                    if rep:
                        hook_ms[b].append(ms)
        if hook:
            hook.stdin.close()
            hook.wait(timeout=60)
        k_new = k_old = k_error = None
        if a.trace_dir:
            try:
                k_new = kernel_times(a.trace_dir, "new", variant, rays_path, "replay-device", None, "k_query<")
                if a.parent_lib:
                    k_old = kernel_times(a.trace_dir, "parent", variant, rays_path, "replay-hook", a.parent_lib, "k_trace<")
            except (RuntimeError, KeyError, subprocess.TimeoutExpired) as e:
                k_error = str(e)  # (reported with the lines: the device and hook times stand on their own)
        for b in BATCHES:
            med = statistics.median(device_ms[b])
            line = {"scene": variant, "tris": arrays.n_tris, "batch": b, "rays": N, "device_ms": round(med, 4),
                    "device_ms_min_max": [round(min(device_ms[b]), 4), round(max(device_ms[b]), 4)], "Mrays_s": round(N / med / 1e3, 1)}
            if b == "camera":
                line["hit_share"] = round(float(rays["camera_hit_share"]), 4)
            if hook:
                line["hook_ms"] = round(statistics.median(hook_ms[b]), 2)
                line["hook_over_device"] = round(line["hook_ms"] / med, 1)
            if k_error:
                line["kernel_error"] = k_error
            if k_new:
                line["kernel_ms"] = round(statistics.median(k_new[b]), 4)
            if k_old:
                line["kernel_parent_ms"] = round(statistics.median(k_old[b]), 4)
                line["kernel_spread_parent_ms"] = round(max(k_old[b]) - min(k_old[b]), 4)
                line["kernel_within_margin"] = bool(line["kernel_ms"] <= line["kernel_parent_ms"] + line["kernel_spread_parent_ms"])
            print(json.dumps(line), flush=True)
            lines.append(line)
        scene.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "reps": REPS, "lines": lines}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
