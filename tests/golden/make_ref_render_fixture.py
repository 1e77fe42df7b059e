#!/usr/bin/env python3
"""Regenerates tests/golden/ref_render_fixture.npz from the REFERENCE'S OWN render() (only where /root/reference exists).

`make -C oracle _ref_render` compiles oracle/ref_render_driver.cpp (own code) against the reference's device headers --
included by path, unmodified, under oracle/ref_shim.h; render.cuh as a launch-rewritten temporary copy -- into
oracle/_ref/ref_render (git-ignored).  This script writes every frame of tests/shade_scenes.py FRAMES as a plain binary
scene description into oracle/_ref/, runs the driver on all of them, and stores per frame the inputs as written (the scene
arrays, camera parameters, w, h, spp, max_bounces, seed) and the driver's outputs: the Camera the reference's constructor
made, the raw fp32 sums, the post-processed image, the per-iteration (mat, gen, ah, ch) queue counts and the emission /
any-hit / closest-hit-shadow deposit counts.  Numbers only.

It fails unless every frame has at most 1 non-finite pixel in 10^4 (the reference's estimator has no guard against NaN).
What the fixture pins: the oracle's literal render, bit for bit (tests/test_ref_render_pins.py), and through it and directly
the default kernels on the GPU (tests/test_gpu_ref_render.py).
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF", "/root/reference")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
MAGIC = 0x52454652


def write_scene(path, d):
    w, h, spp, max_bounces, seed = (int(x) for x in d["params"])
    with open(path, "wb") as f:
        f.write(np.array([MAGIC, len(d["tris"]), len(d["materials"]), len(d["lights"]), w, h, spp, max_bounces, seed], "<i4").tobytes())
        for key, dtype in (("tris", "<f4"), ("tri_material", "<i4"), ("tri_light", "<i4"), ("materials", "u1"), ("lights", "u1"),
                           ("camera_params", "<f4")):
            f.write(np.ascontiguousarray(d[key], dtype).tobytes())


def read_output(path):
    b = open(path, "rb").read()
    magic, w, h, n_iter = np.frombuffer(b, "<i4", 4)
    assert magic == MAGIC
    off = 16

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(b, dtype, count, off)
        off += a.nbytes
        return a.copy()
    out = {"cam12": take("<f4", 12), "sums": take("<f4", 3 * w * h).reshape(h, w, 3), "image": take("<f4", 3 * w * h).reshape(h, w, 3),
           "iter_counts": take("<i4", 4 * n_iter).reshape(n_iter, 4), "deposits": take("<i8", 3)}
    assert off == len(b), (off, len(b))
    return out


def make(out_path):
    import shade_scenes as ss
    if not os.path.isdir(REF):
        raise SystemExit(f"{REF} does not exist: the fixture can only be regenerated where the reference is present")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "_ref_render", f"REF={REF}"], stdout=subprocess.DEVNULL)
    ref = os.path.join(ROOT, "oracle", "_ref")
    frames = {name: ss.frame_arrays(name) for name in ss.FRAMES}
    args = []
    for name, d in sorted(frames.items(), key=lambda kv: int(kv[1]["params"][4])):   # by seed: the driver keeps one seed's states
        src, dst = os.path.join(ref, f"render_{name}.scene.bin"), os.path.join(ref, f"render_{name}.out.bin")
        write_scene(src, d)
        args += [src, dst]
    subprocess.check_call([os.path.join(ref, "ref_render")] + args)
    store = {"frames": np.array(list(ss.FRAMES))}
    over = []
    for name, d in frames.items():
        o = read_output(os.path.join(ref, f"render_{name}.out.bin"))
        bad = int((~np.isfinite(o["image"])).any(axis=2).sum())
        npix = o["image"].shape[0] * o["image"].shape[1]
        print(f"{name:18s} {npix:5d} px, {len(o['iter_counts']):3d} iterations, sums of (mat, gen, ah, ch) {o['iter_counts'].sum(axis=0).tolist()}, "
              f"deposits {o['deposits'].tolist()}, non-finite pixels {bad}, mean {np.nanmean(o['image']):.4f}")
        if bad * 10000 > npix:
            over.append(f"{name}: {bad} non-finite pixels of {npix}")
        for k, v in {**d, **o}.items():
            store[f"{name}__{k}"] = v
    if over:
        raise SystemExit("above 1 non-finite pixel in 10^4 -- choose other scenes or seeds:\n  " + "\n  ".join(over))
    ss.save_npz(out_path, store)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    make(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ref_render_fixture.npz"))
