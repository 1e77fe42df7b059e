"""What temporal accumulation buys, and where the defaults of rt_temporal_accumulate_fixed come from: two 8-frame sequences on
the CPU, written to profiles/temporal_quality.json.  No GPU: frames are the oracle's, the motion records, the accumulator and the
denoiser are the CPU twins (hc_motion_records, hc_temporal_accumulate, hc_denoise_dual: the kernels' arithmetic, bit for bit).

Scene full_bsdf at 64x48 and 192x144, 4 spp per frame as two 2-spp halves (shards (0, 2) and (1, 2) of the per-sample frame), a
new seed per frame, one AOV frame per frame.  Sequence `orbit`: the camera orbits the box by ORBIT_DEGREES per frame.  Sequence
`bunny`: the camera stands still and the bunny translates by BUNNY_STEP per frame, the previous frame's vertices handed over.
The LAST frame is compared against the oracle's 1024-spp frame of that view, with the metric of tools/denoise_dual_quality.py
(rms over pixels and channels; relmse = mean of (x - ref)^2 / (ref^2 + 0.01); ratios against the noisy frame), for four cases:
the noisy frame, denoise_dual alone, accumulation alone (the sum of the two accumulated halves, 2 samples of the accumulated mean),
accumulation then denoise_dual(hist_a, 1, hist_b, 1).  The defaults are the set with the lowest geometric mean of the four relmse
ratios of the last case among the sets whose rms ratio is below 1 on both 64x48 sequences -- that file's selection rule.  No ratio
is fixed in advance.

    python tools/temporal_quality.py [--out profiles/temporal_quality.json] [--small]
"""
import argparse
import ctypes
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((64, 48), (192, 144))
FRAMES, SPP = 8, 4
REFERENCE_SPP, REFERENCE_SEED = 1024, 2
ORBIT_DEGREES = 2.0
BUNNY_STEP = (0.01, 0.0, -0.005)
GRID = dict(max_history=(4, 8, 16, 32), alpha_min=(0.03125, 0.0625, 0.125, 0.25), depth_tolerance=(0.03125, 0.125), normal_cos_min=(0.5, 0.875))


def twins():
    from rtcuda_amd import api
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.hc_denoise_dual.argtypes = [vp, ci, vp, ci, vp, ci, ci, ci, ci, cf, cf, ci, vp, vp]
    L.hc_motion_records.argtypes = [ci, vp, vp, vp, vp, ci, vp, ci, ci, vp]
    L.hc_temporal_accumulate.argtypes = [vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, cf, cf, cf, vp, vp, vp]
    dp = api.denoise_dual_default_params()

    def dual(a, spp_a, b, spp_b, aov, aov_spp, w, h):
        a, b, aov = (np.ascontiguousarray(t, np.int64) for t in (a, b, aov))
        out = np.zeros((w * h, 3), np.float32)
        assert L.hc_denoise_dual(a.ctypes.data, spp_a, b.ctypes.data, spp_b, aov.ctypes.data, aov_spp, w, h, dp["passes"], dp["sigma_variance"],
                                 dp["sigma_depth"], dp["normal_power_log2"], out.ctypes.data, None) == 0
        return out

    def motion(tri, u, v, prev_tris, prev_cam, w, h):
        tri, u, v = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
        prev_tris, prev_cam = np.ascontiguousarray(prev_tris, np.float32).reshape(-1, 9), np.ascontiguousarray(prev_cam, np.float32)
        out = np.zeros((tri.size, 4), np.float32)
        assert L.hc_motion_records(tri.size, tri.ctypes.data, u.ctypes.data, v.ctypes.data, prev_tris.ctypes.data, prev_tris.shape[0],
                                   prev_cam.ctypes.data, w, h, out.ctypes.data) == 0
        return out

    def accumulate(a, b, aov, mo, hist, w, h, prm):
        n = w * h
        oa, ob, ol = np.zeros((n, 3), np.int64), np.zeros((n, 3), np.int64), np.zeros(n, np.int32)
        hp = [None] * 4 if hist is None else [x.ctypes.data for x in hist]
        assert L.hc_temporal_accumulate(a.ctypes.data, SPP // 2, b.ctypes.data, SPP // 2, aov.ctypes.data, SPP, mo.ctypes.data, hp[0], hp[1], hp[2], hp[3], SPP,
                                        w, h, prm["max_history"], prm["alpha_min"], prm["depth_tolerance"], prm["normal_cos_min"], oa.ctypes.data,
                                        ob.ctypes.data, ol.ctypes.data) == 0
        return oa, ob, ol
    return dual, motion, accumulate


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def relmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.mean((a - b) ** 2 / (b ** 2 + 0.01)))


def mean_of(sums, spp):
    return np.asarray(sums, np.int64).astype(np.float64) * (2.0 ** -30 / spp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_quality.json"))
    ap.add_argument("--small", action="store_true", help="64x48 only (a quick look; the committed file has both sizes)")
    args = ap.parse_args()
    import aov_expected as ae
    import temporal_expected as te
    from oracle.oracle import Oracle, build, usable_cpus
    from rtcuda_amd import api, scenes
    build()
    orc = Oracle("pinned")
    base = scenes.cornell_bunny("full_bsdf")
    dual, motion, accumulate = twins()
    threads = usable_cpus()

    def camera(k, aspect, orbit):
        a = np.deg2rad(ORBIT_DEGREES * k) if orbit else 0.0
        return orc.camera((0.5 + 1.5 * np.sin(a), 0.5, 1.5 * np.cos(a)), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8, aspect)

    sequences = []  # (name, w, h, frames [(a, b, aov, motion)], reference mean, noisy rms, noisy relmse, denoise_dual alone)
    for (w, h), name in itertools.product(SIZES[:1] if args.small else SIZES, ("orbit", "bunny")):
        frames, prev_cam, prev_tris, osc = [], None, None, None
        for k in range(FRAMES):
            arrays = base if name == "orbit" else te.moved_arrays(base, tuple(k * s for s in BUNNY_STEP))
            if osc is None or name == "bunny":
                osc = orc.scene(arrays).set_watertight(True)
            cam = camera(k, w / h, name == "orbit")
            halves = []
            for r in (0, 1):
                half = np.zeros((h, w, 3), np.int64)
                osc.render(cam, w, h, SPP, seed=100 + k, threads=threads, fixed_out=half, rng_mode="per_sample", shard=(r, 2))
                halves.append(half.reshape(-1, 3))
            aov = ae.frame_expected(orc, osc, cam, w, h, SPP, seed=100 + k)[0]
            o, d = te.centre_rays(orc, cam, w, h)
            tri, _, u, v = osc.trace_closest(o, d, np.full(w * h, te.FLT_MAX, np.float32), threads=threads)
            mo = motion(tri, u, v, arrays.tris if prev_tris is None else prev_tris, cam if prev_cam is None else prev_cam, w, h)
            frames.append((halves[0], halves[1], aov, mo))
            prev_cam, prev_tris = cam, arrays.tris
        fixed = np.zeros((h, w, 3), np.int64)
        osc.render(cam, w, h, REFERENCE_SPP, seed=REFERENCE_SEED, threads=threads, fixed_out=fixed, rng_mode="per_sample")
        ref = mean_of(fixed.reshape(-1, 3), REFERENCE_SPP)
        a, b, aov, _ = frames[-1]
        noisy = mean_of(a + b, SPP)
        alone = dual(a, SPP // 2, b, SPP // 2, aov, SPP, w, h)
        sequences.append((name, w, h, frames, ref, rms(noisy, ref), relmse(noisy, ref), alone))
        print(f"{name} {w}x{h}: noisy rms {sequences[-1][5]:.5f} relmse {sequences[-1][6]:.5f}; denoise_dual alone rms ratio "
              f"{rms(alone, ref) / sequences[-1][5]:.4f} relmse ratio {relmse(alone, ref) / sequences[-1][6]:.4f}", flush=True)

    def run(prm, detail=False):
        out = []
        for name, w, h, frames, ref, n_rms, n_rel, _ in sequences:
            hist = None
            for a, b, aov, mo in frames:
                oa, ob, ol = accumulate(a, b, aov, mo, hist, w, h, prm)
                hist = (oa, ob, ol, aov)
            acc = mean_of(oa + ob, 2)
            both = dual(oa, 1, ob, 1, aov, SPP, w, h)
            out.append(dict(kept=round(float(np.mean(ol > 1)), 4), mean_len=round(float(np.mean(ol)), 3),
                            acc_rms=round(rms(acc, ref) / n_rms, 4), acc_relmse=round(relmse(acc, ref) / n_rel, 4),
                            both_rms=round(rms(both, ref) / n_rms, 4), both_relmse=round(relmse(both, ref) / n_rel, 4)))
            if detail:  # where the accumulated frame's relmse sits: its worst 0.5 % of pixels, and how many of those touch an emitter
                e = ((acc - ref) ** 2 / (ref ** 2 + 0.01)).sum(axis=1)
                worst = np.argsort(e)[::-1][:max(w * h // 200, 1)]
                lit = (aov[:, ae.EMISSION:ae.EMISSION + 3] > 0).any(axis=1).reshape(h, w)
                near = np.zeros_like(lit)
                for dy, dx in itertools.product(range(-2, 3), repeat=2):
                    near[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] |= lit[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
                out[-1].update(acc_relmse_share_of_worst_half_percent=round(float(e[worst].sum() / e.sum()), 4),
                               worst_within_2_pixels_of_an_emitter=round(float(near.reshape(-1)[worst].mean()), 4))
        return out

    rows = []
    for mh, am, dt, nc in itertools.product(*(GRID[k] for k in ("max_history", "alpha_min", "depth_tolerance", "normal_cos_min"))):
        if am > 1.0 / mh * 4:  # (the floor already caps the history well below max_history: the same filter as a smaller max_history)
            continue
        res = run(dict(max_history=mh, alpha_min=am, depth_tolerance=dt, normal_cos_min=nc))
        rows.append(dict(max_history=mh, alpha_min=am, depth_tolerance=dt, normal_cos_min=nc, sequences=res,
                         score=round(float(np.exp(np.mean(np.log([r["both_relmse"] for r in res])))), 4)))
    rows.sort(key=lambda r: r["score"])
    small = [k for k, s in enumerate(sequences) if s[1:3] == (64, 48)]
    best = next(r for r in rows if all(r["sequences"][k]["both_rms"] < 1 for k in small))
    print("best:", best, flush=True)
    detail = run({k: best[k] for k in GRID}, detail=True)
    alone_score = round(float(np.exp(np.mean(np.log([relmse(s[7], s[4]) / s[6] for s in sequences])))), 4)
    doc = dict(scene="full_bsdf", build_id=api.build_id(), frames_per_sequence=FRAMES, spp_per_frame=SPP,
               halves="the oracle's per-sample frames of shard (0, 2) and (1, 2), seed 100 + frame", reference_spp=REFERENCE_SPP, reference_seed=REFERENCE_SEED,
               orbit_degrees_per_frame=ORBIT_DEGREES, bunny_step_per_frame=list(BUNNY_STEP),
               sequences=[dict(name=s[0], width=s[1], height=s[2], noisy_rms=round(s[5], 6), noisy_relmse=round(s[6], 6),
                               denoise_dual_alone_rms=round(rms(s[7], s[4]) / s[5], 4), denoise_dual_alone_relmse=round(relmse(s[7], s[4]) / s[6], 4)) for s in sequences],
               metric="the last frame against the reference of its view, linear mean radiance; ratios are against the noisy 4-spp frame; rms over pixels "
                      "and channels; relmse = mean of (x - ref)^2 / (ref^2 + 0.01); acc = the two accumulated halves summed; both = denoise_dual(hist_a, 1, "
                      "hist_b, 1) at its defaults; kept = share of pixels of the last frame with len > 1; score = geometric mean of the both_relmse "
                      "ratios; defaults = lowest score among the rows whose both_rms is below 1 on both 64x48 sequences",
               denoise_dual_params=api.denoise_dual_default_params(), grid={k: list(v) for k, v in GRID.items()},
               defaults={k: best[k] for k in ("max_history", "alpha_min", "depth_tolerance", "normal_cos_min")}, default_sequences=detail,
               default_score=best["score"], denoise_dual_alone_score=alone_score, accumulation_lowers_the_score=bool(best["score"] < alone_score),
               table=rows)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
