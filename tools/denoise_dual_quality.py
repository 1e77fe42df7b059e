"""Where the defaults of rt_denoise_dual_fixed come from: a sweep of its four parameters on the CPU, written to
profiles/denoise_dual_quality.json.  No GPU.  Frames, 1024-spp references, metrics and selection rule are those of
tools/denoise_quality.py (full_bsdf, 64x48 and 192x144, 4 and 16 spp; rms and relmse as ratios denoised / noisy; the defaults are
the set with the lowest geometric mean of the four relmse ratios among the sets whose rms ratio is below 1 on both 64x48 frames).
The two half frames are the oracle's per-sample frames of shard (0, 2) and (1, 2) -- what rt_render_shard_fixed leaves with
RT_FLAG_RNG_PER_SAMPLE for rank r of 2 -- and are asserted to sum to the whole frame; the filter is the CPU twin hc_denoise_dual
(the kernels' arithmetic, bit for bit).  For comparison the file also records rt_denoise_fixed at ITS defaults on the summed
frames (`rt_denoise_fixed_defaults`; the same numbers as profiles/denoise_quality.json's defaults).

    python tools/denoise_dual_quality.py [--out profiles/denoise_dual_quality.json]
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

FRAMES = ((64, 48, 4), (64, 48, 16), (192, 144, 4), (192, 144, 16))
REFERENCE_SPP, REFERENCE_SEED = 1024, 2
GRID = dict(passes=(2, 3, 4, 5), sigma_variance=(0.5, 1.0, 2.0, 4.0, 8.0), sigma_depth=(0.03125, 0.125, 0.5),
            normal_power_log2=(1, 3, 5))


def twins():
    from rtcuda_amd import api
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.hc_denoise_dual.argtypes = [vp, ci, vp, ci, vp, ci, ci, ci, ci, cf, cf, ci, vp, vp]
    L.hc_denoise.argtypes = [vp, ci, vp, ci, ci, ci, ci, cf, cf, ci, vp]

    def dual(a, spp_a, b, spp_b, aov, aov_spp, w, h, passes, sigma_variance, sigma_depth, normal_power_log2):
        a, b, aov = (np.ascontiguousarray(t, np.int64) for t in (a, b, aov))
        out = np.zeros((w * h, 3), np.float32)
        rc = L.hc_denoise_dual(a.ctypes.data, spp_a, b.ctypes.data, spp_b, aov.ctypes.data, aov_spp, w, h, passes, sigma_variance,
                               sigma_depth, normal_power_log2, out.ctypes.data, None)
        assert rc == 0, "hc_denoise_dual refused its arguments"
        return out

    def single(beauty, spp, aov, aov_spp, w, h):
        p = api.denoise_default_params()
        beauty, aov = np.ascontiguousarray(beauty, np.int64), np.ascontiguousarray(aov, np.int64)
        out = np.zeros((w * h, 3), np.float32)
        rc = L.hc_denoise(beauty.ctypes.data, spp, aov.ctypes.data, aov_spp, w, h, p["passes"], p["sigma_color"], p["sigma_depth"],
                          p["normal_power_log2"], out.ctypes.data)
        assert rc == 0, "hc_denoise refused its arguments"
        return out, p
    return dual, single


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def relmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.mean((a - b) ** 2 / (b ** 2 + 0.01)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_dual_quality.json"))
    args = ap.parse_args()
    import aov_expected as ae
    import denoise_expected as de
    from oracle.oracle import Oracle, build, usable_cpus
    from rtcuda_amd import scenes
    build()
    orc = Oracle("pinned")
    osc = orc.scene(scenes.cornell_bunny("full_bsdf")).set_watertight(True)
    dual, single = twins()
    frames, refs = [], {}
    for w, h, spp in FRAMES:
        cam = orc.camera((0.5, 0.5, 1.5), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8, w / h)
        if (w, h) not in refs:
            fixed = np.zeros((h, w, 3), np.int64)  # (the fixed-point sums: a sample that is not finite deposits nothing there)
            osc.render(cam, w, h, REFERENCE_SPP, seed=REFERENCE_SEED, threads=usable_cpus(), fixed_out=fixed, rng_mode="per_sample")
            refs[(w, h)] = fixed.reshape(-1, 3).astype(np.float64) * (2.0 ** -30 / REFERENCE_SPP)
        beauty = np.zeros((h, w, 3), np.int64)
        osc.render(cam, w, h, spp, threads=usable_cpus(), fixed_out=beauty, rng_mode="per_sample")
        aov = ae.frame_expected(orc, osc, cam, w, h, spp)[0]
        beauty = beauty.reshape(-1, 3)
        halves = []
        for r in (0, 1):
            half = np.zeros((h, w, 3), np.int64)
            osc.render(cam, w, h, spp, threads=usable_cpus(), fixed_out=half, rng_mode="per_sample", shard=(r, 2))
            halves.append(half.reshape(-1, 3))
        assert np.array_equal(halves[0] + halves[1], beauty), "the two half frames do not sum to the whole frame"
        noisy = de.noisy_mean(beauty, spp)
        frames.append((w, h, spp, beauty, aov, rms(noisy, refs[(w, h)]), relmse(noisy, refs[(w, h)]), halves))
        print(f"{w}x{h}x{spp}: noisy frame rms {frames[-1][5]:.5f} relmse {frames[-1][6]:.5f}", flush=True)
    rows = []
    for p, sc, sd, npw in itertools.product(*(GRID[k] for k in ("passes", "sigma_variance", "sigma_depth", "normal_power_log2"))):
        outs = [dual(hv[0], spp // 2, hv[1], spp // 2, a, spp, w, h, p, sc, sd, npw) for w, h, spp, _, a, _, _, hv in frames]
        r_rms = [rms(o, refs[f[:2]]) / f[5] for o, f in zip(outs, frames)]
        r_rel = [relmse(o, refs[f[:2]]) / f[6] for o, f in zip(outs, frames)]
        rows.append(dict(passes=p, sigma_variance=sc, sigma_depth=sd, normal_power_log2=npw, rms_ratios=[round(r, 4) for r in r_rms],
                         relmse_ratios=[round(r, 4) for r in r_rel], score=round(float(np.exp(np.mean(np.log(r_rel)))), 4)))
    rows.sort(key=lambda r: r["score"])
    small = [k for k, f in enumerate(frames) if f[:2] == (64, 48)]
    best = next(r for r in rows if all(r["rms_ratios"][k] < 1 for k in small))
    print("best:", best, flush=True)
    fixed_outs, fixed_prm = zip(*(single(b, spp, a, spp, w, h) for w, h, spp, b, a, _, _, _ in frames))
    f_rms = [rms(o, refs[f[:2]]) / f[5] for o, f in zip(fixed_outs, frames)]
    f_rel = [relmse(o, refs[f[:2]]) / f[6] for o, f in zip(fixed_outs, frames)]
    fixed = dict(params=fixed_prm[0], rms_ratios=[round(r, 4) for r in f_rms], relmse_ratios=[round(r, 4) for r in f_rel],
                 score=round(float(np.exp(np.mean(np.log(f_rel)))), 4))
    print("rt_denoise_fixed at its defaults on the summed frames:", fixed, flush=True)
    from rtcuda_amd import api
    doc = dict(scene="full_bsdf", build_id=api.build_id(), halves="the oracle's per-sample frames of shard (0, 2) and (1, 2); they sum to the whole frame", frames=[list(f[:3]) for f in frames], reference_spp=REFERENCE_SPP, reference_seed=REFERENCE_SEED,
               metric="ratios are denoised / noisy against the reference frame, linear mean radiance; rms over pixels and channels; "
                      "relmse = mean of (x - ref)^2 / (ref^2 + 0.01); score = geometric mean of the four relmse ratios; defaults = "
                      "lowest score among the rows with both 64x48 rms ratios below 1",
               noisy_rms=[round(f[5], 6) for f in frames], noisy_relmse=[round(f[6], 6) for f in frames],
               grid={k: list(v) for k, v in GRID.items()},
               defaults={k: best[k] for k in ("passes", "sigma_variance", "sigma_depth", "normal_power_log2")},
               default_rms_ratios=best["rms_ratios"], default_relmse_ratios=best["relmse_ratios"], default_score=best["score"],
               rt_denoise_fixed_defaults=fixed, beats_rt_denoise_fixed=bool(best["score"] < fixed["score"]), table=rows)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
