"""Where the defaults of rt_denoise_fixed come from: a sweep of its four parameters on the CPU, written to
profiles/denoise_quality.json.  No GPU: the beauty sums are the oracle's per-sample frames (what rt_render_shard_fixed leaves
with RT_FLAG_RNG_PER_SAMPLE), the AOV sums tests/aov_expected.frame_expected (what rt_render_aov_fixed leaves), the filter the CPU
twin hc_denoise (the kernels' arithmetic, bit for bit).  full_bsdf, 64x48 and 192x144, 4 and 16 spp, against the oracle's frame
of the same view at 1024 spp (another seed); all frames are LINEAR mean radiance.  Two errors per frame, each as the ratio
denoised / noisy:
  rms     the RMS difference over all pixels and channels.  On this scene 94 % to 99.9 % of it sits in 1 % of the pixels: the
          anti-aliased edge of the light (first-hit emission, which the filter leaves alone by design) and, at 192x144, fireflies
          of the 1024-spp frame itself.  It says whether the filter does harm there; it cannot rank parameter sets.
  relmse  the mean over pixels and channels of (x - ref)^2 / (ref^2 + 0.01): the usual firefly-robust error of denoising papers.
The defaults are the set with the lowest geometric mean of the four relmse ratios among the sets whose rms ratio is below 1 on
both 64x48 frames (what tests/test_denoise_host.py asserts of the defaults).

    python tools/denoise_quality.py [--out profiles/denoise_quality.json]
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
GRID = dict(passes=(2, 3, 4, 5), sigma_color=(0.03125, 0.0625, 0.125, 0.25, 0.5, 1.0, 2.0), sigma_depth=(0.03125, 0.125, 0.5),
            normal_power_log2=(1, 3, 5))


def twin():
    from rtcuda_amd import api
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.hc_denoise.argtypes = [vp, ci, vp, ci, ci, ci, ci, cf, cf, ci, vp]

    def run(beauty, spp, aov, aov_spp, w, h, passes, sigma_color, sigma_depth, normal_power_log2):
        beauty, aov = np.ascontiguousarray(beauty, np.int64), np.ascontiguousarray(aov, np.int64)
        out = np.zeros((w * h, 3), np.float32)
        rc = L.hc_denoise(beauty.ctypes.data, spp, aov.ctypes.data, aov_spp, w, h, passes, sigma_color, sigma_depth,
                          normal_power_log2, out.ctypes.data)
        assert rc == 0, "hc_denoise refused its arguments"
        return out
    return run


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def relmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.mean((a - b) ** 2 / (b ** 2 + 0.01)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_quality.json"))
    args = ap.parse_args()
    import aov_expected as ae
    import denoise_expected as de
    from oracle.oracle import Oracle, build, usable_cpus
    from rtcuda_amd import scenes
    build()
    orc = Oracle("pinned")
    osc = orc.scene(scenes.cornell_bunny("full_bsdf")).set_watertight(True)
    run = twin()
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
        noisy = de.noisy_mean(beauty, spp)
        frames.append((w, h, spp, beauty, aov, rms(noisy, refs[(w, h)]), relmse(noisy, refs[(w, h)])))
        print(f"{w}x{h}x{spp}: noisy frame rms {frames[-1][5]:.5f} relmse {frames[-1][6]:.5f}", flush=True)
    rows = []
    for p, sc, sd, npw in itertools.product(*(GRID[k] for k in ("passes", "sigma_color", "sigma_depth", "normal_power_log2"))):
        outs = [run(b, spp, a, spp, w, h, p, sc, sd, npw) for w, h, spp, b, a, _, _ in frames]
        r_rms = [rms(o, refs[f[:2]]) / f[5] for o, f in zip(outs, frames)]
        r_rel = [relmse(o, refs[f[:2]]) / f[6] for o, f in zip(outs, frames)]
        rows.append(dict(passes=p, sigma_color=sc, sigma_depth=sd, normal_power_log2=npw, rms_ratios=[round(r, 4) for r in r_rms],
                         relmse_ratios=[round(r, 4) for r in r_rel], score=round(float(np.exp(np.mean(np.log(r_rel)))), 4)))
    rows.sort(key=lambda r: r["score"])
    small = [k for k, f in enumerate(frames) if f[:2] == (64, 48)]
    best = next(r for r in rows if all(r["rms_ratios"][k] < 1 for k in small))
    print("best:", best, flush=True)
    doc = dict(scene="full_bsdf", frames=[list(f[:3]) for f in frames], reference_spp=REFERENCE_SPP, reference_seed=REFERENCE_SEED,
               metric="ratios are denoised / noisy against the reference frame, linear mean radiance; rms over pixels and channels; "
                      "relmse = mean of (x - ref)^2 / (ref^2 + 0.01); score = geometric mean of the four relmse ratios; defaults = "
                      "lowest score among the rows with both 64x48 rms ratios below 1",
               noisy_rms=[round(f[5], 6) for f in frames], noisy_relmse=[round(f[6], 6) for f in frames],
               grid={k: list(v) for k, v in GRID.items()},
               defaults={k: best[k] for k in ("passes", "sigma_color", "sigma_depth", "normal_power_log2")},
               default_rms_ratios=best["rms_ratios"], default_relmse_ratios=best["relmse_ratios"], default_score=best["score"],
               table=rows)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
