"""What a count map buys at an equal budget, and where the documented adaptive loop's min_count / max_count come from: uniform
16 spp against a 4-spp base pass plus 12 samples per pixel placed by rt_sample_allocate, written to profiles/adaptive_quality.json.
No GPU: a counted frame is the masked sum of the oracle's sample frames (what rt_render_counts_fixed leaves, bit for bit:
tests/render_counts_expected.py), the allocator and the normaliser are their Python-integer twins, the denoiser is the CPU twin
hc_denoise_variance (the kernels' arithmetic, bit for bit).  The frames, the 1024-spp references (another seed) and the two
errors -- rms and the firefly-robust relmse -- are tools/denoise_quality.py's: full_bsdf at 64x48 and 192x144, linear mean radiance.

Both arms get the same budget, 16 samples per pixel of the SAME per-sample frame (sample_stride 16):
  uniform   samples 0 .. 15 of every pixel.
  adaptive  samples 0 .. 3 of every pixel (the base pass), then count[p] more from sample 4 on, the counts from the allocator on
            weight = s / (m + 0.05) + floor: s the square root of the base pass's two-half variance of the mean (demodulated
            radiance, halves = even and odd samples, the denoisers' own estimate |u_a - u_b|^2 / 4, optionally through the
            denoisers' 3 x 3 prefilter), m the demodulated mean.  What flooring leaves of the budget is not placed (`placed`).
Each arm noisy (sums over the pixel's own count) and through denoise_variance with the library's default parameters and the
arm's own two-half variance from ALL its samples (even / odd again).  Every ratio is adaptive / uniform: below 1 the count map
wins, above 1 it LOSES.  Swept: min_count, floor, the prefilter.  max_count is 12, all that is left of the stride.  The defaults
of the documented loop are the row with the lowest geometric mean of the four relmse ratios (noisy and denoised, both frames)
among the rows whose denoised rms ratio is below 1 on the 64x48 frame (the rule of the earlier sweeps); if no row qualifies,
the lowest score as it is, and `qualified` says so.

    python tools/adaptive_quality.py [--out profiles/adaptive_quality.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from denoise_quality import REFERENCE_SEED, REFERENCE_SPP, relmse, rms  # noqa: E402

SIZES = ((64, 48), (192, 144))
STRIDE, BASE = 16, 4
GRID = dict(min_count=(0, 2, 4, 8), floor=(0.0, 0.1, 0.5, 2.0), blur=(0, 1))
MAX_COUNT = STRIDE - BASE


def variance_twin():
    from rtcuda_amd import api
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.hc_denoise_variance.argtypes = [vp, ci, vp, vp, ci, ci, ci, ci, cf, cf, ci, vp, vp]
    dp = api.denoise_dual_default_params()

    def run(sums, spp, var, aov, aov_spp, w, h):
        sums, aov, var = np.ascontiguousarray(sums, np.int64), np.ascontiguousarray(aov, np.int64), np.ascontiguousarray(var, np.float32)
        out = np.zeros((w * h, 3), np.float32)
        assert L.hc_denoise_variance(sums.ctypes.data, spp, var.ctypes.data, aov.ctypes.data, aov_spp, w, h, dp["passes"], dp["sigma_variance"],
                                     dp["sigma_depth"], dp["normal_power_log2"], out.ctypes.data, None) == 0
        return out
    return run


def demodulated(sums, n, aov, aov_spp):
    """u of rt_denoise.h's dn_prepare for sums over n[p] samples (float64 here: a weight, not a pinned value); 0 where n == 0."""
    fx = 2.0 ** -30
    a = np.maximum(aov[:, 0:3] * (fx / aov_spp), 2.0 ** -10)
    e = aov[:, 6:9] * (fx / aov_spp)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(n[:, None] > 0, sums * fx / np.maximum(n, 1)[:, None], 0.0)
    return np.maximum(c - e, 0.0) / a


def two_half_variance(frames, first, count, aov, aov_spp):
    """|u_a - u_b|^2 / 4 per pixel, the halves = the pixel's even and odd samples among first .. first + count - 1."""
    n = frames[0].shape[0]
    sa, sb = np.zeros((n, 3), np.int64), np.zeros((n, 3), np.int64)
    na, nb = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for k, f in enumerate(frames):
        m = (first <= k) & (k < first + count)
        if k % 2 == 0:
            sa += f * m[:, None]
            na += m
        else:
            sb += f * m[:, None]
            nb += m
    d = demodulated(sa, na, aov, aov_spp) - demodulated(sb, nb, aov, aov_spp)
    v = (d * d).sum(axis=1) / 4.0
    v[(na == 0) | (nb == 0)] = 0.0
    return v


def blur3(v, w, h):
    """the denoisers' 3 x 3 prefilter {1/4, 1/2, 1/4}^2, renormalised at the frame's edge"""
    img = v.reshape(h, w)
    k = np.array([0.25, 0.5, 0.25])
    pad, one = np.pad(img, 1), np.pad(np.ones_like(img), 1)
    num, den = np.zeros_like(img), np.zeros_like(img)
    for dy, dx in itertools.product(range(3), range(3)):
        num += k[dy] * k[dx] * pad[dy:dy + h, dx:dx + w]
        den += k[dy] * k[dx] * one[dy:dy + h, dx:dx + w]
    return (num / den).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_quality.json"))
    args = ap.parse_args()
    import aov_expected as ae
    import render_counts_expected as rc
    from oracle.oracle import Oracle, build, usable_cpus
    from rtcuda_amd import scenes
    build()
    orc = Oracle("pinned")
    osc = orc.scene(scenes.cornell_bunny("full_bsdf")).set_watertight(True)
    denoise = variance_twin()
    setups = []
    for w, h in SIZES:
        cam = orc.camera((0.5, 0.5, 1.5), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8, w / h)
        fixed = np.zeros((h, w, 3), np.int64)
        osc.render(cam, w, h, REFERENCE_SPP, seed=REFERENCE_SEED, threads=usable_cpus(), fixed_out=fixed, rng_mode="per_sample")
        ref = fixed.reshape(-1, 3).astype(np.float64) * (2.0 ** -30 / REFERENCE_SPP)
        frames = rc.sample_frames(orc, osc, "full_bsdf", w, h, STRIDE)
        aov = ae.frame_expected(orc, osc, cam, w, h, STRIDE)[0]
        n = w * h
        zero, full = np.zeros(n, np.int64), np.full(n, STRIDE, np.int64)
        uni = sum(frames)
        uni_noisy = uni * (2.0 ** -30 / STRIDE)
        uni_var = two_half_variance(frames, zero, full, aov, STRIDE)
        uni_dn = denoise(uni, STRIDE, uni_var, aov, STRIDE, w, h)
        base = sum(frames[:BASE])
        base_var = two_half_variance(frames, zero, np.full(n, BASE, np.int64), aov, STRIDE)
        base_u = demodulated(base, np.full(n, BASE, np.int64), aov, STRIDE).mean(axis=1)
        setups.append(dict(w=w, h=h, ref=ref, frames=frames, aov=aov, base=base, base_var=base_var, base_u=base_u,
                           uniform=dict(noisy_rms=rms(uni_noisy, ref), noisy_relmse=relmse(uni_noisy, ref), denoised_rms=rms(uni_dn, ref),
                                        denoised_relmse=relmse(uni_dn, ref))))
        print(f"{w}x{h}: uniform {STRIDE} spp", setups[-1]["uniform"], flush=True)
    rows = []
    for lo, floor, blur in itertools.product(GRID["min_count"], GRID["floor"], GRID["blur"]):
        row = dict(min_count=lo, max_count=MAX_COUNT, floor=floor, blur=blur, placed=[], noisy_rms_ratios=[], noisy_relmse_ratios=[],
                   denoised_rms_ratios=[], denoised_relmse_ratios=[], max_share=[])
        for s in setups:
            w, h, n = s["w"], s["h"], s["w"] * s["h"]
            v = blur3(s["base_var"], w, h) if blur else s["base_var"]
            weight = (np.sqrt(v) / (s["base_u"] + 0.05) + floor).astype(np.float32)
            count, total = rc.allocate_twin(weight, lo, MAX_COUNT, MAX_COUNT * n)
            count = count.astype(np.int64)
            first = np.full(n, BASE, np.int64)
            sums = s["base"] + rc.expected_by_frames(orc, osc, "full_bsdf", w, h, STRIDE, first, count)
            samples = (BASE + count).astype(np.int32)
            noisy = sums * 2.0 ** -30 / samples[:, None]
            var = two_half_variance(s["frames"], np.zeros(n, np.int64), BASE + count, s["aov"], STRIDE)
            dn = denoise(rc.normalize_twin(sums, samples), 1, var, s["aov"], STRIDE, w, h)
            u = s["uniform"]
            row["placed"].append(round(total / (MAX_COUNT * n), 4))
            row["max_share"].append(round(float((count == MAX_COUNT).mean()), 4))
            row["noisy_rms_ratios"].append(round(rms(noisy, s["ref"]) / u["noisy_rms"], 4))
            row["noisy_relmse_ratios"].append(round(relmse(noisy, s["ref"]) / u["noisy_relmse"], 4))
            row["denoised_rms_ratios"].append(round(rms(dn, s["ref"]) / u["denoised_rms"], 4))
            row["denoised_relmse_ratios"].append(round(relmse(dn, s["ref"]) / u["denoised_relmse"], 4))
        row["score"] = round(float(np.exp(np.mean(np.log(row["noisy_relmse_ratios"] + row["denoised_relmse_ratios"])))), 4)
        rows.append(row)
        print(row, flush=True)
    rows.sort(key=lambda r: r["score"])
    ok = [r for r in rows if r["denoised_rms_ratios"][0] < 1]
    best = (ok or rows)[0]
    doc = dict(scene="full_bsdf", sizes=[list(s) for s in SIZES], sample_stride=STRIDE, base_samples=BASE, reference_spp=REFERENCE_SPP,
               reference_seed=REFERENCE_SEED,
               metric="every ratio is adaptive / uniform at the same budget of 16 samples per pixel, against the reference frame, linear mean "
                      "radiance: below 1 the count map wins, above 1 it LOSES; rms over pixels and channels; relmse = mean of (x - ref)^2 / "
                      "(ref^2 + 0.01); placed = the share of the 12 * pixels extra samples the allocator placed; max_share = the share of "
                      "pixels at max_count; score = geometric mean of the noisy and denoised relmse ratios of both frames; defaults = lowest "
                      "score among the rows whose denoised rms ratio on 64x48 is below 1 (qualified: whether any row was)",
               uniform=[s["uniform"] for s in setups], grid={k: list(v) for k, v in GRID.items()}, qualified=bool(ok),
               defaults=dict(min_count=best["min_count"], max_count=best["max_count"], floor=best["floor"], blur=best["blur"]),
               default_row=best, table=rows)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("best:", best, flush=True)


if __name__ == "__main__":
    main()
