"""What followed AOVs buy the denoisers: rt_denoise_fixed and rt_denoise_dual_fixed at their current defaults, guided by first-hit
AOVs and by followed AOVs at max_specular 1, 2 and 5, written to profiles/aov_follow_quality.json.  No GPU.  Frames, 1024-spp
references, metrics and the rule of tools/denoise_dual_quality.py (full_bsdf, 64x48 and 192x144, 4 and 16 spp; rms and relmse as
ratios denoised / noisy), reported for three pixel sets taken from the ids of the AOV frame: the whole image, the pixels whose
first hit is glass, and those whose first hit is the mirror.  The followed AOVs are tests/aov_follow_expected.py's (what
k_aov_follow is held to, bit for bit); the filters are the CPU twins hc_denoise / hc_denoise_dual (the kernels' arithmetic, bit
for bit).  Nothing is swept: the defaults are what they are.

    python tools/aov_follow_quality.py [--out profiles/aov_follow_quality.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from denoise_dual_quality import FRAMES, REFERENCE_SEED, REFERENCE_SPP, twins  # noqa: E402

CAPS = (1, 2, 5)


def errors(img, ref, mask):
    a, b = np.asarray(img, np.float64)[mask], ref[mask]
    return float(np.sqrt(np.mean((a - b) ** 2))), float(np.mean((a - b) ** 2 / (b ** 2 + 0.01)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aov_follow_quality.json"))
    args = ap.parse_args()
    import aov_expected as ae
    import aov_follow_expected as fe
    import denoise_expected as de
    from oracle.oracle import Oracle, build, usable_cpus
    from rtcuda_amd import api, scenes
    build()
    orc = Oracle("pinned")
    arrays = scenes.cornell_bunny("full_bsdf")
    osc = orc.scene(arrays).set_watertight(True)
    dual, single = twins()
    p2 = api.denoise_dual_default_params()
    refs, rows = {}, []
    for w, h, spp in FRAMES:
        cam = orc.camera((0.5, 0.5, 1.5), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8, w / h)
        if (w, h) not in refs:
            fixed = np.zeros((h, w, 3), np.int64)
            osc.render(cam, w, h, REFERENCE_SPP, seed=REFERENCE_SEED, threads=usable_cpus(), fixed_out=fixed, rng_mode="per_sample")
            refs[(w, h)] = fixed.reshape(-1, 3).astype(np.float64) * (2.0 ** -30 / REFERENCE_SPP)
        ref = refs[(w, h)]
        halves = []
        for r in (0, 1):
            half = np.zeros((h, w, 3), np.int64)
            osc.render(cam, w, h, spp, threads=usable_cpus(), fixed_out=half, rng_mode="per_sample", shard=(r, 2))
            halves.append(half.reshape(-1, 3))
        beauty = halves[0] + halves[1]
        noisy = de.noisy_mean(beauty, spp)
        aovs = {0: ae.frame_expected(orc, osc, cam, w, h, spp)}
        for cap in CAPS:
            aovs[cap] = fe.frame_expected(orc, osc, cam, w, h, spp, cap, census=False)
        mat = aovs[0][1][:, 1]  # (the material of every pixel's first sample)
        kind = np.where(mat >= 0, arrays.materials["type"][np.maximum(mat, 0)], -1)
        sets = {"all": np.ones(w * h, bool), "glass": kind == scenes.GLASS, "mirror": kind == scenes.MIRROR}
        row = dict(frame=[w, h, spp], pixels={k: int(m.sum()) for k, m in sets.items()},
                   noisy={k: dict(zip(("rms", "relmse"), (round(x, 6) for x in errors(noisy, ref, m)))) for k, m in sets.items()}, guides={})
        for cap, frame in aovs.items():
            aov = frame[0]
            outs = {"denoise": single(beauty, spp, aov, spp, w, h)[0],
                    "denoise_dual": dual(halves[0], spp // 2, halves[1], spp // 2, aov, spp, w, h, p2["passes"], p2["sigma_variance"],
                                         p2["sigma_depth"], p2["normal_power_log2"])}
            entry = {}
            for name, img in outs.items():
                entry[name] = {}
                for k, m in sets.items():
                    e_rms, e_rel = errors(img, ref, m)
                    n_rms, n_rel = errors(noisy, ref, m)
                    entry[name][k] = dict(rms_ratio=round(e_rms / n_rms, 4), relmse_ratio=round(e_rel / n_rel, 4))
            row["guides"]["first_hit" if cap == 0 else "follow_%d" % cap] = entry
            print((w, h, spp), "first_hit" if cap == 0 else "follow_%d" % cap, json.dumps(entry), flush=True)
        rows.append(row)
    doc = dict(scene="full_bsdf", build_id=api.build_id(), reference_spp=REFERENCE_SPP, reference_seed=REFERENCE_SEED,
               metric="ratios are denoised / noisy against the reference frame over the pixels of the set, linear mean radiance; rms over "
                      "pixels and channels; relmse = mean of (x - ref)^2 / (ref^2 + 0.01)",
               sets="from the ids of the first-hit AOV frame: the material type of every pixel's first sample",
               denoise_defaults=api.denoise_default_params(), denoise_dual_defaults=p2, frames=rows)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
