"""What the emission stop, the triangle stop and the single-buffer loop buy, and where the defaults of
rt_temporal_accumulate_moments_fixed come from: the two 8-frame sequences of tools/temporal_quality.py (same sizes, seeds,
1024-spp references, metric and selection rule) on the CPU, written to profiles/temporal_moments_quality.json.  No GPU: frames are
the oracle's; the motion records, the accumulators and the denoisers are the CPU twins (the kernels' arithmetic, bit for bit).

Rows (ratios against the noisy 4-spp frame of the last view, as in that tool):
  a  the parent's table -- two halves, rt_temporal_accumulate_fixed's parameters -- run through the NEW entry point with the new
     features off (emission_tolerance = +inf, no previous motion, no moments); it must reproduce profiles/temporal_quality.json.
  b  two halves + the emission stop -> denoise_dual(hist_a, 1, hist_b, 1).
  c  b with the triangle stop (the previous frame's motion buffer).
  d  ONE buffer of the same 4 spp (the sum of the halves: the shards of a per-sample frame add up to it exactly) + the emission
     stop + moments -> denoise_variance(hist_a, 1, variance).  The like-for-like partner of b.
  dt d with the triangle stop.  The like-for-like partner of c.
  e  denoise_dual alone on the last frame's halves.
b, c, d and dt are swept over a reduced grid of the old parameters times emission_tolerance in {1/16, 1, +inf} (and, for d and dt,
variance_min_history in {1, 4}).  The defaults are the row of d and dt together with the lowest geometric mean of the four relmse
ratios among the rows whose rms ratio is below 1 on both 64x48 sequences (`defaults_from` says which table it is in: whether the
loop should hand over the previous motion buffer).  No ratio is fixed in advance.

    python tools/temporal_moments_quality.py [--out profiles/temporal_moments_quality.json] [--small] [--cache DIR]
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

import temporal_quality as tq  # noqa: E402  (the sequences' constants, the metric)

GRID = dict(max_history=(4, 8, 16, 32), alpha_min=(0.03125, 0.125), depth_tolerance=(0.03125,), normal_cos_min=(0.5,))
EMISSION_TOLERANCES = (0.0625, 1.0, float("inf"))
VARIANCE_MIN_HISTORIES = (1, 4)
MODES = ("b", "c", "d", "dt")
OLD_KEYS = ("max_history", "alpha_min", "depth_tolerance", "normal_cos_min")
ALL_KEYS = OLD_KEYS + ("emission_tolerance", "variance_min_history")


def twins():
    from rtcuda_amd import api
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.hc_denoise_dual.argtypes = [vp, ci, vp, ci, vp, ci, ci, ci, ci, cf, cf, ci, vp, vp]
    L.hc_denoise_variance.argtypes = [vp, ci, vp, vp, ci, ci, ci, ci, cf, cf, ci, vp, vp]
    L.hc_temporal_accumulate_moments.argtypes = [vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, ci, ci, ci, cf, cf, cf, cf, ci, vp, vp, vp, vp, vp]
    dp = api.denoise_dual_default_params()
    spp = tq.SPP

    def ptr(a):
        return None if a is None else a.ctypes.data

    def dual(a, spp_a, b, spp_b, aov, w, h):
        out = np.zeros((w * h, 3), np.float32)
        assert L.hc_denoise_dual(a.ctypes.data, spp_a, b.ctypes.data, spp_b, aov.ctypes.data, spp, w, h, dp["passes"], dp["sigma_variance"],
                                 dp["sigma_depth"], dp["normal_power_log2"], out.ctypes.data, None) == 0
        return out

    def variance(s, var, aov, w, h):
        out = np.zeros((w * h, 3), np.float32)
        assert L.hc_denoise_variance(s.ctypes.data, 1, var.ctypes.data, aov.ctypes.data, spp, w, h, dp["passes"], dp["sigma_variance"],
                                     dp["sigma_depth"], dp["normal_power_log2"], out.ctypes.data, None) == 0
        return out

    def accumulate(a, b, aov, mo, hist, w, h, prm, moments):
        """hist: None or [hist_a, hist_b or None, len, prev_aov, prev_motion or None, prev_moments or None]."""
        n = w * h
        oa, ol = np.zeros((n, 3), np.int64), np.zeros(n, np.int32)
        ob = None if b is None else np.zeros((n, 3), np.int64)
        om, ov = (np.zeros((n, 4), np.float32), np.zeros(n, np.float32)) if moments else (None, None)
        hp = [None] * 6 if hist is None else [ptr(x) for x in hist]
        assert L.hc_temporal_accumulate_moments(a.ctypes.data, spp if b is None else spp // 2, ptr(b), spp // 2, aov.ctypes.data, spp, mo.ctypes.data,
                                                hp[0], hp[1], hp[2], hp[3], spp, hp[4], hp[5], w, h, prm["max_history"], prm["alpha_min"],
                                                prm["depth_tolerance"], prm["normal_cos_min"], prm["emission_tolerance"], prm["variance_min_history"],
                                                oa.ctypes.data, ptr(ob), ol.ctypes.data, ptr(om), ptr(ov)) == 0
        return oa, ob, ol, om, ov
    return dual, variance, accumulate


def make_sequences(small, cache):
    """[(name, w, h, frames [(a, b, aov, motion)], reference mean)] exactly as tools/temporal_quality.py makes them."""
    import aov_expected as ae
    import temporal_expected as te
    from oracle.oracle import Oracle, build, usable_cpus
    from rtcuda_amd import scenes
    path = os.path.join(cache, "temporal_moments_sequences%s.npz" % ("_small" if small else "")) if cache else None
    sizes = tq.SIZES[:1] if small else tq.SIZES
    todo = list(itertools.product(sizes, ("orbit", "bunny")))
    if path and os.path.exists(path):
        z = np.load(path)
        return [(name, w, h, [tuple(z[f"{i}_{k}_{j}"] for j in range(4)) for k in range(tq.FRAMES)], z[f"{i}_ref"]) for i, ((w, h), name) in enumerate(todo)]
    build()
    orc = Oracle("pinned")
    base = scenes.cornell_bunny("full_bsdf")
    motion = tq.twins()[1]
    threads = usable_cpus()
    out = []
    for (w, h), name in todo:
        frames, prev_cam, prev_tris, osc = [], None, None, None
        for k in range(tq.FRAMES):
            arrays = base if name == "orbit" else te.moved_arrays(base, tuple(k * s for s in tq.BUNNY_STEP))
            if osc is None or name == "bunny":
                osc = orc.scene(arrays).set_watertight(True)
            a = np.deg2rad(tq.ORBIT_DEGREES * k) if name == "orbit" else 0.0
            cam = orc.camera((0.5 + 1.5 * np.sin(a), 0.5, 1.5 * np.cos(a)), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8, w / h)
            halves = []
            for r in (0, 1):
                half = np.zeros((h, w, 3), np.int64)
                osc.render(cam, w, h, tq.SPP, seed=100 + k, threads=threads, fixed_out=half, rng_mode="per_sample", shard=(r, 2))
                halves.append(half.reshape(-1, 3))
            aov = ae.frame_expected(orc, osc, cam, w, h, tq.SPP, seed=100 + k)[0]
            o, d = te.centre_rays(orc, cam, w, h)
            tri, _, u, v = osc.trace_closest(o, d, np.full(w * h, te.FLT_MAX, np.float32), threads=threads)
            mo = motion(tri, u, v, arrays.tris if prev_tris is None else prev_tris, cam if prev_cam is None else prev_cam, w, h)
            frames.append((halves[0], halves[1], np.ascontiguousarray(aov, np.int64), mo))
            prev_cam, prev_tris = cam, arrays.tris
        fixed = np.zeros((h, w, 3), np.int64)
        osc.render(cam, w, h, tq.REFERENCE_SPP, seed=tq.REFERENCE_SEED, threads=threads, fixed_out=fixed, rng_mode="per_sample")
        out.append((name, w, h, frames, tq.mean_of(fixed.reshape(-1, 3), tq.REFERENCE_SPP)))
        print(f"{name} {w}x{h}: frames made", flush=True)
    if path:
        os.makedirs(cache, exist_ok=True)
        np.savez_compressed(path, **{f"{i}_{k}_{j}": s[3][k][j] for i, s in enumerate(out) for k in range(tq.FRAMES) for j in range(4)},
                            **{f"{i}_ref": s[4] for i, s in enumerate(out)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_moments_quality.json"))
    ap.add_argument("--small", action="store_true", help="64x48 only (a quick look; the committed file has both sizes)")
    ap.add_argument("--cache", default=None, help="a directory to keep the oracle's frames in between runs")
    args = ap.parse_args()
    import aov_expected as ae
    from rtcuda_amd import api
    sequences = make_sequences(args.small, args.cache)
    dual, variance, accumulate = twins()
    spp = tq.SPP
    noisy, alone = [], []
    for name, w, h, frames, ref in sequences:
        a, b, aov, _ = frames[-1]
        x = tq.mean_of(a + b, spp)
        noisy.append((tq.rms(x, ref), tq.relmse(x, ref)))
        y = dual(a, spp // 2, b, spp // 2, aov, w, h)
        alone.append(dict(rms=round(tq.rms(y, ref) / noisy[-1][0], 4), relmse=round(tq.relmse(y, ref) / noisy[-1][1], 4)))

    def near_emitter(aov, w, h):
        lit = (aov[:, ae.EMISSION:ae.EMISSION + 3] > 0).any(axis=1).reshape(h, w)
        near = np.zeros_like(lit)
        for dy, dx in itertools.product(range(-2, 3), repeat=2):
            near[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] |= lit[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
        return near.reshape(-1)

    def run(mode, prm, detail=False):
        """mode a / b: two halves, no previous motion; c: with it; d: one buffer and moments, no previous motion; dt: with it."""
        out, single = [], mode in ("d", "dt")
        for (name, w, h, frames, ref), (n_rms, n_rel) in zip(sequences, noisy):
            hist = None
            for a, b, aov, mo in frames:
                if single:
                    oa, ob, ol, om, ov = accumulate(a + b, None, aov, mo, hist, w, h, prm, True)
                else:
                    oa, ob, ol, om, ov = accumulate(a, b, aov, mo, hist, w, h, prm, False)
                hist = [oa, ob, ol, aov, mo if mode in ("c", "dt") else None, om]
            if single:
                acc, both = tq.mean_of(oa, 1), variance(oa, ov, aov, w, h)
            else:
                acc, both = tq.mean_of(oa + ob, 2), dual(oa, 1, ob, 1, aov, w, h)
            out.append(dict(kept=round(float(np.mean(ol > 1)), 4), mean_len=round(float(np.mean(ol)), 3),
                            acc_rms=round(tq.rms(acc, ref) / n_rms, 4), acc_relmse=round(tq.relmse(acc, ref) / n_rel, 4),
                            both_rms=round(tq.rms(both, ref) / n_rms, 4), both_relmse=round(tq.relmse(both, ref) / n_rel, 4)))
            if detail:  # where the final image's relmse sits
                e = ((np.asarray(both, np.float64) - ref) ** 2 / (ref ** 2 + 0.01)).sum(axis=1)
                near = near_emitter(aov, w, h)
                out[-1].update(both_relmse_share_within_2_pixels_of_an_emitter=round(float(e[near].sum() / e.sum()), 4),
                               pixels_within_2_pixels_of_an_emitter=round(float(near.mean()), 4))
        return out

    def score(res):
        return round(float(np.exp(np.mean(np.log([r["both_relmse"] for r in res])))), 4)

    small = [k for k, s in enumerate(sequences) if s[1:3] == (64, 48)]

    def pick(rows):
        rows.sort(key=lambda r: r["score"])
        return next((r for r in rows if all(r["sequences"][k]["both_rms"] < 1 for k in small)), None)

    # a: the parent's table through the new entry point
    parent = json.load(open(os.path.join(ROOT, "profiles", "temporal_quality.json")))
    rows_a = []
    for row in parent["table"]:
        prm = dict({k: row[k] for k in OLD_KEYS}, emission_tolerance=float("inf"), variance_min_history=1)
        res = run("a", prm)
        rows_a.append(dict({k: row[k] for k in OLD_KEYS}, sequences=res, score=score(res)))
    if args.small:
        same = all(r["sequences"] == p["sequences"][:2] for r, p in zip(rows_a, parent["table"]))
    else:
        same = all(r["sequences"] == p["sequences"] and r["score"] == p["score"] for r, p in zip(rows_a, parent["table"]))
    print("a reproduces the parent's table:", same, flush=True)
    parent_default = next(r for r in rows_a if all(r[k] == parent["defaults"][k] for k in OLD_KEYS))

    tables = {}
    for mode in MODES:
        rows = []
        for mh, am, dt, nc in itertools.product(*(GRID[k] for k in OLD_KEYS)):
            if am > 1.0 / mh * 4:
                continue
            for et, vmh in itertools.product(EMISSION_TOLERANCES, VARIANCE_MIN_HISTORIES if mode in ("d", "dt") else (1,)):
                prm = dict(max_history=mh, alpha_min=am, depth_tolerance=dt, normal_cos_min=nc, emission_tolerance=et, variance_min_history=vmh)
                res = run(mode, prm)
                rows.append(dict(prm, sequences=res, score=score(res)))
        tables[mode] = rows
        print(mode, "best:", pick(rows), flush=True)
    best = {m: pick(tables[m]) for m in MODES}
    single_rows = [dict(r, table=m) for m in ("d", "dt") for r in tables[m]]  # (d first: it wins a tie, the loop with one input fewer)
    chosen = pick(single_rows) or single_rows[0]
    detail = {m: (None if best[m] is None else run(m, {k: best[m][k] for k in ALL_KEYS}, detail=True)) for m in MODES}
    detail["a"] = run("a", dict({k: parent["defaults"][k] for k in OLD_KEYS}, emission_tolerance=float("inf"), variance_min_history=1), detail=True)

    def js(x):  # (+inf is not JSON)
        if isinstance(x, dict):
            return {k: js(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return [js(v) for v in x]
        return "inf" if isinstance(x, float) and np.isinf(x) else x

    doc = dict(scene="full_bsdf", build_id=api.build_id(), frames_per_sequence=tq.FRAMES, spp_per_frame=spp, reference_spp=tq.REFERENCE_SPP,
               reference_seed=tq.REFERENCE_SEED, orbit_degrees_per_frame=tq.ORBIT_DEGREES, bunny_step_per_frame=list(tq.BUNNY_STEP),
               sequences=[dict(name=s[0], width=s[1], height=s[2], noisy_rms=round(n[0], 6), noisy_relmse=round(n[1], 6)) for s, n in zip(sequences, noisy)],
               metric="as profiles/temporal_quality.json: the last frame against the 1024-spp reference of its view, linear mean radiance; ratios against "
                      "the noisy 4-spp frame; both = the loop's final image (a, b, c: denoise_dual(hist_a, 1, hist_b, 1); d, dt: denoise_variance(hist_a, 1, "
                      "variance); c and dt hand the previous motion buffer over (the triangle stop), b and d do not) at denoise_dual's defaults; score = geometric mean of the both_relmse ratios; a row is picked as the lowest score among "
                      "the rows whose both_rms is below 1 on both 64x48 sequences; emission_tolerance 'inf' = the stop is open",
               denoise_dual_params=api.denoise_dual_default_params(), grid=js(dict(GRID, emission_tolerance=EMISSION_TOLERANCES, variance_min_history=VARIANCE_MIN_HISTORIES)),
               a_reproduces_profiles_temporal_quality_json=bool(same), a_parent_defaults=dict(parent["defaults"], sequences=detail["a"], score=parent_default["score"]),
               e_denoise_dual_alone=dict(sequences=alone, score=round(float(np.exp(np.mean(np.log([x["relmse"] for x in alone])))), 4)),
               b_best=js(None if best["b"] is None else dict(best["b"], sequences=detail["b"])),
               c_best=js(None if best["c"] is None else dict(best["c"], sequences=detail["c"])),
               d_best=js(None if best["d"] is None else dict(best["d"], sequences=detail["d"])),
               dt_best=js(None if best["dt"] is None else dict(best["dt"], sequences=detail["dt"])),
               a_row_of_d_or_dt_passes_the_rms_rule=bool(best["d"] is not None or best["dt"] is not None),
               defaults=js({k: chosen[k] for k in ALL_KEYS}), default_score=chosen["score"], defaults_from=chosen["table"],
               table_a=rows_a, table_b=js(tables["b"]), table_c=js(tables["c"]), table_d=js(tables["d"]), table_dt=js(tables["dt"]))
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
