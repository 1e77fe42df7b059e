"""rt_upsample_fixed and rt_upsample_rgb in numpy float32, restated from the text of include/rtcuda_amd.h:
every intermediate is a float32 array, so every operation is rounded on its own, in the order the header writes it.  Nothing here
reads rtcuda_amd/csrc/rt_upsample.h.  tests/test_upsample_host.py holds the CPU twin (hc_upsample) to this file,
tests/test_gpu_upsample.py the kernel."""
import numpy as np

import aov_expected as ae
import denoise_expected as de

F32 = np.float32
GUIDED, TENT, SHORTCUT = 0, 1, 2
FACTORS = (2, 3, 4)
MAX_NORMAL_POWER_LOG2 = 8


def default_params():
    """What rt_upsample_default_params writes (profiles/upsample_quality.json is where they come from)."""
    return dict(sigma_depth=F32(0.03125), normal_power_log2=5)


def depth_constant(sigma_depth):
    """kz as the host makes it: two rounded operations."""
    with np.errstate(all="ignore"):
        return F32(F32(1.0) / F32(F32(sigma_depth) * F32(sigma_depth)))


def prepare_low_rgb(rgb, aov, aov_spp):
    """Step 1 of rt_upsample_rgb: c is the given float, NaN and infinities taken as 0; the rest is the denoiser's steps 1 and 2."""
    rgb = np.asarray(rgb, F32).reshape(-1, 3)
    c = np.where(np.isfinite(rgb), rgb, F32(0)).astype(F32)
    f = ae.resolve(np.asarray(aov, np.int64).reshape(-1, ae.CHANNELS), aov_spp)
    a, n, e, z = f[:, ae.ALBEDO:ae.ALBEDO + 3], f[:, ae.NORMAL:ae.NORMAL + 3], f[:, ae.EMISSION:ae.EMISSION + 3], f[:, ae.DEPTH]
    d = np.where(a > de.ALBEDO_FLOOR, a, de.ALBEDO_FLOOR).astype(F32)
    t = (c - e).astype(F32)
    u = (np.where(t > 0, t, F32(0)).astype(F32) / d).astype(F32)
    return u, z.astype(F32).copy(), n.astype(F32).copy()


def position(n_full, factor):
    """Step 3 for the coordinates 0 .. n_full - 1 of one axis: (X0 (int64), f (float32))."""
    x = np.arange(n_full, dtype=np.int64)
    a = 2 * x + 1 - factor
    x0 = np.floor_divide(a, 2 * factor)  # toward minus infinity
    r = a - 2 * factor * x0
    return x0, (r.astype(F32) / F32(2 * factor)).astype(F32)


def tent(j, f):
    t = (F32(j) - f).astype(F32)
    return (F32(1) - (F32(0.5) * np.where(t < 0, -t, t).astype(F32)).astype(F32)).astype(F32)


def _upsample(u_lo, z_lo, n_lo, lw, lh, factor, aov_hi, aov_spp_hi, sigma_depth, normal_power_log2):
    dp = default_params()
    sigma_depth = dp["sigma_depth"] if sigma_depth is None else sigma_depth
    npow = dp["normal_power_log2"] if normal_power_log2 is None else normal_power_log2
    assert factor in FACTORS and u_lo.shape == (lw * lh, 3)
    w, h = factor * lw, factor * lh
    aov_hi = np.asarray(aov_hi, np.int64).reshape(-1, ae.CHANNELS)
    assert aov_hi.shape[0] == w * h
    _, zp, np_, dp_, ep = de.prepare(np.zeros((w * h, 3), np.int64), 1, aov_hi, aov_spp_hi)  # step 2: z, n, d, e of the full pixels
    Z, N = zp.reshape(h, w), np_.reshape(h, w, 3)
    U, ZL, NL = u_lo.reshape(lh, lw, 3), z_lo.reshape(lh, lw), n_lo.reshape(lh, lw, 3)
    kz = depth_constant(sigma_depth)
    x0, fx = position(w, factor)
    y0, fy = position(h, factor)
    sw, sh = np.zeros((h, w), F32), np.zeros((h, w), F32)
    su, sb = np.zeros((h, w, 3), F32), np.zeros((h, w, 3), F32)
    with np.errstate(all="ignore"):
        for jy in range(-1, 3):
            qy = y0 + jy
            ky = tent(jy, fy)
            for jx in range(-1, 3):
                qx = x0 + jx
                inside = ((qy >= 0) & (qy < lh))[:, None] & ((qx >= 0) & (qx < lw))[None, :]
                cy, cx = np.clip(qy, 0, lh - 1)[:, None], np.clip(qx, 0, lw - 1)[None, :]
                hk = (ky[:, None] * tent(jx, fx)[None, :]).astype(F32)
                uq, zq, nq = U[cy, cx], ZL[cy, cx], NL[cy, cx]
                du = (uq - uq).astype(F32)  # both colour arguments of the tap weight are u_q
                sq = (du * du).astype(F32)
                xc = (((sq[..., 0] + sq[..., 1]).astype(F32) + sq[..., 2]).astype(F32) * F32(0)).astype(F32)
                dz = (zq - Z).astype(F32)
                xz = ((dz * dz).astype(F32) * kz).astype(F32)
                ex = de.expnegf(-((xc + xz).astype(F32)))
                pr = (N * nq).astype(F32)
                dot = ((pr[..., 0] + pr[..., 1]).astype(F32) + pr[..., 2]).astype(F32)
                wn = np.where(dot > 0, np.where(dot < 1, dot, F32(1)), F32(0)).astype(F32)
                for _ in range(npow):
                    wn = (wn * wn).astype(F32)
                wt = ((hk * ex).astype(F32) * wn).astype(F32)
                sw = np.where(inside, (sw + wt).astype(F32), sw)
                su = np.where(inside[..., None], (su + (wt[..., None] * uq).astype(F32)).astype(F32), su)
                sh = np.where(inside, (sh + hk).astype(F32), sh)
                sb = np.where(inside[..., None], (sb + (hk[..., None] * uq).astype(F32)).astype(F32), sb)
        guided = sw > 0
        up = np.where(guided[..., None], (su / sw[..., None]).astype(F32), (sb / sh[..., None]).astype(F32)).astype(F32)
        hit = (aov_hi[:, ae.HITS] > 0).reshape(h, w)
        up = np.where(hit[..., None], up, F32(0)).astype(F32).reshape(-1, 3)
        out = ((up * dp_).astype(F32) + ep).astype(F32)
    form = np.where(hit, np.where(guided, GUIDED, TENT), SHORTCUT).astype(np.uint8).reshape(-1)
    return out, ae.to_fixed(out).reshape(-1, 3), form == TENT, form == SHORTCUT


def upsample(beauty_lo, spp, aov_lo, aov_spp_lo, lw, lh, factor, aov_hi, aov_spp_hi, sigma_depth=None, normal_power_log2=None):
    """rt_upsample_fixed: (rgb (n, 3) float32, fixed (n, 3) int64, the mask of pixels that took step 5's second form, the mask of
    pixels that took step 2's shortcut), n = factor^2 * lw * lh."""
    u, z, n, _, _ = de.prepare(beauty_lo, spp, aov_lo, aov_spp_lo)
    return _upsample(u, z, n, lw, lh, factor, aov_hi, aov_spp_hi, sigma_depth, normal_power_log2)


def upsample_rgb(rgb_lo, aov_lo, aov_spp_lo, lw, lh, factor, aov_hi, aov_spp_hi, sigma_depth=None, normal_power_log2=None):
    """rt_upsample_rgb: as upsample."""
    u, z, n = prepare_low_rgb(rgb_lo, aov_lo, aov_spp_lo)
    return _upsample(u, z, n, lw, lh, factor, aov_hi, aov_spp_hi, sigma_depth, normal_power_log2)


bits = de.bits


# ---- inputs the host and the GPU tests share
def synthetic_pair(lw, lh, factor, seed=5):
    """Seeded random sums with structure at both sizes, independent of each other (the filter does not ask that they show one
    view): (beauty_lo, spp, aov_lo, aov_spp_lo, aov_hi, aov_spp_hi).  de.synthetic_frame's: a few normal directions, depths in
    steps, misses, partial coverage, emission, black albedo, fireflies."""
    beauty, spp, aov_lo, aov_spp = de.synthetic_frame(lw, lh, seed)
    _, _, aov_hi, aov_spp_hi = de.synthetic_frame(factor * lw, factor * lh, seed + 1)
    return beauty, spp, aov_lo, aov_spp, aov_hi, aov_spp_hi


def wild_rgb(n, seed=6):
    """Float radiance from denormals to 2^100, both signs, with every value step 1 must mend.  (Step 1 mends what is not finite;
    a finite c of 2^118 or more over the albedo floor 2^-10 would overflow u, which the header leaves undefined.)"""
    rng = np.random.default_rng(seed + n)
    c = (np.exp2(rng.uniform(-140, 100, (n, 3))) * np.where(rng.random((n, 3)) < 0.2, -1.0, 1.0)).astype(F32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 2.0 ** 100, 1.0, 2.5], F32)
    flat = c.reshape(-1)
    flat[:min(flat.size, special.size)] = special[:flat.size]
    return c
