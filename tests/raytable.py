"""Ray tables for the render_rays tests (numpy only): the camera rays of the reference's pinhole gen(), made outside the
renderer.  `pinhole_table` is held to the oracle by tests/test_render_rays_host.py (its per-ray restatement through
Oracle.xorwow_draw / Oracle.camera_get_ray, and the oracle's own ray log) before any GPU test leans on it."""
import numpy as np

W = 1 << 20  # path slots
_C = np.float32(2.3283064e-10)


def _xorwow_next(st):
    """One XORWOW step on rows of {d, v0 .. v4} (uint32), in place -> the raw draws."""
    d, v0, v4 = st[:, 0], st[:, 1], st[:, 5]
    t = v0 ^ (v0 >> np.uint32(2))
    nv4 = (v4 ^ (v4 << np.uint32(4))) ^ (t ^ (t << np.uint32(1)))
    st[:, 1:5] = st[:, 2:6].copy()
    st[:, 5] = nv4
    st[:, 0] = d + np.uint32(362437)
    return st[:, 0] + st[:, 5]


def _uniform(raw):
    """curand_uniform of a raw draw, in float32: raw * 2^-32 + 2^-33."""
    return raw.astype(np.float32) * _C + (_C / np.float32(2.0))


def jitter(oracle, n, seed=1):
    """(jx, jy) of the first camera ray of slots 0 .. n-1: the first two draws of subsequence s (x first, then y)."""
    assert 0 < n <= W
    st = oracle.xorwow_init_range(seed, 0, n).copy()
    jx = _uniform(_xorwow_next(st))
    jy = _uniform(_xorwow_next(st))
    return jx, jy


def pinhole_table(oracle, cam12, w, h, spp, seed=1):
    """(origins (n, 3), dirs (n, 3), pixel (n,)) of a one-generation frame (n = w * h * spp <= W): camera ray c is slot c's
    first, pixel c // spp, ray = camera.get_ray((px + jx) / w, (py + jy) / h), every operation in float32 and in gen()'s
    order (render.cuh:250-275, camera.cuh:31-34)."""
    n = w * h * spp
    jx, jy = jitter(oracle, n, seed)
    pixel = (np.arange(n, dtype=np.int64) // spp).astype(np.int32)
    px, py = (pixel % w).astype(np.float32), (pixel // w).astype(np.float32)
    x = ((px + jx) / np.float32(w)).astype(np.float32)[:, None]
    y = ((py + jy) / np.float32(h)).astype(np.float32)[:, None]
    cam12 = np.asarray(cam12, np.float32)
    lf, ul, hz, vt = cam12[0:3], cam12[3:6], cam12[6:9], cam12[9:12]
    d = ((ul + hz * x) + vt * y) - lf
    inv_len = np.float32(1.0) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    d = (d * inv_len[:, None]).astype(np.float32)
    o = np.ascontiguousarray(np.broadcast_to(lf, (n, 3)), np.float32)
    return o, np.ascontiguousarray(d), pixel


def pinhole_table_literal(oracle, cam12, w, h, spp, seed=1):
    """The same table ray by ray through the oracle's own functions (slow: small frames only)."""
    n = w * h * spp
    st = oracle.xorwow_init_range(seed, 0, n)
    o, d = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    for c in range(n):
        _, (jx, jy) = oracle.xorwow_draw(st[c].copy(), 2)
        p = c // spp
        x = (np.float32(p % w) + jx) / np.float32(w)
        y = (np.float32(p // w) + jy) / np.float32(h)
        r = oracle.camera_get_ray(cam12, float(x), float(y))
        o[c], d[c] = r[0:3], r[3:6]
    return o, d


def degenerate_camera(oracle, lookfrom, target):
    """A camera whose horizontal = vertical = 0: every camera ray, whatever its jitter and pixel, is
    (lookfrom, unit(target - lookfrom)) exactly (x * 0 = 0 in fp32).  -> (cam12, origin (3,), dir (3,))"""
    cam = np.zeros(12, np.float32)
    cam[0:3] = np.asarray(lookfrom, np.float32)
    cam[3:6] = np.asarray(target, np.float32)  # upper_left
    r = oracle.camera_get_ray(cam, 0.25, 0.75)
    return cam, r[0:3].copy(), r[3:6].copy()
