"""Keyed ray tables for the render_rays_keyed tests (numpy only): the camera rays of a pinhole's RT_FLAG_RNG_PER_SAMPLE frame,
made outside the renderer.  Camera ray K of such a frame starts the stream of (seed, K), draws its jitter (x, then y) and
lands on pixel K // spp.  `keyed_pinhole_table` is held to the oracle by tests/test_render_rays_keyed_host.py (its states to
Oracle.sample_stream, its rays to Oracle.xorwow_draw + Oracle.camera_get_ray, key by key) before any GPU test leans on it."""
import numpy as np

import raytable

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15  # splitmix64's increment: key K of seed s is output K + 1 of the generator started at s


def shifted_seed(seed, first):
    """The seed under which key c has the stream that key first + c has under `seed`:
    seed + GOLDEN * (first + c + 1) == (seed + GOLDEN * first) + GOLDEN * (c + 1)  (mod 2^64)."""
    return (seed + GOLDEN * first) & M64


def stream_states(oracle, seed, keys):
    """XORWOW states {d, v0 .. v4} (n, 6) uint32 of the per-sample streams of `keys` (ascending Python ints or an integer
    array): the oracle's 64-bit words, then curand_init's seed scramble of each word in numpy."""
    keys = [int(k) for k in keys]
    n = len(keys)
    first = keys[0]
    if keys == list(range(first, first + n)):
        z = oracle.sample_stream_words(seed, first, n)
    else:
        z = np.array([int(oracle.sample_stream_words(seed, k, 1)[0]) for k in keys], np.uint64)
    s0 = (z & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ np.uint32(0xAAD26B49)
    s1 = (z >> np.uint64(32)).astype(np.uint32) ^ np.uint32(0xF7DCEFDD)
    t0 = np.uint32(1099087573) * s0
    t1 = np.uint32(2591861531) * s1
    st = np.zeros((n, 6), np.uint32)
    st[:, 0] = np.uint32(6615241) + t1 + t0
    st[:, 1] = np.uint32(123456789) + t0
    st[:, 2] = np.uint32(362436069) ^ t0
    st[:, 3] = np.uint32(521288629) + t1
    st[:, 4] = np.uint32(88675123) ^ t1
    st[:, 5] = np.uint32(5783321) + t0
    return st


def keyed_pinhole_table(oracle, cam12, w, h, spp, seed, keys):
    """(origins (n, 3), dirs (n, 3), pixel (n,) int32) of the camera rays `keys` of the w x h x spp per-sample frame of seed
    `seed`: pixel K // spp, jitter = the first two draws of the stream of (seed, K), ray = camera.get_ray((px + jx) / w,
    (py + jy) / h) with every operation in float32 and in gen()'s order, as raytable.pinhole_table forms it."""
    with np.errstate(over="ignore"):
        st = stream_states(oracle, seed, keys)
        jx = raytable._uniform(raytable._xorwow_next(st))
        jy = raytable._uniform(raytable._xorwow_next(st))
    n = st.shape[0]
    pix64 = np.array([int(k) // spp for k in keys], np.int64)
    assert pix64.min() >= 0 and pix64.max() < w * h, "a key outside the frame"
    pixel = pix64.astype(np.int32)
    px, py = (pixel % w).astype(np.float32), (pixel // w).astype(np.float32)
    x = ((px + jx) / np.float32(w)).astype(np.float32)[:, None]
    y = ((py + jy) / np.float32(h)).astype(np.float32)[:, None]
    cam12 = np.asarray(cam12, np.float32)
    lf, ul, hz, vt = cam12[0:3], cam12[3:6], cam12[6:9], cam12[9:12]
    d = ((ul + hz * x) + vt * y) - lf
    inv_len = np.float32(1.0) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    d = (d * inv_len[:, None]).astype(np.float32)
    o = np.array(np.broadcast_to(lf, (n, 3)), np.float32)  # (a writable copy, also for n = 1)
    return o, np.ascontiguousarray(d), pixel
