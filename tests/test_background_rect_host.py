"""The background rectangle (rtcuda_amd/csrc/rt_background.h) against the product's own CPU walk.  No GPU.

k_paths makes no camera ray for a pixel outside the rectangle, so the rectangle's guarantee is checked where it can be checked
exhaustively: every ray that gen_core would make for a pixel outside it -- any jitter in [0, 1)^2 -- must miss every triangle,
under the product's walk of its padded 4-wide records (rt_hostwalk_trace) and under the default kernels' decision procedure
with the reference's literal walk behind it (rt_hostwalk_trace_verified).  And the rectangle must be tight: within 4 pixels
inside each of its edges that lies inside the frame some ray hits.

The rays are formed as the kernels form them (gen_camera_ray / camera_get_ray of rt_device.h), in fp32, operation by operation.

The last three tests take their inputs from tests/background_views.py -- oblique, rolled, near and far views, the scene scaled,
shifted and stretched, the scene moved under a fixed camera -- which tests/test_gpu_background_views.py renders on the device.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import background_views as bv
from conftest import ROOT, default_camera
from test_traversal_audit import HostWalk

F = np.float32
ONE_BELOW = np.nextafter(F(1), F(0))  # the largest jitter rng_uniform can return is below 1


@functools.lru_cache(maxsize=None)
def _lib():
    """The host-check library, built and loaded once per session."""
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "../librt_hostcheck.so"], stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(os.path.join(ROOT, "rtcuda_amd", "librt_hostcheck.so"))
    lib.rt_background_rect.restype = ctypes.c_int
    lib.rt_background_rect.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def rect(cam, w, h, lo, hi):
    cam, lo, hi = (np.ascontiguousarray(v, F) for v in (cam, lo, hi))
    out = np.full(4, -7, np.int32)
    assert _lib().rt_background_rect(cam.ctypes.data, w, h, lo.ctypes.data, hi.ctypes.data, out.ctypes.data) == 0
    x0, y0, x1, y1 = (int(v) for v in out)
    assert 0 <= x0 <= x1 <= w and 0 <= y0 <= y1 <= h, (x0, y0, x1, y1)
    return x0, y0, x1, y1


def camera_rays(cam, w, h, px, py, jx, jy):
    """camera_get_ray(cam, (px + jx) / width, (py + jy) / height) in fp32, as gen_camera_ray calls it."""
    cam = np.asarray(cam, F)
    lf, ul, hz, vt = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    x = ((px.astype(F) + jx.astype(F)) / F(w)).astype(F)[:, None]
    y = ((py.astype(F) + jy.astype(F)) / F(h)).astype(F)[:, None]
    d = (((ul[None, :] + hz[None, :] * x).astype(F) + (vt[None, :] * y).astype(F)).astype(F) - lf[None, :]).astype(F)
    inv_len = (F(1) / np.sqrt(((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F), dtype=F)).astype(F)
    d = (d * inv_len[:, None]).astype(F)
    o = np.broadcast_to(lf, d.shape).copy()
    return o, d


def jittered(px, py, rng, n_random):
    """Every pixel at its four corners and at n_random jitters of its own."""
    corners = [(F(0), F(0)), (ONE_BELOW, F(0)), (F(0), ONE_BELOW), (ONE_BELOW, ONE_BELOW)]
    n = len(px)
    jx = np.concatenate([np.full(n, c[0], F) for c in corners] + [rng.random(n, dtype=F) for _ in range(n_random)])
    jy = np.concatenate([np.full(n, c[1], F) for c in corners] + [rng.random(n, dtype=F) for _ in range(n_random)])
    reps = len(corners) + n_random
    return np.tile(px, reps), np.tile(py, reps), jx, jy


def hits(walk, cam, w, h, px, py, jx, jy, verified=False):
    o, d = camera_rays(cam, w, h, px, py, jx, jy)
    tri = walk.closest_verified(o, d)[0] if verified else walk.closest(o, d)[0]
    return tri >= 0


def check_rectangle(walk, cam, w, h, lo, hi, seed, n_random_pixels=100_000):
    """The guarantee and the tightness of the rectangle of one frame; returns it."""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = r = rect(cam, w, h, lo, hi)
    yy, xx = np.mgrid[0:h, 0:w]
    inside = (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1)
    # a 3-pixel band just outside the rectangle (where it exists), whole
    band = ~inside & (xx >= x0 - 3) & (xx < x1 + 3) & (yy >= y0 - 3) & (yy < y1 + 3)
    sets = [(xx[band].astype(np.int32), yy[band].astype(np.int32))]
    # random pixels anywhere outside
    ox, oy = xx[~inside], yy[~inside]
    if len(ox):
        k = rng.integers(0, len(ox), min(n_random_pixels, 4 * len(ox)))
        sets.append((ox[k].astype(np.int32), oy[k].astype(np.int32)))
    for px, py in sets:
        if len(px) == 0:
            continue
        a = jittered(px, py, rng, 8)
        for verified in (False, True):
            got = hits(walk, cam, w, h, *a, verified=verified)
            assert not got.any(), (r, "verified" if verified else "product", int(got.sum()), a[0][got][:4], a[1][got][:4])
    # tight: within 4 pixels inside each edge that lies inside the frame, at least one ray hits
    if x1 > x0:
        strips = {"left": (x0 > 0, inside & (xx < x0 + 4)), "right": (x1 < w, inside & (xx >= x1 - 4)),
                  "top": (y0 > 0, inside & (yy < y0 + 4)), "bottom": (y1 < h, inside & (yy >= y1 - 4))}
        for name, (in_frame, strip) in strips.items():
            if in_frame:
                a = jittered(xx[strip].astype(np.int32), yy[strip].astype(np.int32), rng, 4)
                assert hits(walk, cam, w, h, *a).any(), (r, name)
    return r


def bounds(arrays):
    v = np.asarray(arrays.tris, F).reshape(-1, 3)
    return v.min(axis=0), v.max(axis=0)


@pytest.fixture(scope="module")
def walk_c2(bunny_full_bsdf):
    return HostWalk(bunny_full_bsdf)


def test_c2_camera_at_full_size(oracle, bunny_full_bsdf, walk_c2):
    w, h = 1920, 1080
    lo, hi = bounds(bunny_full_bsdf)
    x0, y0, x1, y1 = check_rectangle(walk_c2, default_camera(oracle, w / h), w, h, lo, hi, seed=1)
    # every hit of the twin walk on an 8-pixel grid of pixel corners lies in columns 440 .. 1480 and rows 16 .. 1064
    assert x0 <= 440 and x1 > 1480 and y0 <= 16 and y1 > 1064, (x0, y0, x1, y1)
    share = 1.0 - (x1 - x0) * (y1 - y0) / (w * h)
    print(f"rectangle [{x0}, {x1}) x [{y0}, {y1}), background share {share:.4f}")
    assert share >= 0.45, share


def _flipped(cam):
    c = np.array(cam, F)
    c[3:6] = c[3:6] + c[9:12]
    c[9:12] = -c[9:12]
    return c


def _sheared(cam):
    c = np.array(cam, F)
    c[6:9] = c[6:9] + F(0.2) * c[9:12]
    return c


@pytest.mark.parametrize("name,w,h,change", [
    ("aspect_1", 512, 512, None),
    ("aspect_4_3", 640, 480, None),
    ("flipped_vertical", 480, 270, _flipped),
    ("sheared_horizontal", 480, 270, _sheared),
    ("8x8", 8, 8, None),
    ("1x1", 1, 1, None),
])
def test_other_frames(oracle, bunny_full_bsdf, walk_c2, name, w, h, change):
    cam = default_camera(oracle, w / h)
    if change:
        cam = change(cam)
    lo, hi = bounds(bunny_full_bsdf)
    r = check_rectangle(walk_c2, cam, w, h, lo, hi, seed=2, n_random_pixels=30_000)
    print(name, r)
    if w >= 480:
        assert (r[2] - r[0]) * (r[3] - r[1]) < w * h, r  # there is background in these frames


def test_four_bunnies_bounds(oracle):
    from rtcuda_amd import scenes
    arrays = scenes.cornell_bunny("four_bunnies")
    w, h = 480, 270
    lo, hi = bounds(arrays)
    r = check_rectangle(HostWalk(arrays), default_camera(oracle, w / h), w, h, lo, hi, seed=3, n_random_pixels=30_000)
    assert (r[2] - r[0]) * (r[3] - r[1]) < w * h, r


BOX = (np.array([0, 0, -1], F), np.array([1, 1, 0], F))


@pytest.mark.parametrize("name,lookfrom,lookat", [
    ("inside_the_box", (0.5, 0.5, -0.5), (0.5, 0.5, -1.0)),
    ("plane_cuts_the_bounds", (1.2, 0.5, -0.5), (0.5, 0.5, -3.0)),
])
def test_whole_frame_cameras(oracle, name, lookfrom, lookat):
    w, h = 320, 180
    cam = oracle.camera(lookfrom, lookat, (0, 1, 0), 37.8, w / h)
    assert rect(cam, w, h, *BOX) == (0, 0, w, h)


def test_whole_frame_for_degenerate_and_non_finite_cameras(oracle):
    w, h = 320, 180
    good = default_camera(oracle, w / h)
    assert rect(good, w, h, *BOX) != (0, 0, w, h)
    bad = []
    c = good.copy(); c[6:9] = 0; bad.append(c)                     # no horizontal
    c = good.copy(); c[9:12] = 2 * c[6:9]; bad.append(c)           # vertical parallel to horizontal
    c = good.copy(); c[3:6] = c[0:3] + 0.3 * c[6:9] + 0.1 * c[9:12]; bad.append(c)  # lookfrom in the image plane
    for k in (0, 4, 8, 11):
        for v in (np.nan, np.inf, -np.inf):
            c = good.copy(); c[k] = v; bad.append(c)
    for c in bad:
        assert rect(c, w, h, *BOX) == (0, 0, w, h), c
    assert rect(good, w, h, np.array([0, np.nan, -1], F), BOX[1]) == (0, 0, w, h)
    assert rect(good, w, h, BOX[0], np.array([1, np.inf, 0], F)) == (0, 0, w, h)
    # a pixel step that does not dominate the fp32 rounding of the ray: a camera 10^6 units from the origin
    far = oracle.camera((1e6 + 0.5, 0.5, 1.5), (1e6 + 0.5, 0.5, 0.0), (0, 1, 0), 37.8, w / h)
    assert rect(far, w, h, BOX[0] + F(1e6) * np.array([1, 0, 0], F), BOX[1] + F(1e6) * np.array([1, 0, 0], F)) == (0, 0, w, h)


@pytest.mark.parametrize("name,lookat", [("behind_the_camera", (0.5, 0.5, 3.0)), ("off_screen", (3.0, 0.5, 0.0))])
def test_empty_rectangle(oracle, name, lookat):
    w, h = 320, 180
    cam = oracle.camera((0.5, 0.5, 1.5), lookat, (0, 1, 0), 37.8, w / h)
    x0, y0, x1, y1 = rect(cam, w, h, *BOX)
    assert x0 == x1 and y0 == y1, (x0, y0, x1, y1)
    # and a scene without a box (the bounds of no triangle)
    r = rect(default_camera(oracle, w / h), w, h, np.full(3, np.finfo(F).max, F), np.full(3, -np.finfo(F).max, F))
    assert r[0] == r[2] and r[1] == r[3], r


def test_exported_function_refuses_bad_frames(oracle):
    lib = _lib()
    assert hasattr(lib, "rt_background_rect")
    cam = np.ascontiguousarray(default_camera(oracle, 1.0), F)
    lo, hi = (np.ascontiguousarray(v, F) for v in BOX)
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        out = np.full(4, -7, np.int32)
        assert lib.rt_background_rect(cam.ctypes.data, w, h, lo.ctypes.data, hi.ctypes.data, out.ctypes.data) == 1
        assert (out == -7).all()
    out = np.full(4, -7, np.int32)
    assert lib.rt_background_rect(None, 8, 8, lo.ctypes.data, hi.ctypes.data, out.ctypes.data) == 1


# ---- other views, placed scenes, moved scenes (tests/background_views.py; the device side: tests/test_gpu_background_views.py)
def check_spare_pixel(walk, cam, w, h, r, seed):
    """Step (3) of the chain in rt_background.h: the rectangle is floor(u0 width) - 1 .. ceil(u1 width) + 1, one whole pixel wider on
    every side than the pixels the inflated bounds project to, against errors of about 1e-6 of a pixel.  So the outermost column
    or row inside each edge that lies inside the frame is spare: no ray through it hits, under either walk.  (A rectangle one
    pixel narrower still keeps the guarantee at these inputs; the spare pixel is what tells it from the one the chain asks for.)"""
    x0, y0, x1, y1 = r
    if x1 <= x0:
        return
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[y0:y1, x0:x1]
    strips = {"left": (x0 > 0, xx == x0), "right": (x1 < w, xx == x1 - 1), "top": (y0 > 0, yy == y0), "bottom": (y1 < h, yy == y1 - 1)}
    for name, (in_frame, strip) in strips.items():
        if in_frame:
            a = jittered(xx[strip].astype(np.int32), yy[strip].astype(np.int32), rng, 8)
            for verified in (False, True):
                got = hits(walk, cam, w, h, *a, verified=verified)
                assert not got.any(), (r, name, "verified" if verified else "product", int(got.sum()))


# What a view is in the table for, at 320 x 180 and at 97 x 131, stated on the computed rectangle r = (x0, y0, x1, y1).
_VIEW_PROPERTY = {
    ("oblique", 320): bv.strictly_inside, ("wide_fov", 320): bv.strictly_inside, ("from_above", 320): bv.strictly_inside,
    ("rolled_oblique", 320): bv.strictly_inside,
    ("rolled", 320): lambda r, w, h: r[1] == 0 and r[3] == h and 0 < r[0] and r[2] < w,
    ("scene_left", 320): lambda r, w, h: r[0] == 0 and r[2] < w,
    ("far_narrow", 320): lambda r, w, h: r[3] == h and r[1] > 0,
    ("thin_column", 320): lambda r, w, h: r[0] == 0 and 0 < r[2] <= 12,
    ("thin_column", 97): lambda r, w, h: bv.empty(r),
    ("rolled", 97): bv.whole, ("scene_left", 97): bv.whole,
}


@pytest.mark.parametrize("w,h", [(320, 180), (97, 131)])
@pytest.mark.parametrize("view", list(bv.VIEWS))
def test_other_views(oracle, bunny_full_bsdf, walk_c2, view, w, h):
    """Oblique, rolled, near and far cameras: rectangles with rows cut off, at the frame's first column and last row, a few
    columns wide, empty, and the whole frame."""
    cam = bv.view_camera(oracle.camera, view, w / h)
    r = check_rectangle(walk_c2, cam, w, h, *bounds(bunny_full_bsdf), seed=4, n_random_pixels=20_000)
    print(view, (w, h), r)
    assert r == bv.rectangle(cam, w, h, bunny_full_bsdf)
    check_spare_pixel(walk_c2, cam, w, h, r, seed=14)
    holds = _VIEW_PROPERTY.get((view, w))
    assert holds is None or holds(r, w, h), (view, w, h, r)


_placed_walks = {}


def _placed_walk(arrays, place):
    if place not in _placed_walks:
        moved = bv.placed(arrays, place)
        _placed_walks[place] = (moved, HostWalk(moved))
    return _placed_walks[place]


_PLACE_PROPERTY = {
    "shift_300": bv.whole, "stretch_x_1e3": bv.whole,
    "squash_y_1e-3": lambda r, w, h: 0 < r[3] - r[1] <= 6,
    "stretch_z_50_shift": lambda r, w, h: 0 < r[2] - r[0] <= 10 and 0 < r[3] - r[1] <= 10,
}


@pytest.mark.parametrize("view", list(bv.PLACED_VIEWS))
@pytest.mark.parametrize("place", list(bv.PLACES))
def test_placed_scenes(oracle, bunny_full_bsdf, place, view):
    """The scene scaled, shifted and stretched, the camera moved with it: the margin terms of step (1) of the chain -- 1e-4 of
    the extent, 2^-22 R, 2^-20 |bound|, 2^-17 D -- away from the unit scene, where each was sized."""
    w, h = 320, 180
    moved, walk = _placed_walk(bunny_full_bsdf, place)
    cam = bv.placed_view(oracle.camera, place, view, w / h)
    r = check_rectangle(walk, cam, w, h, *bounds(moved), seed=5, n_random_pixels=20_000)
    print(place, view, r)
    check_spare_pixel(walk, cam, w, h, r, seed=15)
    holds = _PLACE_PROPERTY.get(place, lambda r, w, h: 0 < bv.area(r) < w * h)
    assert holds(r, w, h), (place, view, r)


_MOVE_PROPERTY = {
    "right_0.6": lambda r, w, h: 35 < r[0] and r[2] == w and r[1] == 0 and r[3] == h,
    "half": bv.strictly_inside,
    "up_left": lambda r, w, h: r[0] == 0 and r[1] == 0 and r[2] < 125 and r[3] < h,
    "double": bv.whole,
}


@pytest.mark.parametrize("move", list(bv.MOVES))
def test_moved_scenes(oracle, bunny_full_bsdf, move):
    """The scene moved under the fixed default camera (what update(), rebuild() and set_triangles() do to a scene on the device):
    rectangles that end at the last column, start at the first column and row, and lie inside the old one."""
    w, h = 160, 90
    moved = bv.moved(bunny_full_bsdf, move)
    walk = HostWalk(moved)
    r = check_rectangle(walk, default_camera(oracle, w / h), w, h, *bounds(moved), seed=6, n_random_pixels=20_000)
    print(move, r)
    check_spare_pixel(walk, default_camera(oracle, w / h), w, h, r, seed=16)
    assert _MOVE_PROPERTY[move](r, w, h), (move, r)
