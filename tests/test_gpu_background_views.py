"""GPU tests of the background skip (rt_background.h) away from the default view: the views, moves and scenes of
tests/background_views.py, whose rectangles tests/test_background_rect_host.py holds to the CPU walks.  Run with -m gpu.

The other files' frames all use the default view, whose rectangle only ever cuts columns off: (35, 0, 125, 90) at 160 x 90.  Here
the rectangle cuts rows off (the row half of the kernels' test, (unsigned)(py - y0) >= h), starts at column 0, ends at the last
row, is a few columns wide; the image plane is rolled and oblique; and the scene changes under a fixed camera, so that the
rectangle has to follow the new records (h_quads, origin_radius) through update(), rebuild() and set_triangles().

Every comparison is exact: RT_FLAG_DETERMINISTIC's int64 sums and every event total EQUAL the CPU oracle's frame for the same camera
and those of the same frame with RT_BG_SKIP=0.  No tolerance, no masked pixel.  (The round pipeline, where it is compared, is held
to test_gpu_background_skip._same_as_rounds: totals exact, sums within the two summation orders' bound.)"""
import numpy as np
import pytest

import background_views as bv
import render_counts_expected as rc
from conftest import oracle_scene, usable_cpus
from test_gpu_background_skip import _arrays, _knobs, _on_off, _same, _sums
from test_gpu_gen_loop import _skipping
from test_gpu_render_counts import _assert_sums, _dev, _ev, _random_map
from test_gpu_scene_rebuild import _device_tree
from test_gpu_slot_chunks import W, _check, _oracle_sums

pytestmark = pytest.mark.gpu

MAIN = (160, 90, 256)  # 3.5 generations, 3.7 M samples


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()  # raises if the HIP library is missing: there is no fallback
    return _api


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    return _torch


@pytest.fixture(scope="module")
def gpu(api):
    sc = api.Scene(_arrays())
    yield sc
    sc.close()


def _camera(api, oracle, view, aspect):
    """The view's 12 floats, as the device gets them (rt_camera_make) -- and the oracle gets the same bits."""
    cam = bv.view_camera(api.make_camera, view, aspect)
    assert np.array_equal(cam.view(np.uint32), bv.view_camera(oracle.camera, view, aspect).view(np.uint32)), view
    return cam


_frames = {}


def _oracle_frame(oracle, tag, osc, cam, w, h, spp, shard=(0, 1), rng_mode="reference"):
    """The oracle's fixed-point sums and stats of (a slot-range shard of) a frame of `osc` through `cam`; once per case, read-only."""
    key = (tag, np.asarray(cam, np.float32).tobytes(), w, h, spp, shard, rng_mode)
    if key not in _frames:
        r, R = shard
        n = W // R
        want = np.zeros((h, w, 3), np.int64)
        _, _, st = osc.render(cam, w, h, spp, threads=usable_cpus(), fixed_out=want, slot_lo=r * n, slot_hi=(r + 1) * n, rng_mode=rng_mode)
        want.setflags(write=False)
        _frames[key] = (want, st)
    return _frames[key]


def _bunny_frame(oracle, cam, w, h, spp, watertight=False, **kw):
    return _oracle_frame(oracle, ("full_bsdf", watertight), oracle_scene(oracle, "full_bsdf", watertight), cam, w, h, spp, **kw)


# ---- 1. the views, camera build
# what a view is in the table for at 160 x 90, asserted on r = (x0, y0, x1, y1) from the rectangle helper
_FIRST_COLUMN = lambda r, w, h: r[0] == 0 < r[2] < w  # noqa: E731
_ROWS_CUT = lambda r, w, h: r[1] > 0 and r[3] < h     # noqa: E731  (rows no other file's frame skips)
_AT_160 = {
    "thin_column": lambda r, w, h: _FIRST_COLUMN(r, w, h) and r[2] <= 6,
    "scene_left": _FIRST_COLUMN,
    "rolled": lambda r, w, h: r[1] == 0 and r[3] == h and 0 < r[0] and r[2] < w,
    "oblique": _ROWS_CUT,
    "wide_fov": _ROWS_CUT,
    "far_narrow": lambda r, w, h: r[1] > 0 and r[3] == h,
}


@pytest.mark.parametrize("view", list(bv.VIEWS))
def test_views_equal_the_oracle_and_the_unskipped_frame(api, gpu, oracle, monkeypatch, view):
    w, h, spp = MAIN
    cam = _camera(api, oracle, view, w / h)
    r = bv.rectangle(cam, w, h, _arrays())
    print(view, (w, h), "rectangle", r)
    assert _AT_160.get(view, lambda r, w, h: True)(r, w, h), (view, r)
    want, st_c = _bunny_frame(oracle, cam, w, h, spp)
    assert st_c["sum_mat"] > 0 and (want.any() or view == "from_above")  # (from above only the ceiling's unlit back is seen)
    _, st = _on_off(api, gpu, monkeypatch, w, h, spp, want, st_c, rounds=view in ("thin_column", "rolled"), cam=cam)
    assert st["camera_rays"] == w * h * spp


# ---- 2. long runs over rows of background
@pytest.mark.parametrize("chunk", [None, 4])
@pytest.mark.parametrize("view", ["oblique", "thin_column"])
def test_long_runs_over_rows_of_background(api, gpu, oracle, monkeypatch, view, chunk):
    """320 x 180 x 256: 14 generations, chains of 14 camera rays.  `oblique` (91, 34, 219, 156): a slot's pixel steps through 34 + 24
    whole rows of background per frame; `thin_column` (0, 0, 9, 180): 311 of every 320 pixels, so most runs end at a limit."""
    w, h, spp = 320, 180, 256
    cam = _camera(api, oracle, view, w / h)
    r = bv.rectangle(cam, w, h, _arrays())
    print(view, (w, h), "rectangle", r)
    assert (r[1] > 0 and r[3] < h) if view == "oblique" else (r[0] == 0 < r[2] <= 12), r
    want, st_c = _bunny_frame(oracle, cam, w, h, spp)
    got, st = _skipping(api, gpu, monkeypatch, w, h, spp, chunk, None, cam=cam)
    print(view, "RT_SLOT_CHUNK", chunk, "dealt", st["slot_chunk"])
    _check(got, st, want, st_c, f"{view} RT_SLOT_CHUNK={chunk}")
    assert st["camera_rays"] == w * h * spp


# ---- 3. odd spp
def test_odd_spp_on_the_oblique_view(api, gpu, oracle, monkeypatch):
    """96 x 54 x 509: the pixel cannot be stepped (dpy < 0) and comes from the divisions, rows and columns of it background."""
    w, h, spp = 96, 54, 509
    cam = _camera(api, oracle, "oblique", w / h)
    r = bv.rectangle(cam, w, h, _arrays())
    print("oblique", (w, h), "rectangle", r)
    assert bv.strictly_inside(r, w, h), r
    want, st_c = _bunny_frame(oracle, cam, w, h, spp)
    _, st = _on_off(api, gpu, monkeypatch, w, h, spp, want, st_c, cam=cam)
    assert st["camera_rays"] == w * h * spp


# ---- 4. the other builds
@pytest.mark.parametrize("view", ["oblique", "scene_left"])
@pytest.mark.parametrize("build", ["two_waves_per_simd", "per_sample", "watertight", "reference_walk"])
def test_the_other_builds(api, gpu, oracle, monkeypatch, build, view):
    """Shard 0 of 8: the 2-waves-per-SIMD build, where gen_core's own loop does the skip; per-sample streams: the build without a
    loop; the watertight and the reference-walk builds.  Each against the oracle of the same mode."""
    w, h, spp = MAIN
    cam = _camera(api, oracle, view, w / h)
    kw, okw, watertight = {}, {}, False
    if build == "two_waves_per_simd":
        kw = okw = {"shard": (0, 8)}
    elif build == "per_sample":
        kw, okw, watertight = {"flags": api.FLAG_RNG_PER_SAMPLE}, {"rng_mode": "per_sample"}, True
    elif build == "watertight":
        kw, watertight = {"flags": api.FLAG_WATERTIGHT}, True
    else:
        kw = {"flags": api.FLAG_REFERENCE_WALK}
    want, st_c = _bunny_frame(oracle, cam, w, h, spp, watertight=watertight, **okw)
    assert want.any()
    _, st = _on_off(api, gpu, monkeypatch, w, h, spp, want, st_c, cam=cam, **kw)
    if build == "per_sample":
        assert st["camera_rays"] == st_c["sum_gen"] == w * h * spp
    elif build != "two_waves_per_simd":
        assert st["camera_rays"] == w * h * spp


# ---- 5. counted frames
def _count_maps(which):
    if which == "random":
        w, h, S = 9, 7, 8
        return (w, h, S) + _random_map(w, h, S)
    w, h, S = 19, 27, 3
    return w, h, S, None, np.full(w * h, S, np.int64)


@pytest.mark.parametrize("blocks", [None, "64"])
@pytest.mark.parametrize("which", ["random", "whole"])
@pytest.mark.parametrize("view", ["oblique", "thin_column"])
def test_counted_frames(api, torch, gpu, oracle, monkeypatch, view, which, blocks):
    """rt_render_counts_fixed (k_paths<PathsCounts>, and under RT_PATHS_BLOCKS=64 the 2-waves-per-SIMD build) through the two views:
    a random map of 9 x 7 x 8 against the oracle's keyed tables, a whole 19 x 27 x 3 frame of counts against its per-sample frame.
    `oblique`: (0, 0, 8, 7), a column cut off, and (0, 4, 19, 25), rows cut off.  `thin_column`: the empty rectangle at both sizes,
    so every drawn id is passed over, the sums are zero and only camera_rays counts."""
    w, h, S, first, count = _count_maps(which)
    cam = _camera(api, oracle, view, w / h)
    r = bv.rectangle(cam, w, h, _arrays())
    print(view, (w, h), "rectangle", r)
    osc = oracle_scene(oracle, "full_bsdf", True)
    if which == "random":
        want, ev_c = rc.expected_by_tables(oracle, osc, w, h, S, first, count, cam=cam)
    else:
        want, st_c = _bunny_frame(oracle, cam, w, h, S, watertight=True, rng_mode="per_sample")
        want, ev_c = want.reshape(-1, 3), rc.events_of(st_c)
    if view == "oblique":
        assert want.any()
    if blocks is not None:
        monkeypatch.setenv("RT_PATHS_BLOCKS", blocks)
    frames = {}
    for skip in (True, False):
        _knobs(monkeypatch, skip=skip)
        out, st = gpu.render_counts(cam, w, h, S, _dev(torch, count), first=None if first is None else _dev(torch, first))
        assert st["background_skip"] == (1 if skip and bv.area(r) < w * h else 0), (view, which, skip, r, st["background_skip"])
        _assert_sums(out, want, (view, which, "skip on" if skip else "RT_BG_SKIP=0", blocks))
        assert _ev(st) == ev_c and st["camera_rays"] == int(count.sum())
        frames[skip] = (out.cpu().numpy(), st)
    _knobs(monkeypatch)
    _same(frames[True][0], frames[True][1], frames[False][0], frames[False][1], ("counted, skip on / off", view, which, blocks))


# ---- 6. changed scenes under the fixed default camera
def _change(sc, via, arrays):
    if via == "update":
        sc.update(arrays.tris)
    elif via == "rebuild":
        sc.rebuild(arrays.tris)
    else:
        sc.set_triangles(arrays)


_moved_scenes = {}


def _moved_frame(oracle, move, w, h, spp, cam):
    """(the moved SceneArrays, the oracle's sums of its frame, the oracle's stats); the oracle's scene is made once per move."""
    if move not in _moved_scenes:
        moved = bv.moved(_arrays(), move)
        _moved_scenes[move] = (moved, oracle.scene(moved))
    moved, osc = _moved_scenes[move]
    return (moved,) + _oracle_frame(oracle, ("moved", move), osc, cam, w, h, spp)


def _lit_outside(want, r_new, r_stale):
    """Whether the oracle's frame has light in pixels of r_new that r_stale does not cover: frames a stale rectangle would lose."""
    mask = np.zeros(want.shape[:2], bool)
    mask[r_new[1]:r_new[3], r_new[0]:r_new[2]] = True
    mask[r_stale[1]:r_stale[3], r_stale[0]:r_stale[2]] = False
    return bool(want[mask].any())


def _there_and_back(api, oracle, monkeypatch, sc, via, move):
    """The scene changed to MOVES[move] and back: each frame equals the oracle's of the same triangles and RT_BG_SKIP=0."""
    w, h, spp = MAIN
    orig = _arrays()
    cam = _camera(api, oracle, "default", w / h)
    want_0, st_0 = _oracle_sums(oracle, w, h, spp)
    moved, want_m, st_m = _moved_frame(oracle, move, w, h, spp, cam)
    r_0, r_m = bv.rectangle(cam, w, h, orig), bv.rectangle(cam, w, h, moved)
    print(via, move, "rectangle", r_0, "->", r_m)
    if move == "half":  # the new rectangle lies inside the old one: the old one's area is background now
        assert bv.covers(r_0, r_m) and bv.pixels_outside(r_0, r_m) > 0, (r_0, r_m)
    else:               # new geometry outside the old rectangle: a frame with the old one would lose it
        assert _lit_outside(want_m, r_m, r_0), (move, r_0, r_m)
    assert _lit_outside(want_0, r_0, r_m), (move, r_0, r_m)  # (and the way back, with the moved scene's)
    _change(sc, via, moved)
    _, st = _on_off(api, sc, monkeypatch, w, h, spp, want_m, st_m, arrays=moved)
    assert st["camera_rays"] == w * h * spp
    _change(sc, via, orig)
    _, st = _on_off(api, sc, monkeypatch, w, h, spp, want_0, st_0)
    assert st["camera_rays"] == w * h * spp


@pytest.mark.parametrize("via", ["update", "rebuild", "set_triangles"])
def test_changed_scenes_under_a_fixed_camera(api, oracle, monkeypatch, via):
    sc = api.Scene(_arrays())
    for move in ("right_0.6", "up_left", "half"):
        _there_and_back(api, oracle, monkeypatch, sc, via, move)
    sc.close()


def test_changed_scenes_with_a_tree_built_on_the_device(api, oracle, monkeypatch):
    sc = api.Scene(_arrays(), device_bvh=True)
    assert sc.info()["builder"] == "ploc"
    for via, move in (("update", "right_0.6"), ("rebuild", "up_left"), ("set_triangles", "half")):
        _there_and_back(api, oracle, monkeypatch, sc, via, move)
    sc.close()


# ---- 7. a grown padding radius
def test_a_grown_padding_radius(api, oracle, monkeypatch):
    """origin_radius grows with the farthest lookfrom a scene has rendered from and never shrinks; the rectangle's margin takes it
    (2^-22 R).  After frames from 5 and from 78 units away the default view and `oblique` still equal their oracle frames."""
    w, h, spp = MAIN
    sc = api.Scene(_arrays())
    cam = _camera(api, oracle, "far_narrow", w / h)
    _on_off(api, sc, monkeypatch, w, h, spp, *_bunny_frame(oracle, cam, w, h, spp), cam=cam)
    far = api.make_camera((40.0, 30.0, 60.0), (0.5, 0.5, -0.5), (0.0, 1.0, 0.0), 2.0, w / h)
    assert np.array_equal(far, oracle.camera((40.0, 30.0, 60.0), (0.5, 0.5, -0.5), (0.0, 1.0, 0.0), 2.0, w / h))
    print("far", bv.rectangle(far, w, h, _arrays()))  # (the pixel step does not dominate the rounding there: the whole frame)
    want, st_c = _bunny_frame(oracle, far, w, h, spp)
    assert want.any()
    _knobs(monkeypatch)
    got, st = _sums(api, sc, w, h, spp, cam=far)
    _check(got, st, want, st_c, "from (40, 30, 60)")
    for view in ("default", "oblique"):
        cam = _camera(api, oracle, view, w / h)
        want, st_c = _oracle_sums(oracle, w, h, spp) if view == "default" else _bunny_frame(oracle, cam, w, h, spp)
        _, st = _on_off(api, sc, monkeypatch, w, h, spp, want, st_c, cam=cam)
        assert st["camera_rays"] == w * h * spp
    sc.close()


# ---- 8. the library's own bounds
def _root_bounds(api, sc):
    """The bounds the library computes the rectangle from: the root's child boxes (rtbg::root_bounds), from rt_scene_tree_copy."""
    recs, _ = _device_tree(api, sc)
    lo, hi = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
    for pair in recs[:2]:
        for box, link in ((pair[0:6], pair[12]), (pair[6:12], pair[13])):
            if link == 0x80000000:  # (kNoChild)
                continue
            b = box.view(np.float32)
            lo, hi = np.minimum(lo, b[:3]), np.maximum(hi, b[3:])
    return lo, hi


def _check_root_bounds(api, oracle, sc, arrays, what):
    from test_background_rect_host import bounds, rect
    w, h = MAIN[:2]
    lo, hi = _root_bounds(api, sc)
    t_lo, t_hi = bounds(arrays)
    assert (lo <= t_lo).all() and (hi >= t_hi).all(), (what, lo, t_lo, hi, t_hi)
    for view in ("default", "oblique"):
        cam = _camera(api, oracle, view, w / h)
        r_root, r_tris = rect(cam, w, h, lo, hi), rect(cam, w, h, t_lo, t_hi)
        print(what, view, "root", r_root, "triangles", r_tris)
        assert bv.covers(r_root, r_tris) and max(abs(a - b) for a, b in zip(r_root, r_tris)) <= 1, (what, view, r_root, r_tris)


def test_root_boxes_hold_the_triangles_after_every_change(api, oracle):
    orig = _arrays()
    for device_bvh in (False, True):
        sc = api.Scene(orig, library=api.tools_lib(), device_bvh=device_bvh)
        _check_root_bounds(api, oracle, sc, orig, ("fresh", device_bvh))
        for via in ("update", "rebuild", "set_triangles"):
            for move in ("right_0.6", "up_left", "half"):
                moved = bv.moved(orig, move)
                _change(sc, via, moved)
                _check_root_bounds(api, oracle, sc, moved, (via, move, device_bvh))
                _change(sc, via, orig)
                _check_root_bounds(api, oracle, sc, orig, (via, move, "back", device_bvh))
        sc.close()
