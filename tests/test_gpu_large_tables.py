"""Scenes with more than 64 materials or lights on the GPU.  Run with -m gpu.

rt_render_shard stages the shading tables in LDS only when n_mats <= 64 and n_lights <= 64 (kLdsTable); above that the
LDS_TABLES = false builds of k_advance and of every k_paths variant run, with the tables read from global memory and no
tables in front of the k_paths LDS top-of-tree and uniforms.  The BASELINE scenes (<= 6 materials, <= 16 lights) never
reach them.  The scenes of tests/table_scenes.py do, at the gate, past it on either count, over several k_build_tables
blocks, and at the C-ABI's limits (65535 materials: material id 0xfffe; 32766 lights: light 32765 packs to 32766 << 16).

Bars, as in tests/test_gpu_multigen.py: event totals EQUAL to the oracle's, RT_FLAG_DETERMINISTIC sums bit-equal to the
oracle's fixed-point sums, image RMS < 2e-6 and no pixel off by 1e-4.  Default kernels and RT_FLAG_REFERENCE_WALK against
the literal oracle, RT_FLAG_WATERTIGHT against the watertight oracle.  The padding tests need no oracle: unused materials
appended to the full-BSDF scene move it across the LDS gate and must change no bit.
"""
import dataclasses

import numpy as np
import pytest

import table_scenes as ts
from conftest import default_camera, usable_cpus
from test_gpu_multigen import _assert_same_events, _max_abs, _rms

pytestmark = pytest.mark.gpu

W = 1 << 20
EVENTS = ("camera_rays", "shade_events", "any_rays", "emission_adds", "shadow_adds", "rr_draws")
FRAMES = {
    "one_gen": (128, 96, 16),     # <= W camera rays: the lockstep k_advance + k_trace pipeline only
    "multi_gen": (256, 256, 20),  # 1.25 generations: k_paths, then the lockstep final generation
}
SIZES = [
    (64, 64),                        # LDS tables, s_tab of k_advance exactly full (1856 dwords)
    (65, 8),                         # global tables, by the material count
    (8, 65),                         # global tables, by the light count
    (300, 300),                      # five k_build_tables blocks
    (ts.MAX_MATS, ts.MAX_LIGHTS),    # the C-ABI's limits
]
MODES = ["default", "reference_walk", "watertight"]


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


def _flags(api, mode):
    return {"default": 0, "reference_walk": api.FLAG_REFERENCE_WALK, "watertight": api.FLAG_WATERTIGHT}[mode]


# ---- module-level caches: one table scene per size, one GPU scene per (scene, creation-time knobs), one oracle scene per
# (size, box-test mode) and one oracle render per distinct argument tuple
_arrays_cache, _gpu_cache, _osc_cache, _orc_cache = {}, {}, {}, {}


def _arrays(size):
    if size not in _arrays_cache:
        _arrays_cache[size] = ts.table_scene(*size)
    return _arrays_cache[size]


def _gpu(api, arrays, key=None):
    key = key or (arrays.name,)
    if key not in _gpu_cache:
        _gpu_cache[key] = api.Scene(arrays)
    return _gpu_cache[key]


def _oracle_render(oracle, size, frame, watertight, slot_lo=0, slot_hi=W):
    """(image, fixed-point sums, stats) of the oracle's render of a table scene."""
    key = (size, frame, watertight, slot_lo, slot_hi)
    if key not in _orc_cache:
        if (size, watertight) not in _osc_cache:
            _osc_cache[(size, watertight)] = oracle.scene(_arrays(size)).set_watertight(watertight)
        w, h, spp = FRAMES[frame]
        fixed = np.zeros((h, w, 3), np.int64)
        img, _, st = _osc_cache[(size, watertight)].render(default_camera(oracle, w / h), w, h, spp, slot_lo=slot_lo,
                                                           slot_hi=slot_hi, threads=usable_cpus(), fixed_out=fixed)
        _orc_cache[key] = (img, fixed, st)
    return _orc_cache[key]


def _fixed(api, sc, frame, flags=0, shards=1, only=None):
    """RT_FLAG_DETERMINISTIC sums of a frame, from `shards` slot-range shards added into one buffer (or shard `only` of
    them) -> (int64 (h, w, 3), summed event totals)."""
    import torch
    w, h, spp = FRAMES[frame]
    cam = api.make_camera(aspect=w / h)
    buf = torch.zeros(h * w * 3, dtype=torch.int64, device="cuda")
    ev = dict.fromkeys(EVENTS, 0)
    for r in (range(shards) if only is None else [only]):
        st = sc.render_shard_fixed(cam, w, h, spp, r, shards, buf.data_ptr(), flags=flags)
        for k in EVENTS:
            ev[k] += st[k]
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(h, w, 3), ev


def _assert_equal_sums(got, want):
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:4])


# ------------------------------------------------------------------------------------------- (a) table sizes vs the oracle
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("size", SIZES, ids=[f"{m}x{n}" for m, n in SIZES])
def test_large_table_scene_matches_oracle(api, oracle, size, frame, mode):
    w, h, spp = FRAMES[frame]
    assert (w * h * spp > W) == (frame == "multi_gen")
    sc = _gpu(api, _arrays(size))
    flags = _flags(api, mode)
    img_c, fixed_c, st_c = _oracle_render(oracle, size, frame, mode == "watertight")
    assert st_c["sum_mat"] > 0.5 * w * h * spp and st_c["emission_adds"] > 0
    img_g, st_g = sc.render(api.make_camera(aspect=w / h), w, h, spp, flags=flags)
    _assert_same_events(st_g, st_c, w * h * spp)
    rms = _rms(img_g, img_c)
    assert rms.max() < 2e-6, rms
    assert _max_abs(img_g, img_c) < 1e-4
    got, ev = _fixed(api, sc, frame, flags)
    _assert_same_events(ev, st_c, w * h * spp)
    _assert_equal_sums(got, fixed_c)


@pytest.mark.parametrize("size", [(65, 8), (ts.MAX_MATS, ts.MAX_LIGHTS)], ids=["65x8", "max"])
def test_slot_shards_of_a_global_table_scene(api, oracle, size):
    """8 slot-range shards (the MIN_WAVES = 2 build of k_paths, each what one rank of an 8-GPU run renders) with the tables
    in global memory: they add up to the full frame exactly, and a shard is the oracle's render of its slot range."""
    frame, shards, r = "multi_gen", 8, 3
    sc = _gpu(api, _arrays(size))
    full, ev_full = _fixed(api, sc, frame)
    acc, ev_acc = _fixed(api, sc, frame, shards=shards)
    assert ev_acc == ev_full
    _assert_equal_sums(acc, full)
    _assert_equal_sums(full, _oracle_render(oracle, size, frame, False)[1])
    n = W // shards
    _, want, st_c = _oracle_render(oracle, size, frame, False, slot_lo=r * n, slot_hi=(r + 1) * n)
    part, ev = _fixed(api, sc, frame, shards=shards, only=r)
    assert ev["shade_events"] == st_c["sum_mat"] and ev["any_rays"] == st_c["sum_ah"]
    assert ev["shadow_adds"] == st_c["ah_adds"] and ev["rr_draws"] == st_c["rr_draws"]
    assert ev["emission_adds"] == st_c["emission_adds"]
    assert part.any()
    _assert_equal_sums(part, want)


# ------------------------------------------------------------------------ (b) LDS vs global tables: padding changes no bit
PAD_SETTINGS = {
    # name: (flags, knobs, shards)
    "default": (0, {}, 1),
    "watertight": ("FLAG_WATERTIGHT", {}, 1),
    "reference_walk": ("FLAG_REFERENCE_WALK", {}, 1),
    "rng_per_sample": ("FLAG_RNG_PER_SAMPLE", {}, 1),
    "shards8": (0, {}, 8),
    "binary_tree": (0, {"RT_BVH_WIDE": "0"}, 1),                              # (read at scene creation)
    "round_pipeline": (0, {"RT_PERSISTENT": "0"}, 1),                         # k_advance for every generation
}


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("setting", list(PAD_SETTINGS))
def test_padding_the_materials_past_the_lds_gate_changes_no_bit(api, bunny_full_bsdf, monkeypatch, setting, frame):
    """The full-BSDF scene (6 materials: LDS tables) and its copies padded with unused materials to 65 and 65535 (global
    tables): equal event totals and equal fixed-point sums in every mode, build and schedule."""
    flags, knobs, shards = PAD_SETTINGS[setting]
    flags = getattr(api, flags) if isinstance(flags, str) else flags
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    tree = knobs.get("RT_BVH_WIDE", "")
    results = []
    for pad in (None, 65, ts.MAX_MATS):
        arrays = bunny_full_bsdf if pad is None else ts.padded(bunny_full_bsdf, pad)
        assert ts.lds_tables(len(arrays.materials), len(arrays.lights)) == (pad is None)
        results.append(_fixed(api, _gpu(api, arrays, (arrays.name, tree)), frame, flags, shards))
    (base, ev), *others = results
    w, h, spp = FRAMES[frame]
    assert ev["camera_rays"] == w * h * spp and ev["shade_events"] > 0 and base.any()
    for got, ev_p in others:
        assert ev_p == ev
        _assert_equal_sums(got, base)


# ---------------------------------------------------------------------------- (c) updates and replicas with large tables
def _move_some_area_lights(arrays):
    """Every other area light of the grid, lowered and grown about its own centre: new vertices for k_build_tables' light
    rows (over two blocks for 100 lights)."""
    tris = np.array(arrays.tris, np.float32)
    area = np.flatnonzero(arrays.lights["type"] == 1)
    moved = arrays.lights["tri"][area[::2]]
    v = tris[moved].reshape(-1, 3, 3)
    c = v.mean(axis=1, keepdims=True)
    v = (v - c) * np.float32(1.3) + c - np.array([0.0, 0.03, 0.0], np.float32)
    tris[moved] = v.reshape(-1, 9).astype(np.float32)
    return tris, moved


@pytest.mark.parametrize("via", ["host", "device"])
def test_moving_area_lights_of_a_global_table_scene(api, oracle, via):
    import torch
    arrays = ts.table_scene(8, 100)
    assert not ts.lds_tables(8, 100)
    new, moved = _move_some_area_lights(arrays)
    assert len(moved) >= 16 and (arrays.lights["tri"][arrays.lights["type"] == 1] >= 0).all()
    fresh_arrays = dataclasses.replace(arrays, tris=new)
    frame = "one_gen"
    a = api.Scene(arrays)
    before, _ = _fixed(api, a, frame)
    if via == "host":
        a.update(new)
    else:
        dev = torch.from_numpy(new).cuda()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            a.update_device(dev.data_ptr(), stream=stream.cuda_stream)
        torch.cuda.synchronize()
    b = api.Scene(fresh_arrays)
    w, h, spp = FRAMES[frame]
    cam = api.make_camera(aspect=w / h)
    for flags in (api.FLAG_DETERMINISTIC, api.FLAG_DETERMINISTIC | api.FLAG_WATERTIGHT):
        ia, sa = a.render(cam, w, h, spp, flags=flags)
        ib, sb = b.render(cam, w, h, spp, flags=flags)
        assert {k: sa[k] for k in EVENTS} == {k: sb[k] for k in EVENTS}, flags
        assert ia.tobytes() == ib.tobytes(), flags
    after, ev = _fixed(api, a, frame)
    assert not np.array_equal(before, after)
    want = np.zeros_like(after)
    _, _, st_c = oracle.scene(fresh_arrays).render(default_camera(oracle, w / h), w, h, spp, threads=usable_cpus(),
                                                   fixed_out=want)
    _assert_same_events(ev, st_c, w * h * spp)
    _assert_equal_sums(after, want)


@pytest.mark.parametrize("frame", list(FRAMES))
def test_render_multi_of_a_global_table_scene(api, frame):
    """rt_render_multi over a device listed twice (two shards, each with its own copy of the tables where the devices
    differ) is the single-device render, bit for bit."""
    sc = _gpu(api, _arrays((300, 300)))
    w, h, spp = FRAMES[frame]
    cam = api.make_camera(aspect=w / h)
    single, st_s = sc.render(cam, w, h, spp, flags=api.FLAG_DETERMINISTIC)
    multi, st_m = sc.render_multi(cam, w, h, spp, [0, 0], flags=api.FLAG_DETERMINISTIC)
    assert {k: st_m[k] for k in EVENTS} == {k: st_s[k] for k in EVENTS}
    assert multi.tobytes() == single.tobytes()
