"""The default kernels against the REFERENCE'S OWN render(), on every frame of tests/golden/ref_render_fixture.npz.  Run with -m gpu.

The fixture holds what the reference's source, compiled for the CPU under oracle/ref_shim.h, computed for the small scenes
of tests/shade_scenes.py: a box centred on the origin (both signs and the |p| < 1/32 branch of the ray-origin offset), glass
of four indices, a mirror at grazing angles, slanted / point / mixed / no / seven lights, an emitter seen directly,
max_bounces 0, 1 and 14, two frames of more than 2^20 camera rays, two seeds.  tests/test_ref_render_pins.py has shown the
pinned oracle EQUAL to that fixture bit for bit; here, through the C-ABI:

  * the shade, camera-ray, shadow-ray and path-ray event totals equal the fixture's sums (a path ray is traced for every
    camera ray and every shade: render.cuh:165-170, 265-274; the BSDF-sampled shadow rays of the reference's ch queue never
    deposit -- the fixture's third deposit count is 0 -- and are not traced);
  * the float image is within the bounds the suite uses against the oracle: RMS < 2e-6 per channel
    and no pixel off by 1e-4; a non-finite fixture pixel must be non-finite here and is left out of the RMS (the maker caps
    them at 1 pixel in 10^4: none in these frames);
  * RT_FLAG_DETERMINISTIC's fixed-point sums equal the oracle's bit for bit -- on the default kernels, under
    RT_FLAG_REFERENCE_WALK, on a device-built tree (RT_SCENE_DEVICE_BVH), and through rt_render_rays_fixed_device fed the
    pinhole's own rays (one-generation frames: tests/raytable.py); with RT_PERSISTENT=0 the events are equal and the image
    holds the float bounds above."""
import os

import numpy as np
import pytest

import raytable
import shade_scenes as ss
from conftest import usable_cpus

pytestmark = pytest.mark.gpu

FIXTURE = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_render_fixture.npz"))
W = 1 << 20


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


_frames, _gpu, _orc = {}, {}, {}


def _frame(name):
    if name not in _frames:
        d = ss.fixture_frame(FIXTURE, name)
        _frames[name] = (d, ss.scene_from_arrays(d, name), *(int(x) for x in d["params"]))
    return _frames[name]


def _scene(api, name, device_bvh=False):
    if (name, device_bvh) not in _gpu:
        _gpu[(name, device_bvh)] = api.Scene(_frame(name)[1], device_bvh=device_bvh)
    return _gpu[(name, device_bvh)]


def _oracle_fixed(oracle, name):
    """The oracle's fixed-point sums of the frame (its float sums ARE the fixture's: tests/test_ref_render_pins.py, re-checked here)."""
    if name not in _orc:
        d, arrays, w, h, spp, max_bounces, seed = _frame(name)
        fixed = np.zeros((h, w, 3), np.int64)
        sc = oracle.scene(arrays)
        _, sums, st = sc.render(d["cam12"], w, h, spp, max_bounces=max_bounces, seed=seed, threads=usable_cpus(), fixed_out=fixed)
        sc.close()
        assert np.array_equal(st["iter_counts"], d["iter_counts"])
        _orc[name] = fixed
    return _orc[name]


def _want_events(d, w, h, spp):
    """Event totals from the fixture's per-iteration queue counts and deposit counts."""
    it = d["iter_counts"].astype(np.int64)
    left, camera = w * h * spp, 0
    for n_gen in it[:, 1]:                      # gen() threads beyond the last camera ray return at once (render.cuh:255)
        camera += min(int(n_gen), left - camera)
    assert camera == w * h * spp
    assert int(d["deposits"][2]) == 0           # the rays the product does not trace never deposit
    return {"camera_rays": camera, "shade_events": int(it[:, 0].sum()), "any_rays": int(it[:, 2].sum()),
            "closest_rays": camera + int(it[:, 0].sum()), "emission_adds": int(d["deposits"][0]), "shadow_adds": int(d["deposits"][1])}


def _assert_events(st, want):
    got = {k: st[k] for k in want}
    assert got == want


def _assert_image(name, img, ref):
    bad = ~np.isfinite(ref)
    assert bad.any(axis=2).sum() * 10000 <= ref.shape[0] * ref.shape[1]
    assert not np.isfinite(img[bad]).any()
    assert np.isfinite(img[~bad]).all()
    diff = np.where(bad, 0.0, img.astype(np.float64) - np.where(bad, 0.0, ref.astype(np.float64)))
    rms = np.sqrt(np.mean(diff ** 2, axis=(0, 1)))
    print(f"[ref-render] {name}: rms {rms.max():.3e} max {np.abs(diff).max():.3e} excluded pixels {int(bad.any(axis=2).sum())}")
    assert rms.max() < 2e-6, rms
    assert np.abs(diff).max() < 1e-4


def _fixed(api, sc, d, w, h, spp, max_bounces, seed, flags=0):
    import torch
    buf = torch.zeros(h * w * 3, dtype=torch.int64, device="cuda")
    st = sc.render_shard_fixed(d["cam12"], w, h, spp, 0, 1, buf.data_ptr(), max_bounces=max_bounces, seed=seed, flags=flags)
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(h, w, 3), st


@pytest.mark.parametrize("name", list(ss.FRAMES))
def test_default_kernels_match_the_reference_frame(api, name):
    d, arrays, w, h, spp, max_bounces, seed = _frame(name)
    img, st = _scene(api, name).render(d["cam12"], w, h, spp, max_bounces=max_bounces, seed=seed)
    _assert_events(st, _want_events(d, w, h, spp))
    _assert_image(name, img, d["image"])


@pytest.mark.parametrize("mode", ["default", "reference_walk", "device_bvh"])
@pytest.mark.parametrize("name", list(ss.FRAMES))
def test_deterministic_sums_equal_the_oracle_that_equals_the_reference(api, oracle, name, mode):
    d, arrays, w, h, spp, max_bounces, seed = _frame(name)
    sc = _scene(api, name, device_bvh=(mode == "device_bvh"))
    got, st = _fixed(api, sc, d, w, h, spp, max_bounces, seed, api.FLAG_REFERENCE_WALK if mode == "reference_walk" else 0)
    want = _want_events(d, w, h, spp)
    if mode == "reference_walk":
        want.pop("closest_rays")  # (that mode counts its walk of the reference's tree on its own)
    _assert_events(st, want)
    ref = _oracle_fixed(oracle, name)
    assert np.array_equal(got, ref), (int((got != ref).sum()), np.argwhere(got != ref)[:4])


@pytest.mark.parametrize("name", list(ss.FRAMES))
def test_round_pipeline_matches_the_reference_frame(api, monkeypatch, name):
    """RT_PERSISTENT=0: one launch per round for every generation.  Equal events; the image to the float bounds."""
    d, arrays, w, h, spp, max_bounces, seed = _frame(name)
    monkeypatch.setenv("RT_PERSISTENT", "0")
    img, st = _scene(api, name).render(d["cam12"], w, h, spp, max_bounces=max_bounces, seed=seed)
    _assert_events(st, _want_events(d, w, h, spp))
    _assert_image(name + " (round pipeline)", img, d["image"])


@pytest.mark.parametrize("name", [n for n, f in ss.FRAMES.items() if f[2] * f[3] * f[4] <= W])
def test_render_rays_fed_the_pinholes_own_rays(api, oracle, name):
    import torch
    d, arrays, w, h, spp, max_bounces, seed = _frame(name)
    o, dirs, _ = raytable.pinhole_table(oracle, d["cam12"], w, h, spp, seed=seed)
    out, st = _scene(api, name).render_rays(torch.from_numpy(o).cuda(), torch.from_numpy(dirs).cuda(), w * h, rays_per_pixel=spp,
                                            max_bounces=max_bounces, seed=seed, fixed=True)
    _assert_events(st, _want_events(d, w, h, spp))
    ref = _oracle_fixed(oracle, name).reshape(-1, 3)
    got = out.cpu().numpy()
    assert np.array_equal(got, ref), (int((got != ref).sum()), np.argwhere(got != ref)[:4])
