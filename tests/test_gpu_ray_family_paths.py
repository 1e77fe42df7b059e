"""Whole paths from rays no pinhole makes, against the table form of the oracle (OracleScene.render_table).  Run with -m gpu.

Until now such tables were compared only with themselves (repeatability, partition invariance, bounce-0 emission): the oracle
could only render from a camera.  Its table form (held to the camera form by tests/test_ray_table_oracle_host.py) takes the
rays as given, so the int64 sums and the six event totals of
  * rt_render_rays_fixed_device, flags 0 (literal oracle) and RT_FLAG_WATERTIGHT (watertight oracle),
  * rt_render_rays_keyed_fixed_device (the per-sample form, a strided key range),
and the first-hit features of rt_render_aov_rays_fixed_device (aov_expected.table_expected; RT_FLAG_WATERTIGHT fed by
EXHAUSTIVE SEARCH) must be the oracle's exactly -- on rays aimed at vertices, parallel rays through vertices, bounce rays that
start ON the surface, rays from far outside and the orthographic grid.  8 192 rays per table, max_bounces 5 and 0.
"""
import numpy as np
import pytest

import aov_expected
from conftest import usable_cpus
import ray_families as rf
import raygen

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N = 8192
TABLES = ("vertex_aimed", "parallel_through", "surface_start", "far_outside", "orthographic")
EVENTS = [("shade_events", "sum_mat"), ("any_rays", "sum_ah"), ("emission_adds", "emission_adds"),
          ("shadow_adds", "ah_adds"), ("rr_draws", "rr_draws")]
KEY_FIRST, KEY_STRIDE, SEED = 7, 3, 5


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


@pytest.fixture(scope="module")
def gpu_full(api, bunny_full_bsdf):
    sc = api.Scene(bunny_full_bsdf)
    yield sc
    sc.close()


_cache = {}


def _oracle_scene(oracle, arrays, watertight):
    if ("scene", watertight) not in _cache:
        _cache["scene", watertight] = oracle.scene(arrays).set_watertight(watertight)
    return _cache["scene", watertight]


def _table(api, oracle, arrays, name):
    """(o, d) float32 (N, 3) of a table, made once per session."""
    if name not in _cache:
        if name == "vertex_aimed":
            o, d = rf.vertex_aimed(arrays.tris, N, 301, "box")
        elif name == "parallel_through":
            o, d = rf.parallel_through(arrays.tris, N, 302, "vertex", "plus_zero")
        elif name == "surface_start":  # bounce rays that start exactly on the surface the oracle's walk finds (eps = 0)
            po, pd = raygen.camera_rays(api.make_camera(), 1, 1, 6 * N, 303)
            tri, t, _, _ = _oracle_scene(oracle, arrays, False).trace_closest(po, pd, np.full(len(po), rf.FLT_MAX, np.float32),
                                                                                threads=usable_cpus())
            o, d = raygen.bounce_rays(po, pd, t, tri >= 0, 304, eps=0.0)
        elif name == "far_outside":
            o, d = raygen.camera_rays(api.make_camera(lookfrom=(40.0, 30.0, 60.0)), 1, 1, N, 305)
        else:
            g = np.linspace(0.02, 0.98, 96, dtype=np.float32)
            ox, oy = np.meshgrid(g, g)
            o = np.stack([ox.ravel(), oy.ravel(), np.full(ox.size, 1.5, np.float32)], axis=1).astype(np.float32)
            d = np.tile(np.array([0, 0, -1], np.float32), (len(o), 1))
        assert len(o) >= N, (name, len(o))
        _cache[name] = np.ascontiguousarray(o[:N]), np.ascontiguousarray(d[:N])
    return _cache[name]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assert_events(st, st_ref):
    assert st["camera_rays"] == N
    got = {g: st[g] for g, _ in EVENTS}
    want = {g: st_ref[c] for g, c in EVENTS}
    print(got, want)
    assert got == want


@pytest.mark.parametrize("max_bounces", [5, 0])
@pytest.mark.parametrize("watertight", [False, True], ids=["flags0-literal", "watertight"])
@pytest.mark.parametrize("name", TABLES)
def test_render_rays_fixed_gives_the_table_oracles_sums_and_events(api, oracle, gpu_full, bunny_full_bsdf, name, watertight, max_bounces):
    o, d = _table(api, oracle, bunny_full_bsdf, name)
    want, st_ref = _oracle_scene(oracle, bunny_full_bsdf, watertight).render_table(o, d, N, max_bounces=max_bounces, seed=SEED,
                                                                                   threads=usable_cpus())
    out, st = gpu_full.render_rays(_dev(o), _dev(d), N, max_bounces=max_bounces, seed=SEED, fixed=True,
                                   flags=api.FLAG_WATERTIGHT if watertight else 0)
    _assert_events(st, st_ref)
    got = out.cpu().numpy()
    print(name, "pixels that differ:", int((got != want).any(axis=1).sum()), "lit pixels:", int(want.any(axis=1).sum()))
    assert np.array_equal(got, want)
    # (with max_bounces = 0 only a ray that hits a light deposits anything: the two light triangles own 4 of 35 000 vertices)
    assert st_ref["ch_adds"] == 0 and (name == "far_outside" or max_bounces == 0 or want.any())


@pytest.mark.parametrize("max_bounces", [5, 0])
@pytest.mark.parametrize("name", TABLES)
def test_render_rays_keyed_fixed_gives_the_table_oracles_sums_and_events(api, oracle, gpu_full, bunny_full_bsdf, name, max_bounces):
    o, d = _table(api, oracle, bunny_full_bsdf, name)
    pixel = np.arange(N, dtype=np.int32)
    want, st_ref = _oracle_scene(oracle, bunny_full_bsdf, True).render_table(o, d, N, pixel=pixel, max_bounces=max_bounces, seed=SEED,
                                                                             keyed=True, key_first=KEY_FIRST, key_stride=KEY_STRIDE)
    out, st = gpu_full.render_rays_keyed(_dev(o), _dev(d), N, pixel=_dev(pixel), key_first=KEY_FIRST, key_stride=KEY_STRIDE,
                                         max_bounces=max_bounces, seed=SEED, fixed=True)
    _assert_events(st, st_ref)
    got = out.cpu().numpy()
    print(name, "pixels that differ:", int((got != want).any(axis=1).sum()), "lit pixels:", int(want.any(axis=1).sum()))
    assert np.array_equal(got, want)


class _Brute:
    """An OracleScene whose closest hit is exhaustive search's (what aov_expected.sample_features asks of its scene)."""

    def __init__(self, osc):
        self.arrays, self.osc = osc.arrays, osc

    def trace_closest(self, o, d, tmax):
        return self.osc.trace_closest_brute(o, d, tmax, threads=usable_cpus())


@pytest.mark.parametrize("watertight", [False, True], ids=["flags0-literal", "watertight-brute"])
@pytest.mark.parametrize("name", TABLES)
def test_render_aov_rays_gives_the_expected_features(api, oracle, gpu_full, bunny_full_bsdf, name, watertight):
    o, d = _table(api, oracle, bunny_full_bsdf, name)
    pixel = (np.arange(N, dtype=np.int32) * 5) % 4096  # two rows per pixel
    osc = _oracle_scene(oracle, bunny_full_bsdf, False)
    want, _ = aov_expected.table_expected(oracle, _Brute(osc) if watertight else osc, o, d, pixel, 4096)
    out, _, st = gpu_full.render_aov_rays(_dev(o), _dev(d), 4096, pixel=_dev(pixel), flags=api.FLAG_WATERTIGHT if watertight else 0)
    got = out.cpu().numpy()
    print(name, "pixels that differ:", int((got != want).any(axis=1).sum()), "hits:", int(want[:, aov_expected.HITS].sum()))
    assert np.array_equal(got, want)
    # (not empty-handed; half of the surface-start rays leave into the surface they start on, the far rays mostly miss the box)
    assert name == "far_outside" or want[:, aov_expected.HITS].sum() > N // 4
