"""The table form of the oracle's renders (OracleScene.render_table) against its camera form.  No GPU.

render_table takes camera ray c's ray and pixel from a table where render() calls camera_get_ray; one text serves both.  So a
pinhole's own table (raytable.pinhole_table, raytable_keyed.keyed_pinhole_table: the rays the camera form makes) must give the
camera form's int64 sums and event totals exactly, in the reference's mode (literal and watertight hits) and in the per-sample
mode.  The GPU tests of whole paths from rays no pinhole makes (tests/test_gpu_ray_family_paths.py) lean on this."""
import numpy as np
import pytest

from conftest import default_camera, usable_cpus
import raytable
import raytable_keyed

TOTALS = ("sum_mat", "sum_ah", "sum_ch", "emission_adds", "ah_adds", "ch_adds", "rr_draws", "rr_kills")
W, H, SPP = 64, 48, 4


@pytest.mark.parametrize("max_bounces", [5, 0])
@pytest.mark.parametrize("watertight", [False, True], ids=["literal", "watertight"])
def test_a_pinholes_own_table_gives_the_camera_forms_sums(oracle, bunny_full_bsdf, watertight, max_bounces):
    cam = default_camera(oracle, W / H)
    sc = oracle.scene(bunny_full_bsdf).set_watertight(watertight)
    want = np.zeros((H, W, 3), np.int64)
    _, _, st = sc.render(cam, W, H, SPP, max_bounces=max_bounces, threads=usable_cpus(), fixed_out=want)
    o, d, pixel = raytable.pinhole_table(oracle, cam, W, H, SPP)
    for pix, rpp in ((None, SPP), (pixel, 1)):
        got, st_t = sc.render_table(o, d, W * H, pixel=pix, rays_per_pixel=rpp, max_bounces=max_bounces, threads=usable_cpus())
        assert np.array_equal(got, want.reshape(-1, 3))
        assert {k: st_t[k] for k in TOTALS + ("iterations", "sum_gen")} == {k: st[k] for k in TOTALS + ("iterations", "sum_gen")}
    assert want.any() and (max_bounces == 0 or st["sum_mat"] > W * H * SPP)


@pytest.mark.parametrize("max_bounces", [5, 0])
def test_a_pinholes_own_keyed_table_gives_the_per_sample_forms_sums(oracle, bunny_full_bsdf, max_bounces):
    cam = default_camera(oracle, W / H)
    sc = oracle.scene(bunny_full_bsdf)
    seed = 9
    want = np.zeros((H, W, 3), np.int64)
    _, _, st = sc.render(cam, W, H, SPP, max_bounces=max_bounces, seed=seed, threads=usable_cpus(), fixed_out=want, rng_mode="per_sample")
    n = W * H * SPP
    o, d, pixel = raytable_keyed.keyed_pinhole_table(oracle, cam, W, H, SPP, seed, range(n))
    for pix in (None, pixel):
        got, st_t = sc.render_table(o, d, W * H, pixel=pix, rays_per_pixel=SPP, max_bounces=max_bounces, seed=seed, keyed=True)
        assert np.array_equal(got, want.reshape(-1, 3))
        assert {k: st_t[k] for k in TOTALS + ("sum_gen",)} == {k: st[k] for k in TOTALS + ("sum_gen",)}
    # a strided key range: every third key from 5 on, in two chunks that add up
    keys = list(range(5, n, 3))
    o, d, pixel = raytable_keyed.keyed_pinhole_table(oracle, cam, W, H, SPP, seed, keys)
    whole, _ = sc.render_table(o, d, W * H, rays_per_pixel=SPP, max_bounces=max_bounces, seed=seed, keyed=True, key_first=5, key_stride=3)
    m = len(keys) // 2
    a, _ = sc.render_table(o[:m], d[:m], W * H, pixel=pixel[:m], max_bounces=max_bounces, seed=seed, keyed=True, key_first=5, key_stride=3)
    b, _ = sc.render_table(o[m:], d[m:], W * H, pixel=pixel[m:], max_bounces=max_bounces, seed=seed, keyed=True, key_first=keys[m], key_stride=3)
    assert np.array_equal(a + b, whole) and whole.any()
