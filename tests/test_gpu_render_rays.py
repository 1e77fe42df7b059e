"""GPU tests of rendering along caller-supplied rays (rt_render_rays_device / rt_render_rays_fixed_device).  Run with -m gpu.

The definition is the reference's render() with camera.get_ray() replaced by a table lookup, so a table that holds a
pinhole camera's own rays (tests/raytable.py, held to the oracle by tests/test_render_rays_host.py) must give the CPU
oracle's fixed-point sums and event totals bit for bit: the literal oracle for flags 0, the watertight oracle for
RT_FLAG_WATERTIGHT.  Rays no pinhole makes are pinned at max_bounces = 0 by the oracle-pinned ray queries."""
import numpy as np
import pytest

from conftest import default_camera, usable_cpus
import raygen
import raytable
from test_scene_update_host import deform

pytestmark = pytest.mark.gpu
FLT_MAX = np.float32(3.4028234663852886e38)
# (camera_rays is compared with the frame's ray count, as in every parity test of the suite: the oracle's `sum_gen` counts the
# entries of the reference's gen() queue, slots that find no camera ray left included -- 1 310 720 for a 262 144-ray frame)
EVENTS = [("shade_events", "sum_mat"), ("any_rays", "sum_ah"), ("emission_adds", "emission_adds"),
          ("shadow_adds", "ah_adds"), ("rr_draws", "rr_draws")]


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    return _torch


@pytest.fixture(scope="module")
def gpu_full(api, bunny_full_bsdf):
    return api.Scene(bunny_full_bsdf)


_oracle_cache = {}


def _oracle_fixed(oracle, arrays, key, cam, w, h, spp, max_bounces=10, watertight=False):
    """(fixed-point sums (w * h, 3) int64, stats) of the oracle's render of a frame; once per session and key."""
    key = (key, w, h, spp, max_bounces, watertight, cam.tobytes())
    if key not in _oracle_cache:
        sc = oracle.scene(arrays).set_watertight(watertight)
        fixed = np.zeros((h, w, 3), np.int64)
        _, _, st = sc.render(cam, w, h, spp, max_bounces=max_bounces, threads=usable_cpus(), fixed_out=fixed)
        sc.close()
        _oracle_cache[key] = (fixed.reshape(-1, 3), st)
    return _oracle_cache[key]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assert_events(st, st_ref, n_rays):
    assert st["camera_rays"] == n_rays
    assert st_ref["ch_adds"] == 0
    for g, c in EVENTS:
        assert st[g] == st_ref[c], (g, st[g], c, st_ref[c])


_tables = {}


def _table(oracle, torch, w, h, spp):
    if (w, h, spp) not in _tables:
        o, d, pixel = raytable.pinhole_table(oracle, default_camera(oracle, w / h), w, h, spp)
        _tables[(w, h, spp)] = (_dev(torch, o), _dev(torch, d), pixel)
    return _tables[(w, h, spp)]


# ---- 3. one generation, real rays
@pytest.mark.parametrize("w,h,spp,max_bounces,watertight", [
    (256, 256, 4, 10, False), (256, 256, 4, 10, True), (256, 256, 4, 0, False), (256, 256, 4, 1, False),
    (256, 256, 16, 10, False), (256, 256, 16, 10, True), (256, 256, 16, 0, False), (256, 256, 16, 1, False)])
def test_pinhole_table_gives_the_oracles_sums_and_events(api, torch, oracle, gpu_full, bunny_full_bsdf, w, h, spp, max_bounces, watertight):
    """A quarter of the slots (lockstep rounds over the live slots only) and exactly W rays; d_pixel = NULL."""
    o, d, _ = _table(oracle, torch, w, h, spp)
    ref, st_ref = _oracle_fixed(oracle, bunny_full_bsdf, "full", default_camera(oracle, w / h), w, h, spp, max_bounces, watertight)
    out, st = gpu_full.render_rays(o, d, w * h, rays_per_pixel=spp, max_bounces=max_bounces, fixed=True,
                                   flags=api.FLAG_WATERTIGHT if watertight else 0)
    _assert_events(st, st_ref, w * h * spp)
    assert np.array_equal(out.cpu().numpy(), ref)


# ---- 4. many generations, persistent kernel
def _glass_target(arrays):
    v = np.asarray(arrays.tris, np.float64)[np.asarray(arrays.tri_material) == 4].reshape(-1, 3)
    return v.mean(axis=0)


@pytest.mark.parametrize("w,h,spp,env", [(64, 64, 1024, {}), (50, 40, 700, {}), (50, 40, 700, {"RT_PERSISTENT": "0"})],
                         ids=["4-generations", "1.34-generations", "1.34-generations-round-pipeline"])
def test_many_generations_of_one_ray_match_the_oracles_degenerate_camera(api, torch, oracle, gpu_full, bunny_full_bsdf, monkeypatch,
                                                                         w, h, spp, env):
    """A camera with horizontal = vertical = 0 sends every camera ray along one known ray, so n_rays copies of it are the
    table of oracle.render(cam_degenerate, w, h, spp) for any number of generations: slot order, stream continuation
    across generations, the c / rays_per_pixel rule, the parked final generation and the stop rule, bit for bit.  The ray
    goes through the glass bunny (long paths)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cam, ro, rd = raytable.degenerate_camera(oracle, (0.5, 0.5, 1.5), _glass_target(bunny_full_bsdf))
    n = w * h * spp
    assert n > raytable.W
    o = _dev(torch, ro[None, :]).repeat(n, 1).contiguous()
    d = _dev(torch, rd[None, :]).repeat(n, 1).contiguous()
    ref, st_ref = _oracle_fixed(oracle, bunny_full_bsdf, "full", cam, w, h, spp)
    assert st_ref["sum_mat"] > 2 * n, "the ray must start long paths"
    out, st = gpu_full.render_rays(o, d, w * h, rays_per_pixel=spp, fixed=True)
    _assert_events(st, st_ref, n)
    # the camera path of the same build and knobs, given the degenerate camera, must give the same integers
    cam_sums = torch.zeros((w * h, 3), dtype=torch.int64, device="cuda")
    gpu_full.render_shard_fixed(cam, w, h, spp, 0, 1, cam_sums.data_ptr())
    assert torch.equal(out, cam_sums)
    if not env:
        assert np.array_equal(out.cpu().numpy(), ref)
    else:
        # RT_PERSISTENT=0 (camera frames too): the round pipeline rounds every contribution to 2^-30 on its own, the
        # persistent kernel and the oracle's fixed-point sums round once per camera ray -- so here the events are the
        # oracle's, the integers are the camera path's (above), and the sums agree as two float accumulations of one
        # frame do (the bound of tests/test_gpu_parity.py's shard-sum test)
        np.testing.assert_allclose(out.cpu().numpy() * 2.0 ** -30, ref * 2.0 ** -30, rtol=2e-5, atol=1e-6)


# ---- 5. pixel map
def test_explicit_pixel_map_and_permutation(api, torch, oracle, gpu_full):
    w, h, spp = 256, 256, 4
    o, d, pixel = _table(oracle, torch, w, h, spp)
    base, st0 = gpu_full.render_rays(o, d, w * h, rays_per_pixel=spp, fixed=True)
    same, st1 = gpu_full.render_rays(o, d, w * h, pixel=_dev(torch, pixel), fixed=True)
    assert torch.equal(base, same)
    perm = np.random.default_rng(5).permutation(w * h).astype(np.int32)
    moved, st2 = gpu_full.render_rays(o, d, w * h, pixel=_dev(torch, perm[pixel]), fixed=True)
    assert torch.equal(moved[_dev(torch, perm.astype(np.int64))], base)
    for g in ["camera_rays"] + [g for g, _ in EVENTS]:
        assert st0[g] == st1[g] == st2[g]


# ---- 6. rays no pinhole makes
def _ray_sets(api, gpu, arrays):
    g = np.linspace(0.02, 0.98, 96, dtype=np.float32)
    ox, oy = np.meshgrid(g, g)
    ortho_o = np.stack([ox.ravel(), oy.ravel(), np.full(ox.size, 1.5, np.float32)], axis=1).astype(np.float32)
    ortho_d = np.tile(np.array([0, 0, -1], np.float32), (len(ortho_o), 1))
    cam = api.make_camera()
    po, pd = raygen.camera_rays(cam, 1, 1, 20000, 3)
    tri, t, _, _ = gpu.trace_closest(po, pd, np.full(len(po), FLT_MAX, np.float32))
    bo, bd = raygen.bounce_rays(po, pd, t, tri >= 0, 4)
    ao, ad = raygen.axis_aligned_rays(8192, 6)
    fo, fd = raygen.camera_rays(api.make_camera(lookfrom=(40.0, 30.0, 60.0)), 1, 1, 8192, 7)
    return {"orthographic": (ortho_o, ortho_d), "bounce": (bo, bd), "axis_aligned": (ao, ad), "far_outside": (fo, fd)}


@pytest.mark.parametrize("name", ["orthographic", "bounce", "axis_aligned", "far_outside"])
def test_rays_no_pinhole_makes(api, torch, gpu_full, bunny_full_bsdf, name):
    """max_bounces = 0: the only deposit is bounce-0 emission, so every pixel is L of the light on the triangle
    Scene.query_closest returns for its ray, or 0 -- bit for bit, float entry point.  Then max_bounces = 5 through both
    entry points: finite, reproducible in fixed point, float within two float accumulations' distance of fixed."""
    o_h, d_h = _ray_sets(api, gpu_full, bunny_full_bsdf)[name]
    n = len(o_h)
    assert n > 1000
    o, d = _dev(torch, o_h), _dev(torch, d_h)
    hit, _, _, _ = gpu_full.query_closest(o, d)
    hit = hit.cpu().numpy()
    light_of = np.where(hit >= 0, np.asarray(bunny_full_bsdf.tri_light)[np.maximum(hit, 0)], -1)
    L = np.asarray(bunny_full_bsdf.lights["L"], np.float32).reshape(-1, 3)
    want = np.zeros((n, 3), np.float32)
    want[light_of >= 0] = L[light_of[light_of >= 0]]
    out0, st0 = gpu_full.render_rays(o, d, n, max_bounces=0)
    assert np.array_equal(out0.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert st0["camera_rays"] == n and st0["emission_adds"] == int((light_of >= 0).sum()) and st0["shade_events"] == 0
    fx1, _ = gpu_full.render_rays(o, d, n, max_bounces=5, fixed=True)
    fx2, _ = gpu_full.render_rays(o, d, n, max_bounces=5, fixed=True)
    fl, _ = gpu_full.render_rays(o, d, n, max_bounces=5)
    assert torch.equal(fx1, fx2)
    fl = fl.cpu().numpy()
    assert np.isfinite(fl).all()
    # (every pixel, saturated ones included: the conversion of a clamped sum is a number like any other)
    np.testing.assert_allclose(fl, fx1.cpu().numpy().astype(np.float64) * 2.0 ** -30, rtol=2e-5, atol=1e-6)


# ---- 7. moved geometry
def test_after_a_scene_update_the_table_frame_is_the_oracles_of_the_new_vertices(api, torch, oracle, bunny_full_bsdf):
    import copy
    w, h, spp = 256, 256, 4
    moved = copy.copy(bunny_full_bsdf)
    moved.tris = deform(bunny_full_bsdf.tris)
    sc = api.Scene(bunny_full_bsdf)
    sc.update(moved.tris)
    o, d, _ = _table(oracle, torch, w, h, spp)
    ref, st_ref = _oracle_fixed(oracle, moved, "moved", default_camera(oracle, w / h), w, h, spp)
    out, st = sc.render_rays(o, d, w * h, rays_per_pixel=spp, fixed=True)
    sc.close()
    _assert_events(st, st_ref, w * h * spp)
    assert np.array_equal(out.cpu().numpy(), ref)


# ---- 8. stream order
def test_call_is_ordered_on_the_callers_stream(api, torch, oracle, gpu_full, bunny_full_bsdf):
    w, h, spp = 256, 256, 4
    o, d, _ = _table(oracle, torch, w, h, spp)
    ref, _ = _oracle_fixed(oracle, bunny_full_bsdf, "full", default_camera(oracle, w / h), w, h, spp)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        junk = torch.randn(4096, 4096, device="cuda")
        for _ in range(8):
            junk = junk @ junk * 1e-3  # keeps the stream busy while the next kernels are queued
        o2 = (o * 2.0 - o).contiguous() + (junk[0, 0] * 0.0).nan_to_num(0.0, 0.0, 0.0)
        d2 = d.clone()
        acc = torch.full((w * h, 3), 123, dtype=torch.int64, device="cuda")
        acc.zero_()
        out, _ = gpu_full.render_rays(o2, d2, w * h, rays_per_pixel=spp, fixed=True, out=acc)
    assert torch.equal(o2, o)
    assert np.array_equal(out.cpu().numpy(), ref)


# ---- 9. errors write nothing
def test_errors_return_a_message_and_leave_the_sum_buffer_untouched(api, torch, gpu_full):
    n, npix = 4096, 1024
    o_h, d_h = raygen.camera_rays(api.make_camera(), 1, 1, n, 11)
    o, d = _dev(torch, o_h), _dev(torch, d_h)
    pixel = _dev(torch, (np.arange(n) % npix).astype(np.int32))
    sentinel = 0x5A5A5A5A

    def refused(pattern, fixed=False, **kw):
        args = dict(o_ptr=o.data_ptr(), d_ptr=d.data_ptr(), pixel_ptr=pixel.data_ptr(), n_rays=n, n_pixels=npix, rays_per_pixel=1, flags=0)
        args.update(kw)
        buf = torch.full((npix, 3), sentinel, dtype=torch.int64 if fixed else torch.int32, device="cuda")
        if args.pop("null_sum", False):
            ptr = 0
        else:
            ptr = buf.data_ptr()
        with pytest.raises(api.RtError, match=pattern):
            gpu_full.render_rays_device(d_sum_ptr=ptr, fixed=fixed, **args)
        torch.cuda.synchronize()
        assert bool((buf == sentinel).all())

    for fixed in (False, True):
        for bad, count in ((float("nan"), 3), (float("inf"), 2), (2.0 ** 126, 1)):
            dd = d.clone()
            dd[torch.arange(count, device="cuda") * 7 + 5, 1] = bad
            refused(f"{count} of {n} directions", fixed, d_ptr=dd.data_ptr())
        for bad in (-1, npix):
            pp = pixel.clone()
            pp[17] = bad
            pp[n - 1] = bad
            refused(f"2 of {n} pixel indices", fixed, pixel_ptr=pp.data_ptr())
        refused("n_rays = 0", fixed, n_rays=0)
        refused("falls on pixel", fixed, pixel_ptr=0, rays_per_pixel=3, n_pixels=npix)  # ray 4095 -> pixel 1365 of 1024
        refused("rays_per_pixel = 0", fixed, pixel_ptr=0, rays_per_pixel=0)
        refused("n_pixels = 0", fixed, n_pixels=0)
        refused("null d_origin_xyz", fixed, o_ptr=0)
        refused("null d_dir_xyz", fixed, d_ptr=0)
        refused("null sum buffer", fixed, null_sum=True)
        refused("RT_FLAG_REFERENCE_WALK", fixed, flags=api.FLAG_REFERENCE_WALK)
        refused("RT_FLAG_RNG_PER_SAMPLE", fixed, flags=api.FLAG_RNG_PER_SAMPLE)
        refused("RT_FLAG_REFERENCE_WALK", fixed, flags=api.FLAG_REFERENCE_WALK | api.FLAG_WATERTIGHT)
        refused("max_bounces", fixed, max_bounces=-1)


def test_a_nan_origin_is_legal_and_that_ray_deposits_nothing(api, torch, gpu_full):
    n = 4096
    o_h, d_h = raygen.camera_rays(api.make_camera(), 1, 1, n, 12)
    o, d = _dev(torch, o_h), _dev(torch, d_h)
    clean, _ = gpu_full.render_rays(o, d, n, max_bounces=5, fixed=True)
    assert int((clean != 0).any(dim=1).sum()) > n // 2
    o2 = o.clone()
    idx = torch.tensor([0, 63, 64, 1000, n - 1], device="cuda")
    o2[idx, 0] = float("nan")
    out, st = gpu_full.render_rays(o2, d, n, max_bounces=5, fixed=True)
    assert st["camera_rays"] == n
    assert bool((out[idx] == 0).all())
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[idx] = False
    assert torch.equal(out[keep], clean[keep])
