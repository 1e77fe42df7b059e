"""GPU test of the one body behind every table's validation on the device (validate_table: the prepasses, the read-back, the
refusals), through its four users: rt_query_closest_device, rt_render_rays_fixed_device, rt_render_rays_keyed_fixed_device
and rt_render_aov_rays_fixed_device.  A table of 65 rows (one wave and one row) over 8 pixels on the Cornell box without the
bunny, with a NaN direction or a pixel index of n_pixels in its LAST row: the entry point's own message with the counts, a
zero-filled output left untouched, and the good table accepted and answered as before straight afterwards.

What the last step can and cannot show: the reference for it is the same library's result on a second scene of the same
arrays that no refusal ever touched (computed once; for the query the oracle's triangles as well).  It catches a refusal that
leaves the scene unusable or changes its answers -- a lock still held, a half-made scratch, the counts of the refused table
reported again -- not a wrong answer that both scenes share: what a good table gives is pinned to the oracle in
test_gpu_query.py, test_gpu_render_rays.py, test_gpu_render_rays_keyed.py and test_gpu_aov.py."""
import ctypes

import numpy as np
import pytest

from conftest import default_camera
import raytable_keyed as rk

pytestmark = pytest.mark.gpu

N, N_PIXELS = 65, 8
FLT_MAX = np.float32(3.4028234663852886e38)
USERS = ("rt_query_closest_device", "rt_render_rays_fixed_device", "rt_render_rays_keyed_fixed_device", "rt_render_aov_rays_fixed_device")
CASES = [(u, bad) for u in USERS for bad in ("nan_direction", "pixel_past_the_end") if not (u == USERS[0] and bad == "pixel_past_the_end")]


def _run(torch, scene, user, o, d, pixel):
    """One call on device tensors into zero-filled outputs -> (rc, message, [outputs])."""
    c = ctypes.c_void_p
    L, h = scene.L, scene.h
    if user == USERS[0]:
        outs = [torch.zeros(N, dtype=torch.int32, device="cuda")] + [torch.zeros(N, dtype=torch.float32, device="cuda") for _ in range(3)]
        rc = L.rt_query_closest_device(h, 0, N, c(o.data_ptr()), c(d.data_ptr()), None, *(c(x.data_ptr()) for x in outs), None)
    elif user == USERS[1]:
        outs = [torch.zeros((N_PIXELS, 3), dtype=torch.int64, device="cuda")]
        rc = L.rt_render_rays_fixed_device(h, N, c(o.data_ptr()), c(d.data_ptr()), c(pixel.data_ptr()), 1, N_PIXELS, 10, 1, 0,
                                           c(outs[0].data_ptr()), None, None)
    elif user == USERS[2]:
        outs = [torch.zeros((N_PIXELS, 3), dtype=torch.int64, device="cuda")]
        rc = L.rt_render_rays_keyed_fixed_device(h, N, c(o.data_ptr()), c(d.data_ptr()), c(pixel.data_ptr()), 1, N_PIXELS, 10, 1, 0, 1, 0,
                                                 c(outs[0].data_ptr()), None, None)
    else:
        outs = [torch.zeros((N_PIXELS, 11), dtype=torch.int64, device="cuda")]
        rc = L.rt_render_aov_rays_fixed_device(h, N, c(o.data_ptr()), c(d.data_ptr()), c(pixel.data_ptr()), 1, N_PIXELS, 0, 1, 0,
                                               c(outs[0].data_ptr()), None, None, None)
    torch.cuda.synchronize()
    return rc, L.rt_last_error().decode(), [x.cpu().numpy() for x in outs]


@pytest.fixture(scope="module")
def box(oracle):
    """(the refused scene, the good table on the device and the host, what each user gives for it on an untouched scene)"""
    import torch
    from rtcuda_amd import api, scenes
    api.lib()
    arrays = scenes.cornell_bunny("full_bsdf", bunny=False)
    o, d, _ = rk.keyed_pinhole_table(oracle, default_camera(oracle, 13 / 5), 13, 5, 1, 1, range(N))
    pixel = (np.arange(N) % N_PIXELS).astype(np.int32)
    table = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (o, d, pixel))
    untouched = api.Scene(arrays)
    want = {}
    for user in USERS:
        rc, msg, outs = _run(torch, untouched, user, *table)
        assert rc == 0, msg
        want[user] = outs
    untouched.close()
    tri = oracle.scene(arrays).trace_closest(o, d, np.full(N, FLT_MAX, np.float32))[0]
    assert np.array_equal(want[USERS[0]][0], tri) and (tri >= 0).any() and (tri < 0).any()  # (the wide view sees the box and past it)
    assert all(w[0].any() for w in want.values())  # (every user writes something for the good table)
    gpu = api.Scene(arrays)
    yield torch, gpu, table, (o, d, pixel), want
    gpu.close()


@pytest.mark.parametrize("user,bad", CASES, ids=["%s-%s" % c for c in CASES])
def test_a_bad_last_row_is_refused_by_name_writes_nothing_and_leaves_the_scratch_clean(box, user, bad):
    torch, gpu, table, (o, d, pixel), want = box
    if bad == "nan_direction":
        d2 = d.copy()
        d2[N - 1, 1] = np.nan
        bad_table = (table[0], torch.from_numpy(d2).cuda(), table[2])
        message = f"{user}: 1 of {N} directions are not finite or reach 2^126"
    else:
        p2 = pixel.copy()
        p2[N - 1] = N_PIXELS
        bad_table = (table[0], table[1], torch.from_numpy(p2).cuda())
        message = f"{user}: 1 of {N} pixel indices are outside 0 .. {N_PIXELS - 1}"
    rc, msg, outs = _run(torch, gpu, user, *bad_table)
    assert rc != 0 and msg == message, (rc, msg)
    assert not any(x.any() for x in outs), "a refused call wrote into its output"
    rc, msg, outs = _run(torch, gpu, user, *table)
    assert rc == 0, msg
    for got, ref in zip(outs, want[user]):
        assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (user, "differs from the untouched scene's result")
