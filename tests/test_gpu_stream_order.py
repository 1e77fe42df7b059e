"""GPU tests of the header's "ordered on `stream`": inputs that arrive LATE on a busy, non-blocking side stream.  Run with -m gpu.

The rest of the suite calls the library with inputs that were finished and synchronised before the call.  Here every input the
call depends on is still on its way when the call is made: one side stream `s` (PyTorch's side streams are non-blocking: the
null stream does not wait for them) first gets delay work, then the copies that replace a DECOY in the call's input buffers by
the real input, then the zeroing of what the call adds to and the poisoning of what it overwrites, then the library call.  A
single launch, memset or copy of the library that went to another stream would read the decoy, or add to sums that are zeroed
afterwards, or be overwritten by the poison.  Decoys are valid inputs that give another answer (finite rays, indices in range,
finite vertices): a call that read too early gives wrong bits, never an access out of range.

The expected value is always the same call made serially -- default stream, everything synchronised -- on a SEPARATE scene
object made from the same arrays (for the denoisers: the numpy restatement, as in their own tests); the rest of the suite pins
that serial path to the oracle.  Every comparison is equality of bits.

Each test asserts `not busy.query()` directly before the library call: the event recorded behind the delay work has not
completed, so the stream was still busy and everything queued behind it had not started.  The side stream is one that the null
stream was SEEN to overtake (_busy_side_stream): streams share a few hardware queues, and a side stream in the null stream's
queue would hide exactly the mistake these tests look for.  test_negative_control_* shows that the harness sees a wrong-stream
read: the same late inputs, the library on the null stream, and the result is the decoy's.
profiles/concurrency_contract.md has the stream table these tests hold the code to."""
import contextlib
import ctypes
import dataclasses

import numpy as np
import pytest

import denoise_expected as de
import denoise_dual_expected as dd
import raygen
from test_scene_update_host import deform

pytestmark = pytest.mark.gpu

F32 = np.float32
FLT_MAX = F32(3.4028234663852886e38)
W, H, SPP = 64, 48, 4   # frames
N_RAYS = 20_000         # ray batches
EVENTS = ("camera_rays", "shade_events", "any_rays", "emission_adds", "shadow_adds", "rr_draws")
# Delay work in front of the late inputs: DELAY_MATMULS 4096^2 fp32 products (137 GFLOP each: about 1 ms apiece at the fp32
# matrix peak of an MI355X, so some 50 ms and more) against a few hundred microseconds of host time between the event and the
# assert: room to spare by two orders of magnitude.
DELAY_MATMULS = 64


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
def delay(torch):
    """The delay work: a chain of 4096^2 matmuls on the current stream (test_gpu_render_rays.py's idiom), warmed up once so
    that no test pays for the BLAS library's start inside its busy window."""
    g = torch.Generator(device="cuda").manual_seed(1)
    a = torch.randn(4096, 4096, device="cuda", generator=g) / 64.0  # (products keep their scale: no overflow, no denormals)
    b = torch.randn(4096, 4096, device="cuda", generator=g)
    c = torch.empty_like(b)

    def run():
        for _ in range(DELAY_MATMULS // 2):
            torch.mm(a, b, out=c)
            torch.mm(a, c, out=b)
    torch.mm(a, b, out=c)
    torch.cuda.synchronize()
    return run


SIDE_STREAM_TRIES = 8


def _busy_side_stream(torch, delay):
    """Steps 1 and 2: (a non-blocking side stream with the delay work queued on it, the event `busy` behind that work) -- and the
    stream is one that the NULL stream is seen not to queue behind.  The runtime maps its streams onto a few hardware queues (four
    by default), so one side stream in four shares the null stream's queue, and there a launch that the library put on the null
    stream by mistake would run in order behind the late inputs after all: invisible.  So a one-word fill goes to the null stream
    and is waited for; if `busy` is still pending then, the two streams run side by side and the delay is still in front of
    everything the caller queues next.  Otherwise the next stream of PyTorch's pool is tried (each try costs one delay)."""
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    for attempt in range(SIDE_STREAM_TRIES):
        torch.cuda.synchronize()
        s, busy, probe = torch.cuda.Stream(), torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(s):
            delay()
            busy.record(s)
        word.fill_(attempt)  # (the current stream here is the null stream)
        probe.record(torch.cuda.default_stream())
        probe.synchronize()
        if not busy.query():
            print(f"side stream: try {attempt + 1} runs beside the null stream")
            return s, busy
    torch.cuda.synchronize()
    pytest.fail(f"none of {SIDE_STREAM_TRIES} side streams runs beside the null stream: the late-input tests would prove nothing")


@contextlib.contextmanager
def late_inputs(torch, delay, copies=(), zero=(), poison=()):
    """Steps 1 to 4 of every test, on one non-blocking side stream (_busy_side_stream) and without a host synchronisation of that
    stream in between: the delay work, the event `busy` behind it, `copies` (buffer, staging) that replace the decoy in `buffer`
    by the real input, `zero` (buffers the call adds to) and `poison` ((buffer, value): buffers the call overwrites).  Yields
    (stream, busy) with the stream current, for the test to assert `not busy.query()` and make its call; synchronises the device
    on the way out."""
    s, busy = _busy_side_stream(torch, delay)
    try:
        with torch.cuda.stream(s):
            for buffer, staging in copies:
                buffer.copy_(staging)
            for buffer in zero:
                buffer.zero_()
            for buffer, value in poison:
                buffer.fill_(value)
            yield s, busy
    finally:
        torch.cuda.synchronize()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(torch, got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.is_floating_point():
        got, want = got.view(torch.int32), want.view(torch.int32)
    assert torch.equal(got, want), (what, int((got != want).sum().item()), "values differ")


def _assert_differs(a, b, what):
    assert a.shape == b.shape and a.tobytes() != b.tobytes(), what + ": the decoy must give another answer"


# ---- the scenes and the serial answers (one per module; never modified)
@pytest.fixture(scope="module")
def serial_scene(api, bunny_full_bsdf):
    """The scene the serial answers are asked of: no test makes a late call on it."""
    return api.Scene(bunny_full_bsdf)


def _far_rays(n, factor, seed):
    """n rays from `factor` scene sizes out, aimed at the scene (as tests/test_gpu_scene_update.py builds them): origins beyond
    the radius the node records are padded for, so the call's device prepass has to report them and the records are re-padded."""
    rng = np.random.default_rng(seed)
    target = rng.uniform(0.1, 0.9, (n, 3)) * np.array([1.0, 1.0, -1.0])
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    o = (target - dirs * factor).astype(np.float32)
    d = target - o.astype(np.float64)
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def rays(api, torch, serial_scene):
    """(real, decoy): each (origins, dirs, tmax, excluded) on the device, N_RAYS rays.  Real: camera rays of the default view
    (raygen.camera_rays) and, for the last fifth, rays from 1e3 and 1e4 scene sizes out; tmax just beyond each ray's own first
    hit and `excluded` that hit's triangle for every other ray, its neighbour for the rest -- so occlusion depends on both.
    Decoy: camera rays of another view, a short tmax, nothing excluded."""
    n_far = N_RAYS // 10
    o, d = raygen.camera_rays(api.make_camera(aspect=W / H), W, H, N_RAYS - 2 * n_far, seed=21)
    parts = [(o, d), _far_rays(n_far, 1e3, 22), _far_rays(n_far, 1e4, 23)]
    o, d = (np.concatenate([p[k] for p in parts]) for k in (0, 1))
    do, dd_ = raygen.camera_rays(api.make_camera(lookfrom=(0.2, 0.8, 1.2), aspect=W / H), W, H, N_RAYS, seed=24)
    o, d, do, dd_ = (_dev(torch, x) for x in (o, d, do, dd_))
    hit, t, _, _ = serial_scene.query_closest(o, d)
    torch.cuda.synchronize()
    hit, t = hit.cpu().numpy(), t.cpu().numpy()
    assert 0.5 < (hit >= 0).mean()
    tmax = np.where(hit >= 0, t * F32(1.001), FLT_MAX).astype(np.float32)
    n_tris = serial_scene.n_tris()
    excluded = np.where(hit >= 0, np.where(np.arange(N_RAYS) % 2 == 0, hit, (hit + 1) % n_tris), -1).astype(np.int32)
    real = (o, d, _dev(torch, tmax), _dev(torch, excluded))
    decoy = (do, dd_, torch.full((N_RAYS,), 0.25, dtype=torch.float32, device="cuda"),
             torch.full((N_RAYS,), -1, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    return real, decoy


def _decoy_buffers(torch, decoy):
    bufs = tuple(x.clone() for x in decoy)
    torch.cuda.synchronize()
    return bufs


def _closest_poisoned(torch):
    return (torch.empty(N_RAYS, dtype=torch.int32, device="cuda"),) + tuple(torch.empty(N_RAYS, dtype=torch.float32, device="cuda") for _ in range(3))


def _query_closest_serial(torch, sc, o, d, tmax, flags):
    out = tuple(x.clone() for x in sc.query_closest(o, d, tmax, flags=flags))
    torch.cuda.synchronize()
    return out


# ---- queries
@pytest.mark.parametrize("watertight", [False, True], ids=["flags0", "watertight"])
def test_query_closest_with_late_rays(api, torch, delay, bunny_full_bsdf, serial_scene, rays, watertight):
    flags = api.FLAG_WATERTIGHT if watertight else 0
    (o, d, tmax, _), decoy = rays
    want = _query_closest_serial(torch, serial_scene, o, d, tmax, flags)
    want_decoy = _query_closest_serial(torch, serial_scene, *decoy[:3], flags)
    _assert_differs(want[0].cpu().numpy(), want_decoy[0].cpu().numpy(), "query_closest")
    sc = api.Scene(bunny_full_bsdf)  # (untouched: the call below also re-pads its records for the far origins)
    bo, bd, bt, _ = _decoy_buffers(torch, decoy)
    hit, t, u, v = _closest_poisoned(torch)
    with late_inputs(torch, delay, copies=((bo, o), (bd, d), (bt, tmax)),
                     poison=((hit, -7), (t, float("nan")), (u, float("nan")), (v, float("nan")))) as (s, busy):
        assert not busy.query()
        sc.query_closest_device(bo.data_ptr(), bd.data_ptr(), bt.data_ptr(), N_RAYS, hit.data_ptr(), t.data_ptr(), u.data_ptr(), v.data_ptr(),
                                flags=flags, stream=s.cuda_stream)
    for g, w_, name in zip((hit, t, u, v), want, "hit t u v".split()):
        _same(torch, g, w_, ("query_closest", flags, name))
    sc.close()


def test_query_closest_refuses_late_bad_directions(api, torch, delay, bunny_full_bsdf, rays):
    """The table's device check is ordered on the stream as well.  (The other thing the prepass reports, the origin radius, cannot
    be seen from outside: the padding of the records never changes an answer.)  The late table has three directions with a
    component of exactly 2^126 -- finite, and what the header refuses; the decoy in the buffers is a good table.  The call must
    see the late table: refuse, name the three, and write nothing."""
    (o, d, _, _), decoy = rays
    bad = d.clone()
    for row, axis, sign in ((0, 0, 1.0), (N_RAYS // 2, 1, -1.0), (N_RAYS - 1, 2, 1.0)):
        bad[row, axis] = sign * 2.0 ** 126
    sc = api.Scene(bunny_full_bsdf)
    bo, bd, _, _ = _decoy_buffers(torch, decoy)
    hit, t, u, v = _closest_poisoned(torch)
    with late_inputs(torch, delay, copies=((bo, o), (bd, bad)),
                     poison=((hit, -7), (t, float("nan")), (u, float("nan")), (v, float("nan")))) as (s, busy):
        assert not busy.query()
        with pytest.raises(api.RtError, match=f"rt_query_closest_device: 3 of {N_RAYS} directions are not finite or reach 2\\^126"):
            sc.query_closest_device(bo.data_ptr(), bd.data_ptr(), 0, N_RAYS, hit.data_ptr(), t.data_ptr(), u.data_ptr(), v.data_ptr(),
                                    stream=s.cuda_stream)
    assert torch.equal(bd, bad)  # (the late table did arrive)
    assert bool((hit == -7).all()) and all(bool(x.isnan().all()) for x in (t, u, v))
    sc.close()


@pytest.mark.parametrize("watertight", [False, True], ids=["flags0", "watertight"])
def test_query_any_with_late_rays_and_late_excluded(api, torch, delay, bunny_full_bsdf, serial_scene, rays, watertight):
    """The first any-query of the scene: k_query_inverse (the inverse leaf order `excluded` is looked up in) runs in the same call."""
    flags = api.FLAG_WATERTIGHT if watertight else 0
    real, decoy = rays
    want = serial_scene.query_any(*real, flags=flags).clone()
    for other in (decoy, real[:3] + (decoy[3],), decoy[:3] + (real[3],)):  # (each late input matters on its own)
        _assert_differs(want.cpu().numpy(), serial_scene.query_any(*other, flags=flags).cpu().numpy(), "query_any")
    assert 0.1 < want.float().mean().item() < 0.9
    sc = api.Scene(bunny_full_bsdf)
    bufs = _decoy_buffers(torch, decoy)
    occ = torch.empty(N_RAYS, dtype=torch.int32, device="cuda")
    with late_inputs(torch, delay, copies=tuple(zip(bufs, real)), poison=((occ, -7),)) as (s, busy):
        assert not busy.query()
        sc.query_any_device(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), N_RAYS, occ.data_ptr(),
                            flags=flags, stream=s.cuda_stream)
    _same(torch, occ, want, ("query_any", flags))
    sc.close()


# ---- the table form of the AOV call
def test_render_aov_rays_with_late_rays_and_a_late_zero(api, torch, delay, bunny_full_bsdf, serial_scene, rays):
    (o, d, _, _), decoy = rays
    n_pixels, rpp = W * H, 7  # (20 000 rays, seven to a pixel: the last pixels get none and keep the ids' poison)
    want, want_ids, _ = serial_scene.render_aov_rays(o, d, n_pixels, rays_per_pixel=rpp, ids=torch.full((n_pixels, 2), -7, dtype=torch.int32, device="cuda"))
    other, _, _ = serial_scene.render_aov_rays(decoy[0], decoy[1], n_pixels, rays_per_pixel=rpp)
    torch.cuda.synchronize()
    _assert_differs(want.cpu().numpy(), other.cpu().numpy(), "render_aov_rays")
    sc = api.Scene(bunny_full_bsdf)
    bo, bd, _, _ = _decoy_buffers(torch, decoy)
    sums = torch.full((n_pixels, api.AOV_CHANNELS), 123, dtype=torch.int64, device="cuda")
    ids = torch.zeros((n_pixels, 2), dtype=torch.int32, device="cuda")
    with late_inputs(torch, delay, copies=((bo, o), (bd, d)), zero=(sums,), poison=((ids, -7),)) as (s, busy):
        assert not busy.query()
        sc.render_aov_rays(bo, bd, n_pixels, rays_per_pixel=rpp, ids=ids, out=sums, stream=s)
    _same(torch, sums, want, "render_aov_rays sums")
    _same(torch, ids, want_ids, "render_aov_rays ids")
    sc.close()


# ---- camera frames: the sum buffer is zeroed late
@pytest.mark.parametrize("per_sample", [True, False], ids=["rng-per-sample", "default-mode"])
def test_render_shard_fixed_with_a_late_zero(api, torch, delay, bunny_full_bsdf, serial_scene, per_sample):
    flags = api.FLAG_RNG_PER_SAMPLE if per_sample else 0
    cam = api.make_camera(aspect=W / H)
    want = torch.zeros((W * H, 3), dtype=torch.int64, device="cuda")
    st_want = serial_scene.render_shard_fixed(cam, W, H, SPP, 0, 1, want.data_ptr(), flags=flags)
    torch.cuda.synchronize()
    assert (want != 0).any()
    sc = api.Scene(bunny_full_bsdf)
    sums = torch.full((W * H, 3), 123, dtype=torch.int64, device="cuda")
    with late_inputs(torch, delay, zero=(sums,)) as (s, busy):
        assert not busy.query()
        st = sc.render_shard_fixed(cam, W, H, SPP, 0, 1, sums.data_ptr(), flags=flags, stream=s.cuda_stream)
    _same(torch, sums, want, ("render_shard_fixed", flags))
    assert {k: st[k] for k in EVENTS} == {k: st_want[k] for k in EVENTS}
    sc.close()


# ---- the denoisers: 97 x 19, four passes; the expected value is the numpy restatement's image
DN_W, DN_H = 97, 19
DN_PRM = dict(passes=4, sigma_depth=0.3, normal_power_log2=3)


@pytest.fixture(scope="module")
def denoise_case(torch):
    """(real frame, decoy frame, the restatement's images of both): the decoy is another valid synthetic frame."""
    real, decoy = de.synthetic_frame(DN_W, DN_H), de.synthetic_frame(DN_W, DN_H, seed=11)
    prm = dict(DN_PRM, sigma_color=F32(0.7), sigma_depth=F32(0.3))
    want, want_decoy = de.denoise(*real, DN_W, DN_H, **prm), de.denoise(*decoy, DN_W, DN_H, **prm)
    assert de.bits(want).tobytes() != de.bits(want_decoy).tobytes()
    return real, decoy, want, want_decoy


def _denoise_buffers(api, torch, decoy, scratch_bytes):
    """Input buffers that hold the decoy, and scratch and output as an earlier call might have left them."""
    beauty, aov = _dev(torch, decoy[0]), _dev(torch, decoy[2])
    scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
    out = torch.zeros((DN_W * DN_H, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return beauty, aov, scratch, out


def test_denoise_with_late_sums_and_late_poison(api, torch, delay, denoise_case):
    real, decoy, want, _ = denoise_case
    beauty, aov, scratch, out = _denoise_buffers(api, torch, decoy, api.denoise_scratch_bytes(DN_W, DN_H))
    with late_inputs(torch, delay, copies=((beauty, _dev(torch, real[0])), (aov, _dev(torch, real[2]))),
                     poison=((scratch, 0xFF), (out, float("nan")))) as (s, busy):
        assert not busy.query()
        api.denoise(beauty, real[1], aov, real[3], DN_W, DN_H, sigma_color=0.7, scratch=scratch, out=out, stream=s, **DN_PRM)
    assert de.bits(out.cpu().numpy()).tobytes() == de.bits(want).tobytes()


def test_denoise_dual_with_late_halves_and_late_poison(api, torch, delay):
    real = dd.split_frame(de.synthetic_frame(DN_W, DN_H), 2, 2)
    decoy = dd.split_frame(de.synthetic_frame(DN_W, DN_H, seed=11), 2, 2)
    prm = dict(DN_PRM, sigma_variance=F32(1.5), sigma_depth=F32(0.3))
    want = dd.denoise_dual(*real, DN_W, DN_H, **prm)
    for other in (decoy, real[:2] + decoy[2:], decoy[:2] + real[2:4] + decoy[4:], decoy[:4] + real[4:]):  # (each late input matters)
        assert dd.bits(dd.denoise_dual(*other, DN_W, DN_H, **prm)).tobytes() != dd.bits(want).tobytes()
    a, b, aov = _dev(torch, decoy[0]), _dev(torch, decoy[2]), _dev(torch, decoy[4])
    scratch = torch.zeros(api.denoise_dual_scratch_bytes(DN_W, DN_H), dtype=torch.uint8, device="cuda")
    out = torch.zeros((DN_W * DN_H, 3), dtype=torch.float32, device="cuda")
    with late_inputs(torch, delay, copies=((a, _dev(torch, real[0])), (b, _dev(torch, real[2])), (aov, _dev(torch, real[4]))),
                     poison=((scratch, 0xFF), (out, float("nan")))) as (s, busy):
        assert not busy.query()
        api.denoise_dual(a, real[1], b, real[3], aov, real[5], DN_W, DN_H, sigma_variance=1.5, scratch=scratch, out=out, stream=s, **DN_PRM)
    assert dd.bits(out.cpu().numpy()).tobytes() == dd.bits(want).tobytes()


def test_negative_control_the_null_stream_reads_the_decoy(api, torch, delay, denoise_case):
    """The harness of test_denoise_with_late_sums_and_late_poison with ONE change: the library is given the null stream while
    the real sums arrive late on the side stream.  A non-blocking stream and the null stream do not wait for each other, so the
    call reads the decoy -- valid sums of another synthetic frame, the only thing the buffers have held so far -- and returns
    while the side stream is still busy: the image must differ from the restatement's image of the real sums, and it is the
    restatement's image of the decoy.  This is what a launch on the wrong stream inside the library looks like to the tests above.
    (Scratch and output are prepared before the delay, not poisoned late: the poison would land on the result.)"""
    real, decoy, want, want_decoy = denoise_case
    beauty, aov, scratch, out = _denoise_buffers(api, torch, decoy, api.denoise_scratch_bytes(DN_W, DN_H))
    scratch.fill_(0xFF)
    out.fill_(float("nan"))
    with late_inputs(torch, delay, copies=((beauty, _dev(torch, real[0])), (aov, _dev(torch, real[2])))) as (s, busy):
        assert not busy.query()
        api.denoise(beauty, real[1], aov, real[3], DN_W, DN_H, sigma_color=0.7, scratch=scratch, out=out,
                    stream=torch.cuda.default_stream(), **DN_PRM)
        returned_early = not busy.query()  # (synchronous on ITS stream at return: the side stream is still at its delay work)
        got = out.clone()  # (on the side stream, behind the late copies: `out` itself is what the call left)
    got = de.bits(got.cpu().numpy()).tobytes()
    assert returned_early, "the runtime made the null stream wait for the side stream: the late-input tests of this module prove nothing"
    assert got != de.bits(want).tobytes()
    assert got == de.bits(want_decoy).tobytes()
    assert np.array_equal(beauty.cpu().numpy(), real[0]) and np.array_equal(aov.cpu().numpy(), real[2])  # (the late copies did land)


# ---- the three calls that only launch: not synchronous at return, so the output is consumed on the side stream
def test_aov_resolve_with_late_sums(api, torch, delay):
    n, spp = W * H, 4
    real, decoy = de.synthetic_frame(W, H)[2], de.synthetic_frame(W, H, seed=11)[2]
    want = api.aov_resolve(_dev(torch, real), spp).clone()
    _assert_differs(want.cpu().numpy(), api.aov_resolve(_dev(torch, decoy), spp).cpu().numpy(), "aov_resolve")
    sums = _dev(torch, decoy)
    out = torch.zeros((n, api.AOV_CHANNELS), dtype=torch.float32, device="cuda")
    with late_inputs(torch, delay, copies=((sums, _dev(torch, real)),), poison=((out, float("nan")),)) as (s, busy):
        assert not busy.query()
        rc = api.lib().rt_aov_resolve(ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(out.data_ptr()), n, spp, ctypes.c_void_p(s.cuda_stream))
        got = out.clone()
    assert rc == 0
    _same(torch, got, want, "aov_resolve")


def _beauty_sums(seed):
    return de.synthetic_frame(W, H, seed=seed)[0]


def test_post_process_fixed_with_late_sums(api, torch, delay):
    n, spp = W * H, 4
    real, decoy = _beauty_sums(3), _beauty_sums(11)
    want, other = (torch.empty((n, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    api.post_process_fixed(_dev(torch, real).data_ptr(), want.data_ptr(), n, spp)
    api.post_process_fixed(_dev(torch, decoy).data_ptr(), other.data_ptr(), n, spp)
    torch.cuda.synchronize()
    _assert_differs(want.cpu().numpy(), other.cpu().numpy(), "post_process_fixed")
    sums = _dev(torch, decoy)
    out = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    with late_inputs(torch, delay, copies=((sums, _dev(torch, real)),), poison=((out, float("nan")),)) as (s, busy):
        assert not busy.query()
        api.post_process_fixed(sums.data_ptr(), out.data_ptr(), n, spp, stream=s.cuda_stream)
        got = out.clone()
    _same(torch, got, want, "post_process_fixed")


def test_post_process_with_a_late_image(api, torch, delay):
    """In place: the image is both the late input and the output."""
    n, spp = W * H, 4
    real, decoy = ((_beauty_sums(seed).astype(np.float64) * 2.0 ** -30).astype(np.float32) for seed in (3, 11))
    want, other = _dev(torch, real), _dev(torch, decoy)
    api.post_process(want.data_ptr(), n, spp)
    api.post_process(other.data_ptr(), n, spp)
    torch.cuda.synchronize()
    _assert_differs(want.cpu().numpy(), other.cpu().numpy(), "post_process")
    rgb = _dev(torch, decoy)
    with late_inputs(torch, delay, copies=((rgb, _dev(torch, real)),)) as (s, busy):
        assert not busy.query()
        api.post_process(rgb.data_ptr(), n, spp, stream=s.cuda_stream)
        got = rgb.clone()
    _same(torch, got, want, "post_process")


# ---- geometry from device buffers: the vertices (and, where taken, the index arrays) arrive late
@pytest.fixture(scope="module")
def deformed(api, torch, bunny_full_bsdf, rays):
    """(the deformed arrays, what a scene created anew from them answers: closest hits of the real rays, one fixed frame)."""
    arrays = dataclasses.replace(bunny_full_bsdf, tris=deform(bunny_full_bsdf.tris, amp=0.02))
    fresh = api.Scene(arrays)
    answers = _scene_answers(api, torch, fresh, rays)
    undeformed = api.Scene(bunny_full_bsdf)
    old = _scene_answers(api, torch, undeformed, rays)
    undeformed.close()
    _assert_differs(answers[0][0].cpu().numpy(), old[0][0].cpu().numpy(), "the deformed scene's hits")
    _assert_differs(answers[1].cpu().numpy(), old[1].cpu().numpy(), "the deformed scene's frame")
    fresh.close()
    return arrays, answers


def _scene_answers(api, torch, sc, rays):
    (o, d, _, _), _ = rays
    hits = _query_closest_serial(torch, sc, o, d, None, 0)
    sums = torch.zeros((W * H, 3), dtype=torch.int64, device="cuda")
    st = sc.render_shard_fixed(api.make_camera(aspect=W / H), W, H, SPP, 0, 1, sums.data_ptr())
    torch.cuda.synchronize()
    return hits, sums, {k: st[k] for k in EVENTS}


def _assert_answers(api, torch, sc, rays, want, what):
    hits, sums, events = _scene_answers(api, torch, sc, rays)
    for g, w_, name in zip(hits, want[0], "hit t u v".split()):
        _same(torch, g, w_, (what, "query_closest", name))
    _same(torch, sums, want[1], (what, "frame"))
    assert events == want[2], what


def _geometry_buffers(torch, arrays_old, arrays_new):
    """(buffers that hold the decoy, stagings of the real input) for vertices, tri_material and tri_light.  The decoy: the
    undeformed vertices, every triangle on material 0, no triangle a light -- all of it a valid scene."""
    n = arrays_old.tris.shape[0]
    bufs = (_dev(torch, np.asarray(arrays_old.tris, np.float32).reshape(-1, 9)), torch.zeros(n, dtype=torch.int32, device="cuda"),
            torch.full((n,), -1, dtype=torch.int32, device="cuda"))
    real = (_dev(torch, np.asarray(arrays_new.tris, np.float32).reshape(-1, 9)), _dev(torch, np.asarray(arrays_new.tri_material, np.int32)),
            _dev(torch, np.asarray(arrays_new.tri_light, np.int32)))
    torch.cuda.synchronize()
    return bufs, real


@pytest.mark.parametrize("entry", ["update_device", "rebuild_device"])
def test_moved_vertices_arrive_late(api, torch, delay, bunny_full_bsdf, rays, deformed, entry):
    arrays, want = deformed
    (verts, _, _), (real, _, _) = _geometry_buffers(torch, bunny_full_bsdf, arrays)
    sc = api.Scene(bunny_full_bsdf)
    with late_inputs(torch, delay, copies=((verts, real),)) as (s, busy):
        assert not busy.query()
        getattr(sc, entry)(verts.data_ptr(), stream=s.cuda_stream)
    _assert_answers(api, torch, sc, rays, want, entry)
    sc.close()


def test_set_triangles_device_with_late_vertices_and_late_indices(api, torch, delay, bunny_full_bsdf, bunny_matte, rays, deformed):
    arrays, want = deformed
    bufs, real = _geometry_buffers(torch, bunny_full_bsdf, arrays)
    sc = api.Scene(bunny_matte)  # (another material assignment and table: every array of the call changes the answer)
    with late_inputs(torch, delay, copies=tuple(zip(bufs, real))) as (s, busy):
        assert not busy.query()
        sc.set_triangles_tensors(bufs[0], bufs[1], bufs[2], arrays.materials, arrays.lights)  # (the current stream: s)
    _assert_answers(api, torch, sc, rays, want, "set_triangles_device")
    sc.close()


def test_scene_from_tensors_with_late_vertices_and_late_indices(api, torch, delay, bunny_full_bsdf, rays, deformed):
    arrays, want = deformed
    bufs, real = _geometry_buffers(torch, bunny_full_bsdf, arrays)
    with late_inputs(torch, delay, copies=tuple(zip(bufs, real))) as (s, busy):
        assert not busy.query()
        sc = api.Scene.from_tensors(bufs[0], bufs[1], bufs[2], arrays.materials, arrays.lights)  # (the current stream: s)
    _assert_answers(api, torch, sc, rays, want, "Scene.from_tensors")
    sc.close()
