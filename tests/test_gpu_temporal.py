"""GPU tests of the temporal accumulator (rt_temporal_accumulate_fixed) and of the whole composition it closes.  Run with -m gpu.

What the outputs must be comes from tests/temporal_expected.py (the header's text in numpy float32, held to the CPU twin by
tests/test_temporal_host.py).  Every comparison is EQUALITY of all int64 sums and all history lengths."""
import ctypes

import numpy as np
import pytest

import aov_expected as ae
import denoise_dual_expected as dd
import temporal_expected as te

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON = -7


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()  # raises if the HIP library is missing: there is no fallback
    return _api


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    return _torch


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _prm(prm):
    return {k: (int(v) if k == "max_history" else float(v)) for k, v in prm.items()}


def _poisoned(torch, n, two=True):
    return (torch.full((n, 3), POISON, dtype=torch.int64, device="cuda"), torch.full((n, 3), POISON, dtype=torch.int64, device="cuda") if two else None,
            torch.full((n,), POISON, dtype=torch.int32, device="cuda"))


def _run(api, torch, case, w, h, prm, history="given", **kw):
    hist = case["history"] if history == "given" else history
    if hist is not None:
        hist = (_dev(torch, hist[0]), _dev(torch, hist[1]), _dev(torch, hist[2]), _dev(torch, hist[3]), hist[4])
    out = api.temporal_accumulate(_dev(torch, case["sum_a"]), case["spp"][0], _dev(torch, case["sum_b"]), case["spp"][1], _dev(torch, case["aov"]),
                                  case["aov_spp"], _dev(torch, case["motion"]), hist, w, h, out=_poisoned(torch, w * h, case["sum_b"] is not None),
                                  **_prm(prm), **kw)
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _assert_same(got, want, what=""):
    for name, g, x in zip(("hist_a", "hist_b", "len"), got, want):
        if x is None:
            assert g is None
            continue
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        bad = g != x
        print(what, name, "values that differ:", int(bad.sum()), "of", bad.size)
        assert g.dtype == x.dtype and not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:6].tolist(), g[bad][:6].tolist(), x[bad][:6].tolist())


# ---- 1. the CPU file's synthetic cases, at the same sizes
@pytest.mark.parametrize("w,h", te.SIZES)
@pytest.mark.parametrize("two", [True, False], ids=["two-buffers", "one-buffer"])
def test_synthetic_cases_equal_the_restatement(api, torch, w, h, two):
    case = te.synthetic_case(w, h, two=two)
    for prm in (te.PARAMS, dict(te.PARAMS, max_history=1), dict(te.PARAMS, alpha_min=F32(1.0)), dict(te.PARAMS, normal_cos_min=F32(-1.0), depth_tolerance=F32(1e30)),
                dict(max_history=0x7fffffff, alpha_min=F32(1e-30), depth_tolerance=F32(0.5), normal_cos_min=F32(1.0))):
        _assert_same(_run(api, torch, case, w, h, prm), te.run_case(te.accumulate, case, w, h, prm), (w, h, two, sorted(_prm(prm).items())))
    _assert_same(_run(api, torch, case, w, h, te.PARAMS, history=None), te.run_case(te.accumulate, case, w, h, te.PARAMS, history=None), "first frame")


@pytest.mark.parametrize("w,h", [(4, 1), (70, 30)])
@pytest.mark.parametrize("two", [True, False], ids=["two-buffers", "one-buffer"])
def test_tiles_mostly_outside_the_image_and_ragged_edges(api, torch, w, h, two):
    """The sizes test_gpu_temporal_moments.py runs for the tiles' sake, on this entry point's instantiation of the same pixel body.
    4 x 1: one 32 x 8 tile of which 4 lanes have a pixel; 70 x 30: three tile columns and four tile rows, so interior tile rows,
    and a ragged right (70 = 2 * 32 + 6) and bottom (30 = 3 * 8 + 6) edge."""
    case = te.synthetic_case(w, h, two=two)
    _assert_same(_run(api, torch, case, w, h, te.PARAMS), te.run_case(te.accumulate, case, w, h, te.PARAMS), (w, h, two, "history"))
    _assert_same(_run(api, torch, case, w, h, te.PARAMS, history=None), te.run_case(te.accumulate, case, w, h, te.PARAMS, history=None), (w, h, two, "first frame"))


def test_stops_on_either_side_of_equality(api, torch):
    case, sets = te.equality_stops()
    for prm, lengths in sets:
        got = _run(api, torch, case, 4, 1, prm)
        assert got[2].tolist() == lengths
        _assert_same(got, te.run_case(te.accumulate, case, 4, 1, prm))


def test_one_buffer_equals_the_two_buffer_a_and_defaults_are_the_librarys(api, torch):
    w, h = 97, 19
    case = te.synthetic_case(w, h)
    d = api.temporal_default_params()
    two = _run(api, torch, case, w, h, {})
    _assert_same(two, te.run_case(te.accumulate, case, w, h, {k: (v if k == "max_history" else F32(v)) for k, v in d.items()}), "defaults")
    one_case = dict(case, sum_b=None, history=(case["history"][0], None) + tuple(case["history"][2:]))
    one = _run(api, torch, one_case, w, h, {})
    assert one[1] is None and np.array_equal(one[0], two[0]) and np.array_equal(one[2], two[2])


# ---- 2. the whole composition on the GPU's own frames
def _orbit(api, k, aspect):
    a = np.deg2rad(3.0 * k)
    return api.make_camera((0.5 + 1.5 * np.sin(a), 0.5, 1.5 * np.cos(a)), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8, aspect)


def test_three_frames_through_the_whole_composition(api, torch):
    """render_shard_fixed halves (a new seed per frame) -> render_aov -> render_motion -> temporal_accumulate -> denoise_dual(a, 1,
    b, 1): hist_* and len equal the restatement run on the same GPU-rendered inputs, the dual denoiser accepts the result and
    equals its own restatement on it.  The two buffer sets are ping-ponged."""
    from rtcuda_amd import scenes
    w, h, spp = 64, 48, 4
    n = w * h
    gpu = api.Scene(scenes.cornell_bunny("full_bsdf"))
    prm = dict(max_history=8, alpha_min=F32(0.125), depth_tolerance=F32(0.1), normal_cos_min=F32(0.9))
    sets = [_poisoned(torch, n), _poisoned(torch, n)]
    hist_t = hist_n = None
    prev_cam = None
    kept = []
    for k in range(3):
        cam = _orbit(api, k, w / h)
        halves = []
        for r in (0, 1):
            t = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
            gpu.render_shard_fixed(cam, w, h, spp, r, 2, t.data_ptr(), seed=11 + k, flags=api.FLAG_RNG_PER_SAMPLE)
            halves.append(t)
        aov, _, _ = gpu.render_aov(cam, w, h, spp, seed=11 + k, flags=api.FLAG_WATERTIGHT)
        motion, _ = gpu.render_motion(cam, w, h, cam if prev_cam is None else prev_cam, flags=api.FLAG_WATERTIGHT)
        out = api.temporal_accumulate(halves[0], spp // 2, halves[1], spp // 2, aov, spp, motion, hist_t, w, h, out=sets[k % 2], **_prm(prm))
        assert out[0] is sets[k % 2][0]
        torch.cuda.synchronize()
        a, b, v, m = halves[0].cpu().numpy(), halves[1].cpu().numpy(), aov.cpu().numpy(), motion.cpu().numpy()
        want = te.accumulate(a, spp // 2, b, spp // 2, v, spp, m, hist_n, w, h, **prm)
        _assert_same(out, want, ("frame", k))
        kept.append(float(np.mean(want[2] > 1)))
        clean = api.denoise_dual(out[0], 1, out[1], 1, aov, spp, w, h)
        want_clean = dd.denoise_dual(want[0], 1, want[1], 1, v, spp, w, h)
        assert np.array_equal(te.bits(clean.cpu().numpy()), te.bits(want_clean)), ("denoise_dual on the accumulated halves, frame", k)
        hist_t = (out[0], out[1], out[2], aov, spp)
        hist_n = (want[0], want[1], want[2], v, spp)
        prev_cam = cam
    print("share of pixels that kept history per frame:", kept)
    assert kept[0] == 0.0 and kept[1] > 0.3 and kept[2] > 0.3  # (most hit pixels find their history under a 3 degree orbit)
    assert int(hist_n[2].max()) == 3
    gpu.close()


# ---- 3. buffers, streams, refusals with device buffers
def test_inputs_are_only_read_side_stream_and_repeat(api, torch):
    w, h = 97, 19
    case = te.synthetic_case(w, h)
    want = te.run_case(te.accumulate, case, w, h, te.PARAMS)
    dev = {k: _dev(torch, case[k]) for k in ("sum_a", "sum_b", "aov", "motion")}
    hist = tuple(_dev(torch, x) for x in case["history"][:4]) + (case["history"][4],)
    out = _poisoned(torch, w * h)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(2):
        got = api.temporal_accumulate(dev["sum_a"], 2, dev["sum_b"], 2, dev["aov"], 4, dev["motion"], hist, w, h, out=out, stream=side, **_prm(te.PARAMS))
        _assert_same(got, want, "side stream")  # (synchronous on its stream at return)
    for k in dev:
        assert np.array_equal(te.bits(dev[k].cpu().numpy()), te.bits(np.ascontiguousarray(case[k])))
    for t, x in zip(hist[:4], case["history"][:4]):
        assert np.array_equal(t.cpu().numpy(), x)


def test_overlaps_and_bad_arguments_with_device_buffers_write_nothing(api, torch):
    w, h = 5, 5
    n = w * h
    case = te.synthetic_case(w, h)
    a, b, v, m = (_dev(torch, case[k]) for k in ("sum_a", "sum_b", "aov", "motion"))
    hist = tuple(_dev(torch, x) for x in case["history"][:4]) + (case["history"][4],)
    out = _poisoned(torch, n)
    f = api.temporal_accumulate
    for bad_out, text in (((hist[0], out[1], out[2]), "d_hist_a_out overlaps d_hist_a_in"), ((out[0], hist[1], out[2]), "d_hist_b_out overlaps d_hist_b_in"),
                          ((out[0], out[1], hist[2]), "d_len_out overlaps d_len_in"), ((a, out[1], out[2]), "d_hist_a_out overlaps d_sum_a"),
                          ((out[0], out[0], out[2]), "d_hist_a_out overlaps d_hist_b_out")):
        with pytest.raises(api.RtError, match="rt_temporal_accumulate_fixed: " + text):
            f(a, 2, b, 2, v, 4, m, hist, w, h, out=bad_out, **_prm(te.PARAMS))
    with pytest.raises(api.RtError, match="rt_temporal_accumulate_fixed: alpha_min must be in"):
        f(a, 2, b, 2, v, 4, m, hist, w, h, out=out, alpha_min=1.5)
    with pytest.raises(api.RtError, match="rt_temporal_accumulate_fixed: normal_cos_min must be in"):
        f(a, 2, b, 2, v, 4, m, hist, w, h, out=out, normal_cos_min=-2)
    L, c = api.lib(), ctypes.c_void_p
    rc = L.rt_temporal_accumulate_fixed(c(a.data_ptr()), 2, c(b.data_ptr()), 2, c(v.data_ptr()), 4, c(m.data_ptr()), c(hist[0].data_ptr()), None,
                                        c(hist[2].data_ptr()), c(hist[3].data_ptr()), 3, w, h, None, c(out[0].data_ptr()), c(out[1].data_ptr()),
                                        c(out[2].data_ptr()), None)
    assert rc != 0 and "d_sum_b and d_hist_b_in must be null together" in L.rt_last_error().decode()
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == POISON).all() for t in out)
    for t, x in zip((a, b, v) + hist[:3], (case["sum_a"], case["sum_b"], case["aov"]) + case["history"][:3]):
        assert np.array_equal(t.cpu().numpy(), x)
