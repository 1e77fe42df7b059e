"""GPU tests of rt_temporal_accumulate_moments_fixed and of the single-buffer loop it closes with rt_denoise_variance_fixed.  Run
with -m gpu.

What the outputs must be comes from tests/temporal_moments_expected.py (the header's text in numpy float32, held to the CPU twin by
tests/test_temporal_moments_host.py).  Every comparison is EQUALITY of all int64 sums, all history lengths and the bits of all
moments and variances; outputs are poisoned before every call, so a pixel that is not written is seen."""
import ctypes

import numpy as np
import pytest

import temporal_expected as te
import temporal_moments_expected as tm

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON = -7
NAMES = ("hist_a", "hist_b", "len", "moments", "variance")


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
    return {k: (int(v) if k in ("max_history", "variance_min_history") else float(v)) for k, v in prm.items()}


def _poisoned(torch, n, two=True, moments=True):
    i64 = lambda: torch.full((n, 3), POISON, dtype=torch.int64, device="cuda")  # noqa: E731
    return (i64(), i64() if two else None, torch.full((n,), POISON, dtype=torch.int32, device="cuda"),
            torch.full((n, 4), POISON, dtype=torch.float32, device="cuda") if moments else None,
            torch.full((n,), POISON, dtype=torch.float32, device="cuda") if moments else None)


def _dev_history(torch, hist):
    return None if hist is None else tuple(x if isinstance(x, int) else _dev(torch, x) for x in hist)


def _run(api, torch, case, w, h, prm, history="given", moments=True, **kw):
    hist = _dev_history(torch, case["history"] if history == "given" else history)
    out = api.temporal_accumulate_moments(_dev(torch, case["sum_a"]), case["spp"][0], _dev(torch, case["sum_b"]), case["spp"][1], _dev(torch, case["aov"]),
                                          case["aov_spp"], _dev(torch, case["motion"]), hist, w, h, moments=moments,
                                          out=_poisoned(torch, w * h, case["sum_b"] is not None, moments), **_prm(prm), **kw)
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _assert_same(got, want, what=""):
    assert len(got) == len(want)
    for name, g, x in zip(NAMES, got, want):
        if x is None:
            assert g is None
            continue
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == x.dtype and g.shape == x.shape, (what, name, g.dtype, g.shape)
        bad = te.bits(g) != te.bits(x)
        print(what, name, "values that differ:", int(bad.sum()), "of", bad.size)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:6].tolist(), g[bad][:6].tolist(), x[bad][:6].tolist())


_param_sets = tm.param_sets


# ---- 1. the CPU file's synthetic cases, at the same sizes
@pytest.mark.parametrize("w,h", tm.SIZES)
@pytest.mark.parametrize("two", [True, False], ids=["two-buffers", "one-buffer"])
def test_synthetic_cases_equal_the_restatement(api, torch, w, h, two):
    case = tm.synthetic_case(w, h, two=two)
    for prm in _param_sets():
        _assert_same(_run(api, torch, case, w, h, prm), tm.run_case(tm.accumulate_moments, case, w, h, prm), (w, h, two, sorted(_prm(prm).items())))
    for alt, moments in tm.history_variants(case["history"]):
        _assert_same(_run(api, torch, case, w, h, tm.PARAMS, history=alt, moments=moments),
                     tm.run_case(tm.accumulate_moments, case, w, h, tm.PARAMS, history=alt, moments=moments), ("history", alt[5] is None, alt[6] is None, moments))
    for vmh in (1, 2):
        prm = dict(tm.PARAMS, variance_min_history=vmh)
        _assert_same(_run(api, torch, case, w, h, prm, history=None), tm.run_case(tm.accumulate_moments, case, w, h, prm, history=None), ("first frame", vmh))


def test_stops_on_either_side_of_equality_and_the_lonely_centre(api, torch):
    for case, prm, lengths in tm.emission_equality_case():
        got = _run(api, torch, case, 4, 1, prm)
        assert got[2].tolist() == lengths
        _assert_same(got, tm.run_case(tm.accumulate_moments, case, 4, 1, prm))
    case, centre = tm.lonely_centre_case()
    prm = dict(tm.PARAMS, variance_min_history=2)
    got = _run(api, torch, case, 5, 5, prm)
    _assert_same(got, tm.run_case(tm.accumulate_moments, case, 5, 5, prm))
    assert got[4][centre] == 0 and (got[4] > 0).sum() >= 20


def test_the_staged_window_at_every_image_edge_and_every_share_of_owing_pixels(api, torch):
    """The spatial estimate is served from a tile and a halo of 2 staged in LDS by the workgroups that owe one.  With every pixel,
    some pixels and no pixel owing one; 1 x 1 and 4 x 1: a tile that is mostly outside the image; 33 x 9 and 97 x 19: tiles whose
    halo crosses the left, right, top and bottom image edge and the edges between tiles; 70 x 30: an interior tile row as well."""
    mh = tm.PARAMS["max_history"]
    for w, h in ((1, 1), (4, 1), (33, 9), (97, 19), (70, 30)):
        case = tm.synthetic_case(w, h, two=False)
        for vmh in (mh + 1, 2, 1):
            prm = dict(tm.PARAMS, variance_min_history=vmh)
            _assert_same(_run(api, torch, case, w, h, prm), tm.run_case(tm.accumulate_moments, case, w, h, prm), (w, h, vmh))
        prm = dict(tm.PARAMS, variance_min_history=2)
        _assert_same(_run(api, torch, case, w, h, prm, history=None), tm.run_case(tm.accumulate_moments, case, w, h, prm, history=None), (w, h, "first"))
    case, centre = tm.lonely_centre_case()
    got = _run(api, torch, case, 5, 5, dict(tm.PARAMS, variance_min_history=2))
    _assert_same(got, tm.run_case(tm.accumulate_moments, case, 5, 5, dict(tm.PARAMS, variance_min_history=2)))
    assert got[4][centre] == 0


def test_defaults_are_the_librarys(api, torch):
    w, h = 97, 19
    case = tm.synthetic_case(w, h)
    d = api.temporal_moments_default_params()
    prm = {k: (v if k in ("max_history", "variance_min_history") else F32(v)) for k, v in d.items()}
    _assert_same(_run(api, torch, case, w, h, {}), tm.run_case(tm.accumulate_moments, case, w, h, prm), "defaults")


# ---- 2. with the new features off it is the old entry point: two GPU calls compared with each other
@pytest.mark.parametrize("two", [True, False], ids=["two-buffers", "one-buffer"])
def test_with_the_new_features_off_it_is_rt_temporal_accumulate_fixed(api, torch, two):
    for w, h in ((33, 9), (97, 19)):
        case = te.synthetic_case(w, h, two=two)
        n = w * h
        dev = {k: _dev(torch, case[k]) for k in ("sum_a", "sum_b", "aov", "motion")}
        hist = _dev_history(torch, case["history"])
        for history in (hist, None):
            old_out = _poisoned(torch, n, two, False)[:3]
            old = api.temporal_accumulate(dev["sum_a"], 2, dev["sum_b"], 2, dev["aov"], 4, dev["motion"], history, w, h, out=old_out, **{k: (int(v) if k == "max_history" else float(v)) for k, v in te.PARAMS.items()})
            new = api.temporal_accumulate_moments(dev["sum_a"], 2, dev["sum_b"], 2, dev["aov"], 4, dev["motion"], None if history is None else history + (None, None),
                                                  w, h, moments=False, out=_poisoned(torch, n, two, False), emission_tolerance=float("inf"),
                                                  variance_min_history=1, **{k: (int(v) if k == "max_history" else float(v)) for k, v in te.PARAMS.items()})
            assert new[3] is None and new[4] is None
            for name, g, x in zip(NAMES, new[:3], old):
                if x is None:
                    assert g is None
                    continue
                assert bool((g == x).all()), (w, h, two, name)
                assert not bool((g == POISON).all())


# ---- 3. the single-buffer loop on the GPU's own frames
def _orbit(api, k, aspect):
    a = np.deg2rad(3.0 * k)
    return api.make_camera((0.5 + 1.5 * np.sin(a), 0.5, 1.5 * np.cos(a)), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 37.8, aspect)


def test_three_frames_through_the_single_buffer_loop(api, torch):
    """render_shard_fixed (ONE call, a new seed per frame) -> render_aov -> render_motion -> temporal_accumulate_moments ->
    denoise_variance(hist_a, 1, variance): every stage equals the restatement run on the same GPU-rendered inputs.  The two sets
    of buffers -- history, length, moments, and the motion and AOV buffers themselves -- are ping-ponged."""
    from rtcuda_amd import scenes
    w, h, spp = 64, 48, 4
    n = w * h
    gpu = api.Scene(scenes.cornell_bunny("full_bsdf"))
    prm = dict(max_history=8, alpha_min=F32(0.125), depth_tolerance=F32(0.1), normal_cos_min=F32(0.9), emission_tolerance=F32(0.0625), variance_min_history=2)
    sets = [_poisoned(torch, n, two=False), _poisoned(torch, n, two=False)]
    hist_t = hist_n = None
    prev_cam = None
    kept, temporal = [], []
    for k in range(3):
        cam = _orbit(api, k, w / h)
        frame = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
        gpu.render_shard_fixed(cam, w, h, spp, 0, 1, frame.data_ptr(), seed=11 + k, flags=api.FLAG_RNG_PER_SAMPLE)
        aov, _, _ = gpu.render_aov(cam, w, h, spp, seed=11 + k, flags=api.FLAG_WATERTIGHT)
        motion, _ = gpu.render_motion(cam, w, h, cam if prev_cam is None else prev_cam, flags=api.FLAG_WATERTIGHT)
        out = api.temporal_accumulate_moments(frame, spp, None, 0, aov, spp, motion, hist_t, w, h, out=sets[k % 2], **_prm(prm))
        assert out[0] is sets[k % 2][0] and out[3] is sets[k % 2][3]
        torch.cuda.synchronize()
        a, v, m = frame.cpu().numpy(), aov.cpu().numpy(), motion.cpu().numpy()
        want = tm.accumulate_moments(a, spp, None, 0, v, spp, m, hist_n, w, h, **prm)
        _assert_same(out, want, ("frame", k))
        kept.append(float(np.mean(want[2] > 1)))
        temporal.append(float(np.mean(want[2] >= 2)))
        clean = api.denoise_variance(out[0], 1, out[4], aov, spp, w, h)
        want_clean = tm.denoise_variance(want[0], 1, want[4], v, spp, w, h)
        assert np.isfinite(want_clean).all()
        assert np.array_equal(te.bits(clean.cpu().numpy()), te.bits(want_clean)), ("denoise_variance on the accumulated frame, frame", k)
        hist_t = (out[0], None, out[2], aov, spp, motion, out[3])
        hist_n = (want[0], None, want[2], v, spp, m, want[3])
        prev_cam = cam
    print("share of pixels that kept history per frame:", kept)
    assert kept[0] == 0.0 and kept[1] > 0.3 and kept[2] > 0.3 and 0.0 < temporal[2] < 1.0  # (both variance estimates are in use)
    assert int(hist_n[2].max()) == 3
    gpu.close()


# ---- 4. buffers, streams, refusals with device buffers
def test_inputs_are_only_read_side_stream_and_repeat(api, torch):
    w, h = 97, 19
    case = tm.synthetic_case(w, h)
    want = tm.run_case(tm.accumulate_moments, case, w, h, tm.PARAMS)
    dev = {k: _dev(torch, case[k]) for k in ("sum_a", "sum_b", "aov", "motion")}
    hist = _dev_history(torch, case["history"])
    out = _poisoned(torch, w * h)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(2):
        got = api.temporal_accumulate_moments(dev["sum_a"], 2, dev["sum_b"], 2, dev["aov"], 4, dev["motion"], hist, w, h, out=out, stream=side, **_prm(tm.PARAMS))
        _assert_same(got, want, "side stream")  # (synchronous on its stream at return)
    for k in dev:
        assert np.array_equal(te.bits(dev[k].cpu().numpy()), te.bits(np.ascontiguousarray(case[k])))
    for t, x in zip(hist, case["history"]):
        if not isinstance(x, int):
            assert np.array_equal(te.bits(t.cpu().numpy()), te.bits(np.ascontiguousarray(x)))


def test_bad_arguments_with_device_buffers_write_nothing(api, torch):
    w, h = 5, 5
    n = w * h
    case = tm.synthetic_case(w, h)
    a, b, v, m = (_dev(torch, case[k]) for k in ("sum_a", "sum_b", "aov", "motion"))
    hist = _dev_history(torch, case["history"])
    out = _poisoned(torch, n)
    shifted = torch.full((4 * n + 4,), POISON, dtype=torch.float32, device="cuda")
    L, c = api.lib(), ctypes.c_void_p
    good = dict(max_history=4, alpha_min=0.5, depth_tolerance=0.1, normal_cos_min=0.5, emission_tolerance=0.25, variance_min_history=2, flags=0)
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def call(history=True, moments_in=P(hist[6]), o_m=P(out[3]), o_v=P(out[4]), **over):
        p = api.RtTemporalMomentsParams(**dict(good, **over))
        hp = [P(hist[0]), P(hist[1]), P(hist[2]), P(hist[3]), P(hist[5])] if history else [None] * 5
        rc = L.rt_temporal_accumulate_moments_fixed(c(P(a)), 2, c(P(b)), 2, c(P(v)), 4, c(P(m)), c(hp[0]), c(hp[1]), c(hp[2]), c(hp[3]), 3, c(hp[4]),
                                                    c(moments_in), w, h, ctypes.byref(p), c(P(out[0])), c(P(out[1])), c(P(out[2])), c(o_m), c(o_v), None)
        return rc, L.rt_last_error().decode()

    for kw, text in ((dict(o_m=shifted.data_ptr() + 4), "d_moments_out must be 16-byte aligned"), (dict(moments_in=shifted.data_ptr() + 4), "d_moments_in must be 16-byte aligned"),
                     (dict(history=False), "d_moments_in and d_prev_motion may be set only when history is given"),
                     (dict(emission_tolerance=float("nan")), "emission_tolerance must be at least 0"), (dict(variance_min_history=0), "variance_min_history must be at least 1"),
                     (dict(o_v=P(hist[2])), "d_variance_out overlaps d_len_in"), (dict(o_v=P(v) + 16), "d_variance_out overlaps d_aov_fixed")):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("rt_temporal_accumulate_moments_fixed: ") and text in msg, (kw, msg)
    with pytest.raises(api.RtError, match="rt_temporal_accumulate_moments_fixed: d_moments_out overlaps d_moments_in"):
        api.temporal_accumulate_moments(a, 2, b, 2, v, 4, m, hist, w, h, out=out[:3] + (hist[6], out[4]), **_prm(tm.PARAMS))
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == POISON).all() for t in out) and bool((shifted == POISON).all())
    for t, x in zip((a, b, v) + hist[:4], (case["sum_a"], case["sum_b"], case["aov"]) + case["history"][:4]):
        assert np.array_equal(t.cpu().numpy(), x)
    rc, msg = call()  # the same call with nothing wrong writes every output
    assert rc == 0, msg
    assert not any((t.cpu().numpy() == POISON).all() for t in out)
