"""Far-off and duplicated geometry on the GPU (tests/placed_scenes.py) against the CPU oracle.  Run with -m gpu.

A scene at 1e4 sends about one ray in 500 down the default kernels' rare path -- the VERIFY finalisation of k_paths, k_trace and
k_query, reference_walk on its LDS column and overflow stack, the retraced / lost / tied counters -- which the scenes in
[0, 1]^3 take once in 10^7 rays; it also gives ensure_origin_radius and the 2^-23 R padding an R four orders of magnitude
from theirs.  Scenes of equal boxes (points(n), copies(n), the bunny at 1e5) were refused by both builders.  The bar: equal bits
against the oracle, every ray, every fixed-point sum, nothing excluded.  tests/test_placed_scenes_host.py holds the CPU side.
"""
import numpy as np
import pytest

import placed_scenes
from conftest import default_camera, usable_cpus
from test_gpu_query import _check_any, _check_closest, _dev, _flag_modes
from test_gpu_scene_rebuild import _device_tree, _twin

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FLT_MAX = placed_scenes.FLT_MAX
EVENTS = [("shade_events", "sum_mat"), ("any_rays", "sum_ah"), ("emission_adds", "emission_adds"), ("shadow_adds", "ah_adds"),
          ("rr_draws", "rr_draws")]
W = 1 << 20  # slots of a frame (rtcuda_amd.dist.W): shard r of R renders the camera rays of slots [r W / R, (r + 1) W / R)


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


# one oracle scene pair and one set of batches per named case and session: the oracle work is the dominant cost
_cases = {}


def _case(oracle, name, variant="matte"):
    key = (name, variant)
    if key not in _cases:
        arrays, s3, t3 = placed_scenes.scene(name, variant)
        lit, wt = oracle.scene(arrays), oracle.scene(arrays).set_watertight(True)
        o, d = placed_scenes.camera_batch(default_camera(oracle, 16 / 9), s3, t3)
        c = wt.trace_closest(o, d, np.full(len(o), FLT_MAX, np.float32))
        o2, d2 = placed_scenes.bounce_batch(o, d, c[1], c[0] >= 0)
        _cases[key] = dict(arrays=arrays, s3=s3, t3=t3, cpu={False: lit, True: wt}, batches=[("camera", o, d), ("bounce", o2, d2)],
                           any={})
    return _cases[key]


def _any(case, watertight):
    if watertight not in case["any"]:
        _, o, d = case["batches"][0]
        case["any"][watertight] = placed_scenes.any_batch(case["cpu"][watertight], case["arrays"], o, d, seed=22,
                                                          tmax_scale=min(case["s3"]))
    return case["any"][watertight]


def _differ(a, b):
    """Rays on which two closest-hit answers (tri, t, ...) differ: the triangle, or t on a hit."""
    return (a[0] != b[0]) | ((a[0] >= 0) & (a[1].view(np.uint32) != b[1].view(np.uint32)))


def _check_queries(api, case, gpu, flag_modes, expect_retraced=False):
    largest = 0
    for flags, watertight in flag_modes:
        cpu = case["cpu"][watertight]
        for what, o, d in case["batches"]:
            want = _check_closest(gpu, cpu, o, d, flags=flags, what=what)
            counters = gpu.query_counters()
            if flags == api.FLAG_WATERTIGHT:
                assert counters == {"retraced": 0, "lost": 0, "tied": 0}, (what, counters)
            if flags == 0 and expect_retraced:
                other = case["cpu"][True].trace_closest(o, d, np.full(len(o), FLT_MAX, np.float32))
                disagree = int(_differ(want, other).sum())
                assert counters["retraced"] == disagree + counters["tied"], (what, counters, disagree)
                assert counters["retraced"] >= 10, (what, counters)
                largest = max(largest, counters["retraced"])
        o3, d3, tm3, excl = _any(case, watertight)
        _check_any(gpu, cpu, o3, d3, tm3, excl, flags)
    return largest


# ---------------------------------------------------------------------------------------------- 1: queries
@pytest.mark.parametrize("device_bvh", [False, True], ids=["host-sah", "device-ploc"])
@pytest.mark.parametrize("name", placed_scenes.QUERY_PLACES)
def test_queries_on_placed_scenes(api, oracle, name, device_bvh):
    """query_closest / query_any, flags 0, RT_FLAG_REFERENCE_WALK and RT_FLAG_WATERTIGHT, against the matching oracle mode.
    On the shifted scenes the default query's `retraced` is the number of rays on which the literal and the watertight
    oracle disagree, plus the exact ties the kernel reports (none measured on the CPU twin)."""
    case = _case(oracle, name)
    gpu = api.Scene(case["arrays"], device_bvh=device_bvh)
    largest = _check_queries(api, case, gpu, _flag_modes(api), expect_retraced=name.startswith("shift"))
    print(f"{name} {'ploc' if device_bvh else 'sah'}: largest retraced count of a batch {largest}")
    gpu.close()


@pytest.mark.parametrize("env", [{"RT_STACK_CAP": "2"}, {"RT_BVH_WIDE": "0"}], ids=["wide-overflow", "pairs"])
@pytest.mark.parametrize("name", placed_scenes.QUERY_PLACES)
def test_default_queries_with_the_overflow_stack_and_the_two_wide_tree(api, oracle, name, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = _case(oracle, name)
    gpu = api.Scene(case["arrays"])
    largest = _check_queries(api, case, gpu, [(0, False)], expect_retraced=name.startswith("shift"))
    print(f"{name} {env}: largest retraced count of a batch {largest}")
    gpu.close()


# ---------------------------------------------------------------------------------------------- 2: frames
FRAME = (96, 64, 8)  # shift_1e4: the literal and the watertight oracle frames differ at 8 spp already (asserted below), the
#                      smallest of {8, 16, 32}: the frame takes the rare path


def _camera(make, case, aspect):
    return placed_scenes.placed_camera(make, case["s3"], case["t3"], aspect)


_frames = {}


def _oracle_frame(oracle, case, key, watertight, frame, slot_hi=W):
    k = (key, watertight, frame, slot_hi)
    if k not in _frames:
        w, h, spp = frame
        fixed = np.zeros((h, w, 3), np.int64)
        _, _, st = case["cpu"][watertight].render(_camera(oracle.camera, case, w / h), w, h, spp, slot_hi=slot_hi,
                                                  threads=usable_cpus(), fixed_out=fixed)
        _frames[k] = (fixed, {g: st[c] for g, c in EVENTS})
    return _frames[k]


def _gpu_fixed(api, oracle, gpu, case, frame, flags, shards=(0, 1)):
    w, h, spp = frame
    buf = torch.zeros(h * w * 3, dtype=torch.int64, device="cuda")
    st = gpu.render_shard_fixed(_camera(oracle.camera, case, w / h), w, h, spp, shards[0], shards[1], buf.data_ptr(), flags=flags)
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(h, w, 3), {g: st[g] for g, _ in EVENTS}


def _check_frames(api, oracle, gpu, case, key, frame):
    w, h, spp = frame
    for watertight in (False, True):
        flags = api.FLAG_DETERMINISTIC | (api.FLAG_WATERTIGHT if watertight else 0)
        want, ev = _oracle_frame(oracle, case, key, watertight, frame)
        got, ev_g = _gpu_fixed(api, oracle, gpu, case, frame, flags)
        assert ev_g == ev, (watertight, ev_g, ev)
        assert np.array_equal(got, want), (watertight, int((got != want).sum()))
        half, ev_h = _oracle_frame(oracle, case, key, watertight, frame, slot_hi=W // 2)  # shard 0 of 2
        got_h, ev_gh = _gpu_fixed(api, oracle, gpu, case, frame, flags, shards=(0, 2))
        assert ev_gh == ev_h and np.array_equal(got_h, half), watertight
        # rt_render: the same events, and the image post-processed from the same sums
        img, st = gpu.render(_camera(oracle.camera, case, w / h), w, h, spp, flags=flags)
        assert {g: st[g] for g, _ in EVENTS} == ev, watertight
        out = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
        api.post_process_fixed(_dev(want.reshape(-1)).data_ptr(), out.data_ptr(), w * h, spp)
        torch.cuda.synchronize()
        assert img.tobytes() == out.cpu().numpy().tobytes(), watertight


@pytest.mark.parametrize("persistent", [True, False], ids=["k_paths", "k_advance-k_trace"])
@pytest.mark.parametrize("variant", ["matte", "full_bsdf"])
@pytest.mark.parametrize("name", ["shift_1e4", "stretch_x_1e3"])
def test_frames_of_placed_scenes(api, oracle, name, variant, persistent, monkeypatch):
    if not persistent:
        monkeypatch.setenv("RT_PERSISTENT", "0")
    case = _case(oracle, name, variant)
    gpu = api.Scene(case["arrays"])
    _check_frames(api, oracle, gpu, case, (name, variant), FRAME)
    if name == "shift_1e4":  # the frame really takes the rare path: the two oracle modes do not render the same frame
        lit, wt = (_oracle_frame(oracle, case, (name, variant), m, FRAME) for m in (False, True))
        assert lit[1] != wt[1] or not np.array_equal(lit[0], wt[0])
    gpu.close()


# ---------------------------------------------------------------------------------------------- 3: refused scenes now render
SMALL_FRAME = (64, 48, 4)


@pytest.mark.parametrize("device_bvh", [False, True], ids=["host-sah", "device-ploc"])
@pytest.mark.parametrize("name", ["points_200", "copies_1000", "shift_1e5"])
def test_scenes_of_equal_boxes_are_built_traced_and_rendered(api, oracle, name, device_bvh):
    case = _case(oracle, name)
    arrays = case["arrays"]
    if name != "shift_1e5" and len(case["batches"]) == 2:  # (rays that cross the run of equal boxes: ties by the thousand)
        case["batches"].append(("aimed",) + placed_scenes.aimed_batch(arrays.tris[:int(name.split("_")[1])]))
    gpu = api.Scene(arrays, library=api.tools_lib(), device_bvh=device_bvh)
    recs, order, info = _twin(arrays.tris)
    print(f"{name}: PLOC twin {int(info[1])} iterations, 4-wide depth {int(info[2])}")
    if device_bvh:
        r, o = _device_tree(api, gpu)
        assert np.array_equal(o, order) and r.shape == recs.shape and np.array_equal(r, recs)
    _check_queries(api, case, gpu, _flag_modes(api))
    _check_frames(api, oracle, gpu, case, (name, "matte"), SMALL_FRAME)
    if not device_bvh:  # rebuild(): the device builder's tree, the same bits
        gpu.rebuild()
        assert gpu.info()["builder"] == "ploc"
        r, o = _device_tree(api, gpu)
        assert np.array_equal(o, order) and np.array_equal(r, recs)
        _check_queries(api, case, gpu, _flag_modes(api))
        _check_frames(api, oracle, gpu, case, (name, "matte"), SMALL_FRAME)
    gpu.close()


# ---------------------------------------------------------------------------------------------- 4: refit
def test_refit_from_the_unit_box_to_1e4(api, oracle, bunny_matte):
    """rt_scene_update_device with the shift_1e4 vertices: a refit whose origin radius grows from 1 to 1e4."""
    case = _case(oracle, "shift_1e4")
    gpu = api.Scene(bunny_matte)
    import raygen
    o, d = raygen.camera_rays(default_camera(oracle, 16 / 9), 1920, 1080, 1000, seed=3)
    gpu.query_closest(_dev(o), _dev(d))  # (a query at the old place first: the records padded for radius 1)
    verts = _dev(case["arrays"].tris)
    gpu.update_device(verts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    largest = _check_queries(api, case, gpu, [(0, False), (api.FLAG_WATERTIGHT, True)], expect_retraced=True)
    print(f"refit to shift_1e4: largest retraced count of a batch {largest}")
    gpu.close()
