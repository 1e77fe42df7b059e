"""What a counted frame (rt_render_counts_fixed) must hold, from the oracle alone (numpy and Python integers; no library call).

Pixel p renders the samples first[p] .. first[p] + count[p] - 1 of the w x h x S per-sample frame; sample k of pixel p is camera
ray G = p * S + k of that frame.  Two routes to the expected sums:

  frames  the oracle's per-sample frame of shard (k, S) is exactly sample k of every pixel (G % S == k), so the counted frame is
          the sum over k of mask_k(p) * frame_k, mask_k(p) = first[p] <= k < first[p] + count[p];
  tables  one keyed table per pixel run -- raytable_keyed.keyed_pinhole_table's rows for the keys p * S + first[p] ..., through
          OracleScene.render_table(keyed=True, key_first = p * S + first[p]) -- which also gives the six event totals, and
          works where S is too large for a frame (keys beyond 32 bits).

tests/test_render_counts_host.py holds the two routes to each other and to `oracle.render(rng_mode="per_sample")`.
Also the Python-integer restatements of rt_normalize_counts_fixed, rt_post_process_counts_fixed and rt_sample_allocate."""
import numpy as np

from conftest import default_camera, usable_cpus
import raytable_keyed as rk

KEYS = ("camera_rays", "shade_events", "any_rays", "emission_adds", "shadow_adds", "rr_draws")

_frames = {}


def events_of(st):
    """The six event totals under rt_stats' names, from the oracle's stats."""
    return {"camera_rays": st["sum_gen"], "shade_events": st["sum_mat"], "any_rays": st["sum_ah"],
            "emission_adds": st["emission_adds"], "shadow_adds": st["ah_adds"], "rr_draws": st["rr_draws"]}


def _camera(oracle, w, h, cam):
    """The 12 floats of the frame's camera: `cam`, or the default view where it is None."""
    return default_camera(oracle, w / h) if cam is None else np.ascontiguousarray(cam, np.float32)


def sample_frames(oracle, osc, tag, w, h, S, max_bounces=10, seed=1, cam=None):
    """[frame_k for k in range(S)]: (w * h, 3) int64 sums of sample k of every pixel; computed once per argument tuple, read-only."""
    key = (tag, w, h, S, max_bounces, seed, None if cam is None else _camera(oracle, w, h, cam).tobytes())
    if key not in _frames:
        out = []
        for k in range(S):
            f = np.zeros((h, w, 3), np.int64)
            osc.render(_camera(oracle, w, h, cam), w, h, S, max_bounces=max_bounces, seed=seed, threads=usable_cpus(), fixed_out=f,
                       rng_mode="per_sample", shard=(k, S))
            f = f.reshape(-1, 3)
            f.setflags(write=False)
            out.append(f)
        _frames[key] = out
    return _frames[key]


def _maps(w, h, first, count):
    n = w * h
    count = np.asarray(count, np.int64).reshape(n)
    first = np.zeros(n, np.int64) if first is None else np.asarray(first, np.int64).reshape(n)
    return first, count


def expected_by_frames(oracle, osc, tag, w, h, S, first, count, max_bounces=10, seed=1, cam=None):
    """(w * h, 3) int64 sums of the counted frame, by masking the sample frames."""
    first, count = _maps(w, h, first, count)
    assert (count >= 0).all() and (first >= 0).all() and (first + count <= S).all()
    want = np.zeros((w * h, 3), np.int64)
    for k, f in enumerate(sample_frames(oracle, osc, tag, w, h, S, max_bounces, seed, cam)):
        mask = (first <= k) & (k < first + count)
        want += f * mask[:, None]
    return want


def expected_by_tables(oracle, osc, w, h, S, first, count, max_bounces=10, seed=1, cam=None):
    """((w * h, 3) int64 sums, the six event totals) of the counted frame, one keyed table per pixel run.  `cam`: the frame's
    camera (12 floats) where it is not the default view."""
    first, count = _maps(w, h, first, count)
    cam = _camera(oracle, w, h, cam)
    want = np.zeros((w * h, 3), np.int64)
    ev = {k: 0 for k in KEYS}
    for p in np.flatnonzero(count > 0):
        p, f, c = int(p), int(first[p]), int(count[p])
        key_first = p * S + f
        o, d, pixel = rk.keyed_pinhole_table(oracle, cam, w, h, S, seed, range(key_first, key_first + c))
        assert (pixel == p).all()
        sums, st = osc.render_table(o, d, w * h, pixel=pixel, max_bounces=max_bounces, seed=seed, keyed=True, key_first=key_first)
        want += sums
        e = events_of(st)
        for k in KEYS:
            ev[k] += e[k]
    return want, ev


# ---- the Python-integer twins
def normalize_twin(sums, samples):
    """rt_normalize_counts_fixed: sign(s) * ((|s| + (n >> 1)) // n), 0 where n == 0, in Python integers."""
    sums = np.asarray(sums, np.int64)
    out = np.zeros_like(sums)
    for p, n in enumerate(np.asarray(samples).tolist()):
        if n < 0:
            raise ValueError("negative sample count")
        if n == 0:
            continue
        for ch in range(sums.shape[1]):
            s = int(sums[p, ch])
            q = (abs(s) + (n >> 1)) // n
            out[p, ch] = -q if s < 0 else q
    return out


def post_process_twin(sums, samples):
    """rt_post_process_counts_fixed: sqrt(float32(float64(s) * 2^-30) * (float32(1) / float32(n))), 0 where n <= 0."""
    sums = np.asarray(sums, np.int64)
    n = np.asarray(samples, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (np.float32(1.0) / n.astype(np.float32)).astype(np.float32)
        v = (sums.astype(np.float64) * (1.0 / 1073741824.0)).astype(np.float32)
        out = np.sqrt((v * inv[:, None]).astype(np.float32)).astype(np.float32)
    out[n <= 0] = 0
    return out


def quantised_weight(weight):
    """q[p] as Python integers: 0 unless w > 0, else floor(min(w, 4096) * 2^20) with every step in float32."""
    w = np.asarray(weight, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = np.floor(np.minimum(w, np.float32(4096.0)) * np.float32(1048576.0)).astype(np.float32)
    return [int(s) if x > 0 else 0 for x, s in zip(w.tolist(), scaled.tolist())]


def allocate_twin(weight, min_count, max_count, budget):
    """rt_sample_allocate in Python integers -> (counts (n,) int32, total).  ValueError where the library refuses."""
    q = quantised_weight(weight)
    n = len(q)
    extra = budget - n * min_count
    if min_count < 0 or max_count < min_count or extra < 0 or extra >= 1 << 31:
        raise ValueError("refused")
    T = sum(q)
    assert all(0 <= x <= 1 << 32 for x in q) and extra * (1 << 32) < 1 << 63
    counts = [min(max_count, min_count + ((extra * x) // T if T else extra // n)) for x in q]
    return np.array(counts, np.int32), sum(counts)
