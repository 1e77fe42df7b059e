"""CPU tests of merge_shard_stats (rtcuda_amd/csrc/rt_stats_merge.h): the rt_stats of a frame from the rt_stats of its shards, as
RT_SPLIT merges the sub-shards of one shard and rt_render_multi merges device shards.  The library's own function, through
hc_merge_shard_stats of librt_hostcheck.so, against the table of the header written out here field by field."""
import ctypes
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


@pytest.fixture(scope="module")
def merge(api):
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    L.hc_merge_shard_stats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.hc_merge_shard_stats.restype = None

    def run(shards, sub_shards):
        arr = (api.RtStats * len(shards))(*shards)
        out = api.RtStats()
        L.hc_merge_shard_stats(ctypes.byref(arr), len(shards), int(sub_shards), ctypes.byref(out))
        return out
    return run


COUNTS = ("camera_rays", "shade_events", "closest_rays", "any_rays", "emission_adds", "shadow_adds", "rr_draws")
INT_FIELDS = COUNTS + ("iterations", "bvh_nodes", "bvh_depth", "launches_trace")
SECONDS = ("seconds_render", "seconds_rng_init", "seconds_trace", "seconds_reference_tree", "seconds_advance")


def random_stats(api, rng):
    s = api.RtStats()
    for f in INT_FIELDS:
        setattr(s, f, int(rng.integers(0, 1 << 40)))
    for f in SECONDS:
        setattr(s, f, float(rng.random()) * 10.0)
    for q in range(7):
        s.reserved[q] = int(rng.integers(0, 1 << 40))
    return s


def flat(s):
    return [getattr(s, f) for f in INT_FIELDS + SECONDS] + [int(s.reserved[q]) for q in range(7)]


def expected(shards, sub_shards):
    """The table, one line per field.  The doubles are added in shard order, as the loop adds them."""
    e = {}
    for f in COUNTS + ("launches_trace",):
        e[f] = sum(getattr(s, f) for s in shards)
    for f in ("seconds_render", "seconds_rng_init", "seconds_reference_tree"):
        e[f] = max(getattr(s, f) for s in shards)
    for f in ("seconds_trace", "seconds_advance"):
        if sub_shards:
            tot = getattr(shards[0], f)
            for s in shards[1:]:
                tot = tot + getattr(s, f)
            e[f] = tot
        else:
            e[f] = max(getattr(s, f) for s in shards)
    e["iterations"] = sum(s.iterations for s in shards) if sub_shards else max(s.iterations for s in shards)
    e["bvh_nodes"], e["bvh_depth"] = shards[0].bvh_nodes, shards[0].bvh_depth
    r = [0] * 7
    r[0] = sum(s.reserved[0] for s in shards) if sub_shards else shards[0].reserved[0]
    r[1] = shards[0].reserved[1]
    r[2] = max(s.reserved[2] for s in shards) if sub_shards else shards[0].reserved[2]
    r[3] = shards[0].reserved[3] if sub_shards else len(shards)
    for q in (4, 5, 6):
        r[q] = sum(s.reserved[q] for s in shards)
    return [e[f] for f in INT_FIELDS + SECONDS] + r


@pytest.mark.parametrize("sub_shards", [True, False], ids=["sub_shards", "device_shards"])
@pytest.mark.parametrize("n", [1, 2, 8])
def test_merge_follows_the_table(api, merge, n, sub_shards):
    rng = np.random.default_rng(1000 * n + int(sub_shards))
    for _ in range(20):
        shards = [random_stats(api, rng) for _ in range(n)]
        before = [flat(s) for s in shards]
        got = flat(merge(shards, sub_shards))
        assert got == expected(shards, sub_shards)  # (exact, the doubles too: the same adds in the same order, and max)
        assert [flat(s) for s in shards] == before


def test_one_shard_is_returned_as_it_is(api, merge):
    s = random_stats(api, np.random.default_rng(7))
    assert flat(merge([s], True)) == flat(s)
    want = flat(s)
    want[len(INT_FIELDS + SECONDS) + 3] = 1  # reserved[3]: one device shard behind the totals
    assert flat(merge([s], False)) == want


def test_the_two_modes_differ_where_the_table_says(api, merge):
    """Two shards with known values: what RT_SPLIT adds up and rt_render_multi takes the maximum (or shard 0's) of."""
    a, b = api.RtStats(), api.RtStats()
    a.iterations, b.iterations = 30, 50
    a.seconds_trace, b.seconds_trace = 0.25, 0.5
    a.seconds_advance, b.seconds_advance = 0.125, 0.0625
    a.reserved[0], b.reserved[0] = 1, 1
    a.reserved[2], b.reserved[2] = 100, 700
    a.reserved[3], b.reserved[3] = 0, 0
    split, multi = merge([a, b], True), merge([a, b], False)
    assert (split.iterations, split.seconds_trace, split.seconds_advance) == (80, 0.75, 0.1875)
    assert (multi.iterations, multi.seconds_trace, multi.seconds_advance) == (50, 0.5, 0.125)
    assert (split.reserved[0], split.reserved[2], split.reserved[3]) == (2, 700, 0)
    assert (multi.reserved[0], multi.reserved[2], multi.reserved[3]) == (1, 100, 2)
