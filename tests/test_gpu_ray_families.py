"""Rays through vertices, edges and along the axes (tests/ray_families.py) through rt_query_closest_device / rt_query_any_device.
Run with -m gpu.

The families and the oracle's answers are those of tests/test_ray_families_host.py (computed once per session).  Expected:
  * flags 0 and RT_FLAG_REFERENCE_WALK: the literal oracle;
  * RT_FLAG_WATERTIGHT: EXHAUSTIVE SEARCH over all triangles (ties to the larger caller index) -- not the oracle's walk, which
    shared the product's hole before both were mended;
every bit of hit, t, u, v and occluded, on a host-built tree, a device-built one and the 2-wide experiment format.
"""
import numpy as np
import pytest

import ray_families as rf
from test_ray_families_host import CASES, N, any_answers, answers

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KINDS = ("host-sah", "device-ploc", "pairs")
VARIANTS = ("full_bsdf", "four_bunnies")


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


@pytest.fixture(scope="module")
def gpu_scenes(api):
    """(variant, kind) -> api.Scene, made on first use and closed with the module."""
    made = {}

    def get(variant, kind):
        if (variant, kind) not in made:
            from rtcuda_amd import scenes
            with pytest.MonkeyPatch.context() as mp:
                if kind == "pairs":  # the 2-wide experiment format: read at creation, under the gate the test session sets
                    mp.setenv("RT_BVH_WIDE", "0")
                made[variant, kind] = api.Scene(scenes.cornell_bunny(variant), device_bvh=kind == "device-ploc")
        return made[variant, kind]

    yield get
    for sc in made.values():
        sc.close()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _modes(api):
    return ((0, "literal"), (api.FLAG_REFERENCE_WALK, "literal"), (api.FLAG_WATERTIGHT, "brute"))


def _closest_case(api, oracle, gpu, variant, family):
    a = answers(oracle, variant, family)
    o, d = _dev(a["o"]), _dev(a["d"])
    for flags, which in _modes(api):
        want = a[which]
        hit, t, u, v = (x.cpu().numpy() for x in gpu.query_closest(o, d, flags=flags))
        h = want[0] >= 0
        wrong = {"hit": int((hit != want[0]).sum())}
        for name, got, ref in (("t", t, want[1]), ("u", u, want[2]), ("v", v, want[3])):
            wrong[name] = int((_bits(got[h]) != _bits(ref[h])).sum())
            wrong[name + " on a miss"] = int((_bits(got[~h]) != 0).sum())
        print(variant, family, "flags", flags, "vs", which, wrong, gpu.query_counters() if flags == 0 else "")
        assert wrong == dict.fromkeys(wrong, 0), (family, flags)
        if flags == 0 and family.startswith(("vertex_aimed", "parallel-vertex")) and "x2^" not in family:
            c = gpu.query_counters()
            assert c["tied"] > 0 and c["lost"] > 0, c


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant,family", CASES)
def test_closest_hit_of_every_family(api, oracle, gpu_scenes, variant, family, kind):
    _closest_case(api, oracle, gpu_scenes(variant, kind), variant, family)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("exclude", ["none", "owner"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_any_hit_rays_that_end_on_a_vertex(api, oracle, gpu_scenes, variant, exclude, kind):
    a = any_answers(oracle, variant, exclude)
    gpu = gpu_scenes(variant, kind)
    o, d, tmax, excl = _dev(a["o"]), _dev(a["d"]), _dev(a["tmax"]), _dev(a["excluded"])
    for flags, which in _modes(api):
        occ = gpu.query_any(o, d, tmax, excl, flags=flags).cpu().numpy()
        wrong = int((occ != a[which]).sum())
        print(exclude, kind, "flags", flags, "vs", which, "wrong", wrong)
        assert wrong == 0, (flags, which)


def test_short_directions_are_refused_with_their_count_and_zero_ones_miss(api, oracle, gpu_scenes):
    """A direction with every component below 2^-60 (and not zero) is refused before anything is written; 2^-24 and 2^-59 are
    served (2^-24: test_closest_hit_of_every_family); a zero direction hits nothing."""
    gpu = gpu_scenes("full_bsdf", "host-sah")
    a = answers(oracle, "full_bsdf", "vertex_aimed-fixed")
    o, d = a["o"][:4096], a["d"][:4096].copy()
    rows = np.array([5, 77, 4095])
    d[rows] = rf.scaled(d[rows], 2.0 ** -70)
    assert (np.abs(d[rows]).max(axis=1) > 0).all() and (np.abs(d[rows]).max(axis=1) < 2.0 ** -60).all()
    hit = torch.full((len(o),), -12345, dtype=torch.int32, device="cuda")
    occ = torch.full((len(o),), -12345, dtype=torch.int32, device="cuda")
    o_dev, d_dev = _dev(o), _dev(d)
    with pytest.raises(api.RtError, match=r"rt_query_closest_device: 3 of 4096 directions are shorter than 2\^-60"):
        gpu.query_closest_device(o_dev.data_ptr(), d_dev.data_ptr(), 0, len(o), hit.data_ptr())
    with pytest.raises(api.RtError, match=r"rt_query_any_device: 3 of 4096 directions are shorter than 2\^-60"):
        gpu.query_any_device(o_dev.data_ptr(), d_dev.data_ptr(), 0, 0, len(o), occ.data_ptr())
    sums = torch.full((len(o), 3), -12345, dtype=torch.int64, device="cuda")
    with pytest.raises(api.RtError, match=r"3 of 4096 directions are shorter than 2\^-60"):  # (the tables share the prepass)
        gpu.render_rays(o_dev, d_dev, len(o), fixed=True, out=sums)
    torch.cuda.synchronize()
    assert bool((hit == -12345).all()) and bool((occ == -12345).all()) and bool((sums == -12345).all())
    # the shortest served length gives exhaustive search's triangles (t scales by 2^59: exact), a zero direction misses
    d = rf.scaled(a["d"][:4096], 2.0 ** -59)
    d[rows] = 0
    got = gpu.query_closest(o_dev, _dev(d), flags=api.FLAG_WATERTIGHT)
    want_tri = a["brute"][0][:4096].copy()
    want_t = (a["brute"][1][:4096] * np.float32(2.0 ** 59)).astype(np.float32)
    want_tri[rows], want_t[rows] = -1, 0
    assert np.array_equal(got[0].cpu().numpy(), want_tri)
    assert np.array_equal(_bits(got[1].cpu().numpy()), _bits(want_t))
    assert N >= 4096
