"""CPU tests of the keyed ray tables (rt_render_rays_keyed_device / rt_render_rays_keyed_fixed_device): the fixture builder
of the GPU tests is held to the oracle key by key, the seed-shift identity the high-key GPU test rests on, dist.ray_chunk, and
the entry points declared / exported / bound / built.  Everything that renders is in tests/test_gpu_render_rays_keyed.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, default_camera
import raytable_keyed as rk

NEW = ("rt_render_rays_keyed_device", "rt_render_rays_keyed_fixed_device")
HIGH_KEYS = (2 ** 32 - 100, 2 ** 40 + 5)  # the first range crosses 2^32


@pytest.fixture(scope="module")
def api():
    from rtcuda_amd import api as _api
    _api.lib()
    return _api


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _literal_rays(oracle, cam, w, h, spp, seed, keys):
    """Ray by ray through the oracle's own functions: sample_stream, two draws, camera_get_ray."""
    o, d = np.zeros((len(keys), 3), np.float32), np.zeros((len(keys), 3), np.float32)
    for c, K in enumerate(keys):
        _, (jx, jy) = oracle.xorwow_draw(oracle.sample_stream(seed, K), 2)
        p = K // spp
        x = (np.float32(p % w) + jx) / np.float32(w)
        y = (np.float32(p // w) + jy) / np.float32(h)
        r = oracle.camera_get_ray(cam, float(x), float(y))
        o[c], d[c] = r[0:3], r[3:6]
    return o, d


def test_stream_states_are_the_oracles_sample_streams(oracle):
    for seed in (1, 2 ** 32 + 7, 0xFFFFFFFF00000007):
        for first in (0,) + HIGH_KEYS:
            keys = range(first, first + 300)
            st = rk.stream_states(oracle, seed, keys)
            for c, K in enumerate(keys):
                assert st[c].tolist() == oracle.sample_stream(seed, K).tolist(), (seed, K)
    # keys that are not consecutive (a strided rank)
    keys = list(range(3, 3 + 8 * 50, 8))
    st = rk.stream_states(oracle, 1, keys)
    assert all(st[c].tolist() == oracle.sample_stream(1, K).tolist() for c, K in enumerate(keys))


def test_keyed_table_is_the_oracle_functions_ray_by_ray(oracle):
    """keyed_pinhole_table (numpy, float32) against Oracle.sample_stream + xorwow_draw + camera_get_ray: every ray of
    19 x 27 x 3, a strided rank of it, and a few hundred keys around 2^32 and 2^40 in frames those keys fall into."""
    w, h, spp = 19, 27, 3
    cam = default_camera(oracle, w / h)
    for seed, keys in ((1, range(w * h * spp)), (2 ** 32 + 5, range(2, w * h * spp, 4))):
        keys = list(keys)
        o, d, pixel = rk.keyed_pinhole_table(oracle, cam, w, h, spp, seed, keys)
        o_l, d_l = _literal_rays(oracle, cam, w, h, spp, seed, keys)
        assert np.array_equal(_bits(o), _bits(o_l)) and np.array_equal(_bits(d), _bits(d_l))
        assert pixel.dtype == np.int32 and np.array_equal(pixel, np.array(keys) // spp)
    for first in HIGH_KEYS:
        keys = list(range(first, first + 300))
        spp_big = 2 ** 22  # a 1024 x 1024 frame whose pixel 1023 (first case) / 262144 (second) these keys fall into
        w2 = h2 = 1024
        cam2 = default_camera(oracle, 1.0)
        o, d, pixel = rk.keyed_pinhole_table(oracle, cam2, w2, h2, spp_big, 1, keys)
        o_l, d_l = _literal_rays(oracle, cam2, w2, h2, spp_big, 1, keys)
        assert np.array_equal(_bits(o), _bits(o_l)) and np.array_equal(_bits(d), _bits(d_l))
        assert np.array_equal(pixel, np.array([K // spp_big for K in keys]))


def test_seed_shift_identity(oracle):
    """sample_stream(seed, F + c) == sample_stream((seed + 0x9E3779B97F4A7C15 * F) mod 2^64, c): what lets a frame whose keys
    start at F be checked against the oracle's frame (keys from 0) of the shifted seed."""
    for seed in (1, 0xFFFFFFFF00000007):
        for F in HIGH_KEYS:
            s2 = rk.shifted_seed(seed, F)
            assert 0 <= s2 < 2 ** 64 and s2 != seed
            assert np.array_equal(oracle.sample_stream_words(seed, F, 1000), oracle.sample_stream_words(s2, 0, 1000))
            for c in (0, 1, 99, 100, 101, 999):
                assert oracle.sample_stream(seed, F + c).tolist() == oracle.sample_stream(s2, c).tolist(), (seed, F, c)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 7, 8, 1000003])
def test_ray_chunks_are_disjoint_even_and_cover_the_table(world, n):
    from rtcuda_amd import dist
    chunks = [dist.ray_chunk(r, world, n) for r in range(world)]
    pos = 0
    for first, count in chunks:
        assert first == pos and count >= 0  # contiguous, in rank order: disjoint
        pos += count
    assert pos == n  # cover [0, n) once
    sizes = [c for _, c in chunks]
    assert max(sizes) - min(sizes) <= 1
    for bad in ((-1, world), (world, world), (0, 0)):
        with pytest.raises(ValueError):
            dist.ray_chunk(bad[0], bad[1], n)


def test_new_entry_points_are_declared_exported_and_bound(api):
    header = open(os.path.join(ROOT, "include", "rtcuda_amd.h")).read()
    for name in NEW:
        assert name in api.EXPORTS
        assert f"int {name}(" in header
        assert getattr(api.lib(), name).argtypes is not None
    syms = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bT {name}$", syms, re.M), name


def test_symbol_table_has_the_keyed_builds_of_the_persistent_kernel(api):
    """k_paths<PathsKeyed, LDS_TABLES, WIDE = true, MIN_WAVES, DRAW_CIDS, false, false>: the full-pool build draws its rows from the
    frame's counter (4, true), the few-blocks build ties them to slots (2, false); each with tables in LDS and in global memory."""
    syms = subprocess.run(["nm", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for lds in (0, 1):
        for waves, draw in ((4, 1), (2, 0)):
            assert f" _Z7k_pathsI10PathsKeyedLb{lds}ELb1ELi{waves}ELb{draw}ELb0ELb0EE" in syms, (lds, waves, draw)


def test_full_pool_keyed_builds_do_not_spill_vector_registers():
    """As test_full_pool_k_paths_builds_do_not_spill_vector_registers reads the camera builds: the compiler's resource remarks
    of the two 4-waves-per-SIMD k_paths<PathsKeyed> builds report no VGPR spill and an occupancy of at least 4."""
    import shutil
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) and not shutil.which("hipcc"):
        pytest.skip("no hipcc in this environment")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "resource-usage"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = r.stdout.splitlines()
    found = 0
    for k, line in enumerate(lines):
        for lds in (0, 1):
            if f"Function Name: _Z7k_pathsI10PathsKeyedLb{lds}ELb1ELi4ELb1ELb0ELb0EE" in line:
                block = "\n".join(lines[k:k + 12])
                m_spill = re.search(r"VGPRs Spill: (\d+)", block)
                m_occ = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", block)
                assert m_spill and m_occ, block
                assert int(m_occ.group(1)) >= 4, block
                assert int(m_spill.group(1)) == 0, block
                found += 1
    assert found == 2, f"{found} of the 2 full-pool k_paths_keyed builds found in the resource remarks"


def test_recorded_resources_show_the_earlier_builds_unchanged():
    """profiles/render_rays_keyed_resources.md: every k_paths / k_advance / k_paths_rays / k_advance_rays build with this
    commit's SGPR, VGPR, spill and code-size figures next to the parent's -- equal, row by row -- and the four new builds."""
    rows = [l for l in open(os.path.join(ROOT, "profiles", "render_rays_keyed_resources.md")) if l.startswith("| `k_")]
    old = [r for r in rows if "k_paths_keyed" not in r]
    assert len(rows) - len(old) == 4
    count = {"k_paths": 0, "k_advance": 0, "k_paths_rays": 0, "k_advance_rays": 0}
    for r in old:
        c = [x.strip() for x in r.strip().strip("|").split("|")]
        name = c[0].strip("`").split("<")[0]
        count[name] += 1
        sgpr, vgpr, spill, _, _, code = c[1:7]
        assert (sgpr, vgpr, spill, code) == tuple(c[7:11]), r
    assert count == {"k_paths": 24, "k_advance": 2, "k_paths_rays": 8, "k_advance_rays": 2}, count


def test_host_side_argument_errors_name_the_entry_point_and_write_nothing(api):
    """What the library refuses before it needs a device: the null scene comes first."""
    L = api.lib()
    rays = np.zeros(6, np.float32)
    out = np.full(3, 7, np.int64)
    p = rays.ctypes.data
    for name in NEW:
        assert getattr(L, name)(None, 1, p, p, None, 1, 1, 10, 1, 0, 1, 0, out.ctypes.data, None, None) != 0
        msg = L.rt_last_error().decode()
        assert msg.startswith(name + ": ") and "null scene" in msg, msg
    assert (out == 7).all()


class _Scene:
    """A Scene without a device scene: the wrapper's checks run before the library is reached."""

    def __new__(cls, api):
        s = api.Scene.__new__(api.Scene)
        s.L, s.h = api.lib(), None
        return s


def test_wrappers_reject_bad_tensors_and_keys_before_reaching_the_library(api):
    torch = pytest.importorskip("torch")

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    def gpu(x):
        return x.as_subclass(OnGpu)

    sc = _Scene(api)
    o, d = gpu(torch.zeros(8, 3)), gpu(torch.zeros(8, 3))
    raw = dict(o_ptr=1, d_ptr=1, pixel_ptr=0, n_rays=8, n_pixels=8, d_sum_ptr=1)
    cases = [
        ("render_rays_keyed: origins must be on the scene's GPU", lambda: sc.render_rays_keyed(torch.zeros(8, 3), torch.zeros(8, 3), 8)),
        ("dirs must be torch.float32", lambda: sc.render_rays_keyed(o, gpu(torch.zeros(8, 3, dtype=torch.float64)), 8)),
        (r"dirs must have shape \(n, 3\)", lambda: sc.render_rays_keyed(o, gpu(torch.zeros(7, 3)), 8)),
        ("pixel must be torch.int32", lambda: sc.render_rays_keyed(o, d, 8, pixel=gpu(torch.zeros(8, dtype=torch.int64)))),
        ("n_pixels must be a positive int", lambda: sc.render_rays_keyed(o, d, 0)),
        ("out must be a torch tensor on the rays' GPU", lambda: sc.render_rays_keyed(o, d, 8, out=torch.zeros(8, 3))),
        ("key_first must be an int in 0 .. 2\\^64 - 1", lambda: sc.render_rays_keyed_device(key_first=2 ** 64, **raw)),
        ("key_first must be an int", lambda: sc.render_rays_keyed_device(key_first=-1, **raw)),
        ("key_stride must be an int in 0 .. 2\\^32 - 1", lambda: sc.render_rays_keyed_device(key_stride=2 ** 32, **raw)),
        ("seed must be an int", lambda: sc.render_rays_keyed_device(seed=1.5, fixed=True, **raw)),
    ]
    for pattern, call in cases:
        with pytest.raises(api.RtError, match=pattern):
            call()


def test_cpp_wrappers_link_and_throw_the_library_message():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "keyedcheck"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "render_rays_keyed_api_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(l.split("=", 1) for l in out.stdout.splitlines())
    assert lines["render_rays_keyed"] == "render_rays_keyed: rt_render_rays_keyed_device: null scene"
    assert lines["render_rays_keyed_fixed"] == "render_rays_keyed_fixed: rt_render_rays_keyed_fixed_device: null scene"
    assert lines["out"] == "7 7"
