"""CPU tests of the persistent launch's geometry (rtcuda_amd/csrc/rt_launch_plan.h through librt_hostcheck.so's
rt_plan_paths_launch): what render_shard_impl launches k_paths / k_paths<PathsRays> / k_paths<PathsKeyed> with, for a given shard size,
device and scene.  Every expected value is worked out by hand from the rules as they stood inside render_shard_impl before
they became a function of their own -- none comes from running the function."""
import ctypes
import os

import numpy as np
import pytest

FIELDS = ("blocks", "few_blocks", "lds_bytes", "top_n", "adv_batch", "gen_batch", "tri_follow", "prio_rotate", "rot_wave", "rot_set")
KNOBS = ("RT_PATHS_BLOCKS", "RT_TOP_NODES", "RT_ADV_BATCH", "RT_GEN_BATCH", "RT_TRI_FOLLOW", "RT_PRIO_ROTATE", "RT_ROT_WAVE", "RT_ROT_SET")
W = 1 << 20
CAP = 10        # kPathsLdsStack: the stack entries k_paths keeps in LDS
FIXED = 7424 + 48 + 112   # some shading tables + a camera + the frame's parameters: any number will do, it is passed in
SLOTS_LDS = 4 * 256 * (CAP + 26)  # 36 864 bytes of slot state per workgroup


@pytest.fixture(scope="module")
def plan_lib():
    from rtcuda_amd import api
    api.build()
    L = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    L.rt_plan_paths_launch.argtypes = [ctypes.c_int] * 8 + [ctypes.c_int64, ctypes.c_void_p]
    L.rt_plan_paths_launch.restype = None
    return L


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def plan(L, n, cus=256, wide=True, n_nodes=70000, cap=CAP, lattice=True, width=1920, spp=256, fixed=FIXED):
    out = np.zeros(10, np.int64)
    L.rt_plan_paths_launch(n, cus, int(wide), n_nodes, cap, int(lattice), width, spp, fixed, out.ctypes.data)
    return dict(zip(FIELDS, out.tolist()))


def expect(blocks, few, top_n, adv, prio, rot_wave, rot_set, fixed=FIXED, cap=CAP, gen=6, tri=1):
    return dict(blocks=blocks, few_blocks=int(few), lds_bytes=4 * 256 * (cap + 26) + fixed + top_n * 64, top_n=top_n, adv_batch=adv,
                gen_batch=gen, tri_follow=tri, prio_rotate=prio, rot_wave=rot_wave, rot_set=rot_set)


# 256 CUs, a 4-wide scene, no knobs.  The camera's lattice at 1920 x 256 spp: a slot moves (2^20 / 256) % 1920 = 256 columns per
# generation, gcd(256, 1920) = 128 columns x 256 / 64 = 4 blocks per pixel: a period of 512 blocks -> 512 / 4 = 128 and
# 128 + 512 / 16 = 160.
CASES = {
    # 4096 workgroups halve down to the 1024 wanted; 1024 > 2 x 256: the 4-waves-per-SIMD builds, ADV 20, GEN 6, rotation 2^5
    "full_pool": (dict(n=W), expect(1024, False, 0, 20, 5, 128, 160)),
    # 1/8 shard: 512 workgroups = 2 per CU: few_blocks, ADV 34, rotation 2^8; 2048 waves >= the period of 512
    "eighth": (dict(n=W // 8), expect(512, True, 0, 34, 8, 128, 160)),
    # no lattice (a table's rays): the fallback max(16, 4096 waves / 8) = 512
    "ray_table": (dict(n=W, lattice=False), expect(1024, False, 0, 20, 5, 128, 160)),
    # 100 spp is no multiple of 64: the same fallback
    "spp_100": (dict(n=W, spp=100), expect(1024, False, 0, 20, 5, 128, 160)),
    # 16 workgroups = 64 waves < the period of 512: the fallback max(16, 64 / 8) = 16 -> 4 and 4 + 1
    "n_4096": (dict(n=4096), expect(16, True, 0, 34, 8, 4, 5)),
    # 2-wide, few blocks: min(384, prefix) records of the top of the tree, prefix = min(n_nodes, kTopPrefix = 1024 records, one
    # per 2-wide node): 384 for a tree of 5000 records, all 100 of a tree of 100.  1000 fixed bytes leave room for
    # (65536 - 36864 - 1000) / 64 = 432 records, so the clamp to the 64 KB stays out of it
    "two_wide": (dict(n=W // 8, wide=False, n_nodes=5000, fixed=1000), expect(512, True, 384, 34, 8, 128, 160, fixed=1000)),
    "two_wide_small_tree": (dict(n=W // 8, wide=False, n_nodes=100, fixed=1000), expect(512, True, 100, 34, 8, 128, 160, fixed=1000)),
    # large tables: 36864 + 7584 = 44448 bytes leave (65536 - 44448) / 64 = 329.5 -> 329 records, fewer than the 384 asked for
    "two_wide_lds_clamp": (dict(n=W // 8, wide=False, n_nodes=5000), expect(512, True, 329, 34, 8, 128, 160)),
    # the full pool keeps no records in LDS whatever the format
    "two_wide_full_pool": (dict(n=W, wide=False, n_nodes=5000), expect(1024, False, 0, 20, 5, 128, 160)),
    # a device of 512 CUs holds the full pool's 1024 workgroups two per CU
    "many_cus": (dict(n=W, cus=512), expect(1024, True, 0, 34, 8, 128, 160)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_is_the_hand_derived_one(plan_lib, name):
    args, want = CASES[name]
    got = plan(plan_lib, **args)
    print(name, got)
    assert got == want
    assert got["lds_bytes"] <= 65536


def test_knobs_apply_under_the_experimental_gate(plan_lib, monkeypatch):
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "1")
    monkeypatch.setenv("RT_PATHS_BLOCKS", "300")
    monkeypatch.setenv("RT_ROT_WAVE", "135")
    # 4096 -> 2048 -> 1024 -> 512 -> 256 (the first count <= 300); 256 <= 2 x 256: few_blocks; 1024 waves >= the period 512:
    # rot_set stays 160, rot_wave = 135 & ~3 = 132
    assert plan(plan_lib, W) == expect(256, True, 0, 34, 8, 132, 160)
    # the 4-wide tree keeps whole nodes: RT_TOP_NODES = 101 records -> 100; the other batch knobs are clamped to 1 .. 64
    monkeypatch.setenv("RT_TOP_NODES", "101")
    monkeypatch.setenv("RT_ADV_BATCH", "99")
    monkeypatch.setenv("RT_GEN_BATCH", "0")
    monkeypatch.setenv("RT_TRI_FOLLOW", "0")
    monkeypatch.setenv("RT_PRIO_ROTATE", "3")
    monkeypatch.setenv("RT_ROT_SET", "7")
    assert plan(plan_lib, W) == expect(256, True, 100, 64, 3, 132, 7, gen=1, tri=0)
    # without the gate the same environment changes nothing
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "0")
    assert plan(plan_lib, W) == CASES["full_pool"][1]
