"""CPU tests of the chunked deal's static head and packed semaphores (rtcuda_amd/csrc/rt_slot_chunks.h and rt_launch_plan.h through
librt_hostcheck.so): the head the launch plan picks, its knob, the fall-back to the static deal where the semaphores' LDS
would cost a resident workgroup, which slots the tasks of the dealt tail mean, the inverse of the static deal a runner finds
its semaphore with, and the 16-bit fields.  The expected values are worked out here from the rules, not by
running the function twice."""
import ctypes
import os

import numpy as np
import pytest

W = 1 << 20
LANES = 256
GRID = 1024 * LANES          # the full pool's launch: 1024 workgroups (rt_launch_plan.h)
ROT_WAVE, ROT_SET = 128, 160  # C2's lattice rotation (tests/test_launch_plan_host.py)
BIAS = 0x4000


@pytest.fixture(scope="module")
def L():
    from rtcuda_amd import api
    api.build()
    lib = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    ci, cu, vp = ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p
    lib.rt_plan_slot_head.argtypes = [ci, ci, vp]
    lib.rt_plan_slot_chunk_if_resident.argtypes = [ci, ci]
    lib.rt_plan_slot_chunk.argtypes = [ci, ci, ci]
    lib.rt_plan_paths_launch.argtypes = [ci] * 8 + [ctypes.c_int64, vp]
    lib.rt_plan_paths_launch.restype = None
    lib.rt_slot_chunk_head_tasks.argtypes = [ci] * 6 + [cu, ci, vp, vp, vp]
    lib.rt_slot_chunk_head_tasks.restype = None
    lib.rt_slot_chunk_owner.argtypes = [ci, ci, ci, ci, vp]
    lib.rt_slot_chunk_owner.restype = None
    lib.rt_slot_chunk_static_slot.argtypes = [ci] * 5
    lib.rt_slot_chunk_sem_word.argtypes = [cu]
    lib.rt_slot_chunk_sem_word.restype = cu
    lib.rt_slot_chunk_sem_unit.argtypes = [cu]
    lib.rt_slot_chunk_sem_unit.restype = cu
    lib.rt_slot_chunk_sem_value.argtypes = [cu, cu]
    lib.rt_slot_chunk_sem_init.restype = cu
    lib.rt_slot_chunk_taker_runs.argtypes = [ci]
    lib.rt_slot_chunk_runner_keeps.argtypes = [ci]
    return lib


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in ("RT_SLOT_HEAD", "RT_SLOT_CHUNK", "RT_PATHS_BLOCKS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "0")


def head(L, n):
    sets = ctypes.c_int(0)
    h = L.rt_plan_slot_head(n, 256, ctypes.byref(sets))
    return h, sets.value


def parent_slot(set_, lane_in_grid, grid):
    """The static deal as k_paths has always made it (tests/test_slot_chunks_host.py)."""
    wave, lane = lane_in_grid >> 6, lane_in_grid & 63
    b = (wave + (wave & 3) * ROT_WAVE + set_ * ROT_SET) & ((grid >> 6) - 1)
    return set_ * grid + b * 64 + lane


def test_default_head_by_slot_sets(L):
    """max(0, sets - 2): the full pool (4 slots per lane) runs two sets statically and deals two, the 2-shard frame is dealt
    whole, and a 4-shard frame -- one slot per lane, dealt only when RT_SLOT_CHUNK asks -- has no head either."""
    assert head(L, W) == (2, 4)
    assert head(L, W // 2) == (0, 2)
    assert head(L, W // 4) == (0, 1)


def test_head_knob_works_only_behind_the_gate(L, monkeypatch):
    monkeypatch.setenv("RT_SLOT_HEAD", "1")
    assert head(L, W) == (2, 4)            # without the gate the knob changes nothing
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "1")
    assert head(L, W) == (1, 4)
    for asked, got in ((0, 0), (2, 2), (3, 3), (4, 3), (99, 3), (-5, 0)):   # clamped to 0 .. sets - 1: one set is always dealt
        monkeypatch.setenv("RT_SLOT_HEAD", str(asked))
        assert head(L, W) == (got, 4), asked
    monkeypatch.setenv("RT_SLOT_HEAD", "1")
    assert head(L, W // 2) == (1, 2) and head(L, W // 4) == (0, 1)
    # G is untouched by the head's knob: still chain / 8
    assert L.rt_plan_slot_chunk(W, 256, 506) == 64
    # fewer workgroups, more sets per lane: never more than the four dealt sets the semaphores hold
    monkeypatch.setenv("RT_SLOT_HEAD", "0")
    monkeypatch.setenv("RT_PATHS_BLOCKS", "256")
    assert head(L, W) == (12, 16)
    monkeypatch.delenv("RT_SLOT_HEAD")
    assert head(L, W) == (14, 16)


def test_static_deal_where_the_semaphores_do_not_fit(L):
    """The semaphores are 2 KB of static LDS in k_paths<PathsChunked>.  The host asks the device how many workgroups of that kernel a
    CU holds at the plan's dynamic LDS; below the four the plan assumes, the frame keeps the static deal."""
    assert L.rt_plan_slot_chunk_if_resident(64, 4) == 64 and L.rt_plan_slot_chunk_if_resident(64, 5) == 64
    assert L.rt_plan_slot_chunk_if_resident(64, 3) == 0 and L.rt_plan_slot_chunk_if_resident(3, 0) == 0
    assert L.rt_plan_slot_chunk_if_resident(0, 4) == 0
    # what that means in bytes, from the plan's own LDS figure: four workgroups share a CU's 160 KB.  C2's small tables leave
    # room for the 2 KB + 32 bytes; 64 materials and 64 lights staged in LDS (7 424 bytes of tables) did not fit four times
    # even before, and such a scene keeps the static deal.
    def lds(fixed):
        out = np.zeros(10, np.int64)
        L.rt_plan_paths_launch(W, 256, 1, 70000, 10, 1, 1920, 256, fixed, out.ctypes.data)
        return int(out[2])
    static = 2048 + 32
    small, large = lds(400 + 48 + 112), lds(7424 + 48 + 112)
    assert small == 4 * 256 * 36 + 560 and large == 4 * 256 * 36 + 7584
    assert 4 * (small + static) <= 160 * 1024 < 4 * (large + static)
    assert 160 * 1024 // (large + static) == 3 and L.rt_plan_slot_chunk_if_resident(64, 160 * 1024 // (large + static)) == 0


@pytest.mark.parametrize("sets,hd", [(4, 2), (4, 0), (4, 3), (4, 1), (2, 0), (2, 1), (1, 0)])
def test_dealt_tasks_cover_exactly_the_sets_behind_the_head(L, sets, hd):
    n = sets * GRID
    S = (sets - hd) * LANES
    for block in (0, 517, 1023):
        dealt = sorted(parent_slot(s, block * LANES + l, GRID) for s in range(hd, sets) for l in range(LANES))
        for level in (0, 5):
            slots, levels, idx = (np.zeros(S, np.int32) for _ in range(3))
            L.rt_slot_chunk_head_tasks(block, sets, hd, GRID, ROT_WAVE, ROT_SET, level * S, S, slots.ctypes.data, levels.ctypes.data, idx.ctypes.data)
            assert sorted(slots.tolist()) == dealt and (levels == level).all()
            assert idx.tolist() == list(range(S))      # entry idx = task mod S: set (idx / 256) behind the head, lane idx % 256
            assert 0 <= slots.min() and slots.max() < n
            # the runner's way back from its slot to that entry
            out = np.zeros(2, np.int32)
            for k in (0, 63, 64, 255, S - 256, S - 1):
                L.rt_slot_chunk_owner(int(slots[k]), GRID, ROT_WAVE, ROT_SET, out.ctypes.data)
                assert (out[0] - hd) * LANES + (out[1] & 255) == k and out[1] >> 8 == block, (block, k, out)


def test_owner_inverts_the_static_deal(L):
    out = np.zeros(2, np.int32)
    rng = np.random.default_rng(5)
    for grid, rw, rs, sets in ((GRID, ROT_WAVE, ROT_SET, 4), (GRID, 0, 0, 2), (4096, 4, 5, 3), (256, 12, 7, 2), (GRID // 2, 64, 83, 4)):
        for _ in range(300):
            s, lane = int(rng.integers(sets)), int(rng.integers(grid))
            slot = L.rt_slot_chunk_static_slot(s, lane, grid, rw, rs)
            L.rt_slot_chunk_owner(slot, grid, rw, rs, out.ctypes.data)
            assert (int(out[0]), int(out[1])) == (s, lane), (grid, rw, rs, s, lane, slot)


def test_packed_fields(L):
    """Entry idx is the 16-bit field idx & 1 of word idx >> 1 and holds bias + the semaphore: banked is bias + 1."""
    assert L.rt_slot_chunk_sem_init() == (BIAS + 1) | (BIAS + 1) << 16
    for idx in (0, 1, 2, 255, 256, 1022, 1023):
        assert L.rt_slot_chunk_sem_word(idx) == idx // 2
        assert L.rt_slot_chunk_sem_unit(idx) == (1 if idx % 2 == 0 else 1 << 16)
        assert L.rt_slot_chunk_sem_value(L.rt_slot_chunk_sem_init(), idx) == 1
    assert L.rt_slot_chunk_sem_word(1023) < 512            # 1 024 fields: 2 KB


def test_fields_never_borrow_within_the_bound(L):
    """A slot has at most 2 047 tasks (camera-ray ids stay 13 W below 2^31), each lowers its field once at most: with every
    task a claim the field reaches bias + 1 - 2 047, and the neighbour, whatever it holds in [bias - 2 046, bias + 1], reads
    the same before and after; the decisions on the unpacked value are the old ones."""
    M = 0xffffffff
    for idx in (6, 7):
        unit, other = L.rt_slot_chunk_sem_unit(idx), idx ^ 1
        for neighbour in (BIAS - 2046, BIAS, BIAS + 1):
            word = L.rt_slot_chunk_sem_init()
            shift_o = 16 * (other & 1)
            word = (word & ~(0xffff << shift_o) & M) | neighbour << shift_o
            want = 1
            for step in range(2047):          # fetch_sub by every task of the slot
                old = word
                assert L.rt_slot_chunk_sem_value(old, idx) == want
                assert bool(L.rt_slot_chunk_taker_runs(L.rt_slot_chunk_sem_value(old, idx))) == (step == 0)
                word = (word - unit) & M
                want -= 1
                assert L.rt_slot_chunk_sem_value(word, other) == neighbour - BIAS
            assert want == -2046 and L.rt_slot_chunk_sem_value(word, idx) == -2046
            for step in range(2047):          # and the releases back up to banked
                old = L.rt_slot_chunk_sem_value(word, idx)
                assert bool(L.rt_slot_chunk_runner_keeps(old)) == (old < 0)
                word = (word + unit) & M
                assert L.rt_slot_chunk_sem_value(word, other) == neighbour - BIAS
            assert L.rt_slot_chunk_sem_value(word, idx) == 1
