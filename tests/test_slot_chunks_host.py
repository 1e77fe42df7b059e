"""CPU tests of the chunked deal of k_paths (rtcuda_amd/csrc/rt_slot_chunks.h through librt_hostcheck.so): which slot a task
of a workgroup means, how many tasks there are, and the decisions of the hand-over.  The expected values are worked out
here from the rules, not by running the function twice."""
import ctypes
import os

import numpy as np
import pytest

W = 1 << 20
LANES = 256
GRID = 1024 * LANES          # the full pool's launch: 1024 workgroups (rt_launch_plan.h)
ROT_WAVE, ROT_SET = 128, 160  # C2's lattice rotation (tests/test_launch_plan_host.py)


@pytest.fixture(scope="module")
def L():
    from rtcuda_amd import api
    api.build()
    lib = ctypes.CDLL(os.path.join(os.path.dirname(api.LIB_PATH), "librt_hostcheck.so"))
    ci, cu, vp = ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p
    lib.rt_slot_chunk_tasks.argtypes = [ci, ci, ci, ci, ci, cu, ci, vp, vp]
    lib.rt_slot_chunk_tasks.restype = None
    lib.rt_slot_chunk_static_slot.argtypes = [ci] * 5
    lib.rt_slot_chunk_levels.argtypes = [cu, cu]
    lib.rt_slot_chunk_levels.restype = cu
    lib.rt_slot_chunk_task_count.argtypes = [cu, cu, cu]
    lib.rt_slot_chunk_task_count.restype = cu
    lib.rt_slot_chunk_ends.argtypes = [cu, cu, ci]
    lib.rt_slot_chunk_taker_runs.argtypes = [ci]
    lib.rt_slot_chunk_runner_keeps.argtypes = [ci]
    lib.rt_plan_slot_chunk.argtypes = [ci, ci, ci]
    return lib


def tasks(L, block, sets, grid, t0, count):
    slots, levels = np.zeros(count, np.int32), np.zeros(count, np.int32)
    L.rt_slot_chunk_tasks(block, sets, grid, ROT_WAVE, ROT_SET, t0, count, slots.ctypes.data, levels.ctypes.data)
    return slots, levels


def parent_slot(set_, lane_in_grid, grid):
    """The static deal as k_paths has always made it: wave j of a workgroup shifted by j * rot_wave 64-slot blocks, slot set k
    by k * rot_set."""
    wave, lane = lane_in_grid >> 6, lane_in_grid & 63
    b = (wave + (wave & 3) * ROT_WAVE + set_ * ROT_SET) & ((grid >> 6) - 1)
    return set_ * grid + b * 64 + lane


@pytest.mark.parametrize("shards", [4, 2, 1])
def test_tasks_of_a_level_are_a_bijection_onto_the_workgroups_own_slots(L, shards):
    """Shards 4, 2, 1 of W = 2^20 on the full launch of 1024 workgroups: 1, 2, 4 slots per lane."""
    n = W // shards
    sets = n // GRID
    assert sets == {4: 1, 2: 2, 1: 4}[shards]
    S = sets * LANES
    for block in (0, 1, 517, 1023):
        own = sorted(parent_slot(s, block * LANES + l, GRID) for s in range(sets) for l in range(LANES))
        assert len(set(own)) == S and 0 <= own[0] and own[-1] < n
        for s in range(sets):
            for l in (0, 63, 64, 255):
                assert L.rt_slot_chunk_static_slot(s, block * LANES + l, GRID, ROT_WAVE, ROT_SET) == parent_slot(s, block * LANES + l, GRID)
        for level in (0, 1, 31):
            slots, levels = tasks(L, block, sets, GRID, level * S, S)
            assert sorted(slots.tolist()) == own
            assert (levels == level).all()
            # entry idx <-> (set idx / 256, lane idx % 256), level-major
            assert slots[0] == parent_slot(0, block * LANES, GRID) and slots[S - 1] == parent_slot(sets - 1, block * LANES + 255, GRID)
    # the workgroups' slots partition the shard
    seen = np.zeros(n, np.int32)
    for block in range(1024):
        slots, _ = tasks(L, block, sets, GRID, 0, S)
        seen[slots] += 1
    assert (seen == 1).all()


def test_lanes_asking_together_get_consecutive_slots(L):
    """A wave that asks for k tasks in one GEN block draws t .. t + k - 1: consecutive slots (samples of one pixel at spp = 256)
    as long as the run stays inside one wave's 64 slots of a set."""
    sets, S = 4, 4 * LANES
    for block in (0, 700):
        slots, _ = tasks(L, block, sets, GRID, 3 * S, S)
        for start in range(0, S, 64):
            run = slots[start:start + 64]
            assert (np.diff(run) == 1).all(), (block, start)


@pytest.mark.parametrize("G", [1, 3, 16, 600])
def test_levels_cover_the_chain(L, G):
    for rays in (506, 507):
        lv = L.rt_slot_chunk_levels(rays, G)
        assert (lv - 1) * G < rays <= lv * G
        assert L.rt_slot_chunk_task_count(4, rays, G) == 4 * LANES * lv
        # the chunk ends the kernel sees along the chain: one per multiple of G below `rays`, none on a lane that has made no
        # ray of this slot yet
        ends = [g for g in range(1, rays) if L.rt_slot_chunk_ends(g, G, 0)]
        assert ends == list(range(G, rays, G))
        assert len(ends) + 1 == lv
        assert not any(L.rt_slot_chunk_ends(g, G, 1) for g in range(0, rays, max(1, G)))
    assert L.rt_slot_chunk_levels(506, 600) == 1


def test_multiples_without_a_division(L):
    for G in (1, 2, 3, 5, 6, 7, 8, 12, 16, 24, 32, 48, 64, 507, 1 << 20):
        for gen in list(range(0, 2100)) + [G * 1000, G * 1000 + 1, 0x7ffffffe, 0x7fffffff]:
            assert bool(L.rt_slot_chunk_ends(gen, G, 0)) == (gen % G == 0), (G, gen)


def test_semaphore_decisions(L):
    # taker: old value of fetch_sub(sem, 1); 1 = banked
    assert L.rt_slot_chunk_taker_runs(1) and not L.rt_slot_chunk_taker_runs(0) and not L.rt_slot_chunk_taker_runs(-3)
    # runner: old value of fetch_add(sem, 1); negative = a claim is pending
    assert L.rt_slot_chunk_runner_keeps(-1) and L.rt_slot_chunk_runner_keeps(-4) and not L.rt_slot_chunk_runner_keeps(0)


def test_knob_travels_through_the_launch_plan(L, monkeypatch):
    monkeypatch.delenv("RT_SLOT_CHUNK", raising=False)
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "0")
    # the default: 8 tasks per slot for chains of 384 .. 768 rays (C2, C4: 506), the plain kernel for every other frame
    # (C5: 1 012, C3: 2 025; short chains)
    assert [L.rt_plan_slot_chunk(W, 256, c) for c in (506, 384, 768, 383, 769, 1012, 2025, 126, 3)] == [64, 48, 96, 0, 0, 0, 0, 0, 0]
    assert L.rt_plan_slot_chunk(W // 2, 256, 506) == 64
    assert L.rt_plan_slot_chunk(W // 4, 256, 506) == 0    # one slot per lane: nothing to deal
    assert L.rt_plan_slot_chunk(W // 8, 256, 506) == 0    # 2 waves per SIMD: the static deal, whatever the knob
    monkeypatch.setenv("RT_SLOT_CHUNK", "3")
    assert L.rt_plan_slot_chunk(W, 256, 506) == 64        # without the gate the knob changes nothing
    monkeypatch.setenv("RTCUDA_EXPERIMENTAL", "1")
    assert L.rt_plan_slot_chunk(W, 256, 506) == 3 and L.rt_plan_slot_chunk(W, 256, 2025) == 3
    assert L.rt_plan_slot_chunk(W // 4, 256, 506) == 3
    assert L.rt_plan_slot_chunk(W // 8, 256, 506) == 0
    monkeypatch.setenv("RT_SLOT_CHUNK", "0")
    assert L.rt_plan_slot_chunk(W, 256, 506) == 0


def test_chunked_kernels_do_not_spill_vector_registers():
    """k_paths<PathsChunked, ...> lives on the same 128-VGPR budget as the 4-waves-per-SIMD builds of k_paths (tests/test_host_logic.py): no
    VGPR spill and 4 waves per SIMD in each of the 10 instances the library launches."""
    import re
    import shutil
    import subprocess
    from conftest import ROOT
    if not os.path.exists("/opt/rocm/bin/hipcc") and not shutil.which("hipcc"):
        pytest.skip("no hipcc in this environment")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "resource-usage"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = r.stdout.splitlines()
    found = 0
    for k, line in enumerate(lines):
        if re.search(r"Function Name: _Z7k_pathsI12PathsChunkedLb[01]ELb[01]ELi4ELb0E", line):
            block = "\n".join(lines[k:k + 12])
            m_spill, m_occ = re.search(r"VGPRs Spill: (\d+)", block), re.search(r"Occupancy \[waves/SIMD\]: (\d+)", block)
            m_vgpr = re.search(r" VGPRs: (\d+)", block)
            assert m_spill and m_occ and m_vgpr, block
            assert int(m_spill.group(1)) == 0 and int(m_occ.group(1)) >= 4 and int(m_vgpr.group(1)) <= 128, block
            found += 1
    assert found == 10, f"{found} of the 10 chunked builds found in the resource remarks"
