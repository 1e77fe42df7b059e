"""The chunked deal of k_paths with a static head and semaphores packed two to a word (rtcuda_amd/csrc/rt_slot_chunks.h), played
by host threads: tests/cpp/slot_chunks_head_check.cpp includes the header the kernel includes, and std::atomic<uint32_t> words
stand in for the workgroup's semaphore words in LDS.  Threads are lanes.  Each first runs the slots of its `head` first slot
sets for their whole chains, then the remaining sets are dealt G rays at a time; lanes yield at random, the chains are ragged
and there are more tasks than the chains need.  The program itself asserts that every ray index of every slot ran exactly
once and in order, that no slot ever had two runners, that all tasks were dealt and that no 16-bit field ever left
[bias - tasks of a slot, bias + 1] (so no field borrows from or carries into its neighbour); it exits 0 only then.
No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "tests", "cpp", "slot_chunks_head_check")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "chunksheadcheck"], stdout=subprocess.DEVNULL)
    assert os.path.exists(EXE)
    return EXE


# lanes, slot sets, G, head, seed, surplus levels, live dealt entries (0 = all)
CASES = [
    (8, 4, 16, 2, 1, 1, 0),    # the full pool's shape at its default head: two sets static, two dealt
    (8, 4, 3, 0, 2, 2, 0),     # everything dealt, G does not divide the chains
    (8, 4, 1, 3, 3, 0, 0),     # one dealt slot per lane-entry, every ray a chunk: claims pile up in neighbouring fields
    (6, 2, 1, 0, 4, 0, 0),     # the 2-shard frame's shape; exactly as many levels as the longest chain needs
    (16, 1, 2, 0, 5, 4, 0),    # more threads than cores on a small machine: long preemptions inside the protocol
    (8, 2, 2, 1, 6, 2, 201),   # an odd number of entries: the last word has one field
]


@pytest.mark.parametrize("lanes,sets,G,head,seed,surplus,live", CASES)
def test_every_ray_runs_once_and_fields_stay_in_range(exe, lanes, sets, G, head, seed, surplus, live):
    r = subprocess.run([exe] + [str(v) for v in (lanes, sets, G, head, seed, surplus, live)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith(f"ok lanes={lanes} sets={sets} G={G} head={head} seed={seed}")
    if live:
        assert f"dealt entries={live} of {(sets - head) * 256} words={(live + 1) // 2} " in r.stdout
