"""The hand-over protocol of k_paths' chunked deal (rtcuda_amd/csrc/rt_slot_chunks.h) played by host threads:
tests/cpp/slot_chunks_check.cpp includes the header the kernel includes, with std::atomic standing in for a slot's semaphore.
Threads are lanes; they yield at random, the slots' chains are ragged, and there are more tasks than the chains need.  The
program itself asserts that every ray index of every slot ran exactly once and in order, that no slot ever had two runners,
and that all tasks were dealt; it exits 0 only then.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "tests", "cpp", "slot_chunks_check")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "chunkscheck"], stdout=subprocess.DEVNULL)
    assert os.path.exists(EXE)
    return EXE


# lanes, slot sets, G, seed, surplus levels
CASES = [
    (8, 1, 3, 1, 2),     # one slot per lane-entry, G does not divide the chains: claims and runner-continues
    (6, 2, 1, 2, 0),     # every ray a chunk; exactly as many levels as the longest chain needs
    (8, 4, 16, 3, 1),    # four sets, the shape of the full pool
    (5, 1, 100, 4, 3),   # G larger than every chain: one task per slot does all the work, the rest are surplus
    (3, 1, 1, 5, 1),
    (16, 1, 2, 6, 4),    # more threads than cores on a small machine: long preemptions inside the protocol
]


@pytest.mark.parametrize("lanes,sets,G,seed,surplus", CASES)
def test_every_ray_runs_once_and_in_order(exe, lanes, sets, G, seed, surplus):
    r = subprocess.run([exe, str(lanes), str(sets), str(G), str(seed), str(surplus)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith(f"ok lanes={lanes} sets={sets} G={G} seed={seed}")
