"""GPU tests of the header's promises to HOST THREADS: renders are thread-safe, rendering may overlap queries and renders of the
same scene, AOV calls and queries of one scene take turns, rt_last_error is per thread.  Run with -m gpu.

The threaded work runs once, in one child process (tests/host_threads_worker.py, which describes the cases): a lock-order
mistake shows as a deadlock, and a deadlocked ctypes call cannot be interrupted from Python.  The worker computes, per case, the
serial answers first and the threaded ones after them, compares bits, and writes one verdict per case; each test below asserts
its own case's verdict.  If the child outlives WORKER_TIMEOUT it is killed and the whole session ends (pytest.exit): after a hang
nothing more is started on the GPU, and the hang is a finding whose cause is to be read from the lock code
(profiles/concurrency_contract.md has the lock table), not found by running the worker again."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# The worker's wall time on an MI355X, process start and imports included, measured once: WORKER_SECONDS (the seven cases take
# 7.4 s of it; profiles/concurrency_contract.md).  The limit is ten times that and not below 120 s: 120 s.
WORKER_SECONDS = 9.6
WORKER_TIMEOUT = max(120.0, 10.0 * WORKER_SECONDS)


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_threads") / "verdicts.json")
    env = dict(os.environ, RTCUDA_EXPERIMENTAL="1")
    env.pop("RT_STACK_CAP", None)
    try:
        done = subprocess.run([sys.executable, os.path.join(HERE, "host_threads_worker.py"), "--out", out], env=env, capture_output=True,
                              text=True, timeout=WORKER_TIMEOUT)  # (on a timeout run() kills the child and waits for it)
    except subprocess.TimeoutExpired:
        case = "before the first case"
        if os.path.exists(out):
            with open(out) as f:
                case = json.load(f).get("in_progress") or "after the last case"
        pytest.exit(f"tests/host_threads_worker.py did not finish within {WORKER_TIMEOUT:.0f} s and was killed; case in progress: {case}. "
                    "A hang of the threaded library: nothing more is started on the GPU in this session", returncode=3)
    print(done.stdout[-4000:], done.stderr[-4000:])
    assert os.path.exists(out), (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    with open(out) as f:
        result = json.load(f)
    result["returncode"], result["stderr"] = done.returncode, done.stderr[-2000:]
    return result


def _assert_case(verdicts, name):
    assert name in verdicts["cases"], (f"the worker ended (exit status {verdicts['returncode']}) before case {name} had a verdict; "
                                       f"in progress: {verdicts['in_progress']}", verdicts["stderr"])
    assert verdicts["cases"][name]["passed"], verdicts["cases"][name]["detail"]


def test_t1_one_context_four_seeds(verdicts):
    """Four threads, render_shard_fixed of one scene at 128 x 72 x 256 with seeds 1 to 4: they queue on one Context::busy, and the
    RNG-state cache is re-keyed at every hand-over.  Sums and event totals equal the serial frame of each seed."""
    _assert_case(verdicts, "t1")


def test_t2_three_contexts_in_flight_with_overflow_stacks(verdicts):
    """RT_STACK_CAP=2; shards (0,1), (0,2), (1,4) of one 256 x 256 x 4 frame: three contexts, each with its own overflow buffer."""
    _assert_case(verdicts, "t2")


def test_t3_first_use_of_everything_at_once(verdicts):
    """Six threads, six entry points, one barrier, a scene no call has touched: the reference's tree, the query scratch, the
    inverse leaf order and the AOV events are all made by racing first calls."""
    _assert_case(verdicts, "t3")


def test_t4_records_repadded_under_load(verdicts):
    """query_closest from 10 to 1e4 scene sizes out re-pads the node records in place while 128 x 72 x 256 frames of the same scene
    are in flight: frames and hits equal the serial ones."""
    _assert_case(verdicts, "t4")


def test_t5_edits_of_one_scene_while_another_renders(verdicts):
    _assert_case(verdicts, "t5")


def test_t6_last_error_belongs_to_the_thread(verdicts):
    _assert_case(verdicts, "t6")


def test_t7_host_output_path(verdicts):
    """Three threads, rt_render at three sizes: the device's cached output buffers regrow between calls under g_dev_busy."""
    _assert_case(verdicts, "t7")


def test_the_worker_ended_cleanly(verdicts):
    assert verdicts["returncode"] == 0 and verdicts["in_progress"] is None, (verdicts["returncode"], verdicts["in_progress"], verdicts["stderr"])
