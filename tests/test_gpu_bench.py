"""bench.py end to end on a small frame (-m gpu): a plain run times the headline and leaves out every record that takes a run
of its own; --full still measures and checks them.

The frame is two generations of the slot pool (256x128x64 = 2^21 samples), so the timed kernel is the persistent one the
headline times, and --cpu-spp equals --spp, so the oracle's sample is the timed frame itself and the per-sample guard of the
parity block compares like with like.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

# records of the line that take runs of their own (extra_configs needs the 1920x1080 frame, so it is null here either way)
FULL_ONLY = ("roofline", "parity", "cpu_baseline", "reference_decisions", "per_sample", "reference_walk_mode")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k != "RTCUDA_EXPERIMENTAL"}  # (bench.py runs without the experiment gate)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--width", "256", "--height", "128", "--spp", "64",
                        "--cpu-spp", "64", "--steps", "2", "--warmup", "1", *extra],
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_times_the_headline_and_nothing_else(tmp_path):
    line = _bench("--dump-outputs", str(tmp_path))
    assert "invalid" not in line and line["value"] > 0 and line["ms_per_step"] > 0
    assert (line["unit"], line["higher_is_better"], line["dtype"], line["steps"], line["warmup"]) == ("Msamples/s", True, "f32", 2, 1)
    assert line["event_totals"]["summed_over_ranks"]["camera_rays"] == 256 * 128 * 64
    for k in FULL_ONLY:
        assert line.get(k) is None, k
    assert np.load(tmp_path / "image.npy").shape == (128, 256, 3)
    assert np.array_equal(np.load(tmp_path / "event_totals.npy"),
                          [line["event_totals"]["summed_over_ranks"][k] for k in line["dump_outputs"]["event_totals_keys"]])


def test_full_run_measures_and_checks_the_rest():
    line = _bench("--full")
    assert "invalid" not in line and line["value"] > 0
    for k in FULL_ONLY:
        assert line.get(k) is not None, k
    assert line["parity"]["events_equal"] and line["parity"]["watertight_flag"]["events_equal"]
    assert line["parity"]["reference_walk_mode"]["events_equal"]
    assert line["roofline"]["kernel"] == "k_paths" and "calibration_error" not in line["roofline"]
    assert line["cpu_baseline"]["value"] > 0
