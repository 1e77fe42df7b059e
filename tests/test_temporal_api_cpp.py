"""The C++ wrappers of temporal accumulation (include/rtcuda/rtcuda.hpp: render_motion, temporal_accumulate,
temporal_default_params) compile, link against the product library and throw the library's message (tests/cpp/temporal_api_check.cpp).
No GPU is needed: every refusal comes before a device is touched."""
import os
import subprocess

from conftest import ROOT


def test_cpp_wrappers_link_and_throw_the_library_message():
    from rtcuda_amd import api
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "temporalcheck"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "temporal_api_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(l.split("=", 1) for l in out.stdout.splitlines())
    me = "temporal_accumulate: rt_temporal_accumulate_fixed: "
    assert lines["defaults"] == str(api.temporal_default_params()["max_history"])
    assert lines["render_motion"] == "render_motion: rt_render_motion: null scene"
    assert lines["null_out"] == me + "null d_len_out"
    assert lines["max_history"] == me + "max_history must be at least 1, it is 0"
    assert lines["buffers"] == me + "d_sum_b and d_hist_b_out must be null together"
    assert lines["samples"].startswith(me + "samples_a, samples_b")
    assert lines["overlap"] == me + "d_hist_a_out overlaps d_sum_a"
    assert lines["out"] == "7 7 7 7 7"
