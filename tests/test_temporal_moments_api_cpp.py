"""The C++ wrappers of the single-buffer loop (include/rtcuda/rtcuda.hpp: temporal_accumulate_moments,
temporal_moments_default_params, denoise_variance) compile, link against the product library, hand back the C-ABI's defaults byte
for byte and throw the library's message (tests/cpp/temporal_moments_api_check.cpp).  No GPU is needed: every refusal comes before
a device is touched."""
import os
import subprocess

from conftest import ROOT


def test_cpp_wrappers_link_give_the_abi_defaults_and_throw_the_library_message():
    from rtcuda_amd import api
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "temporalmomentscheck"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "temporal_moments_api_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(l.split("=", 1) for l in out.stdout.splitlines())
    d = api.temporal_moments_default_params()
    got = lines["defaults"].split()
    assert [int(got[0]), int(got[5]), int(got[6])] == [d["max_history"], d["variance_min_history"], 0]
    assert [float(x) for x in got[1:5]] == [d["alpha_min"], d["depth_tolerance"], d["normal_cos_min"], d["emission_tolerance"]]
    assert lines["same_bytes"] == "1"
    me = "temporal_accumulate_moments: rt_temporal_accumulate_moments_fixed: "
    assert lines["null_out"] == me + "null d_len_out"
    assert lines["moments_without_history"] == me + "d_moments_in and d_prev_motion may be set only when history is given"
    assert lines["misaligned"] == me + "d_moments_out must be 16-byte aligned"
    assert lines["tolerance"] == me + "emission_tolerance must be at least 0 (+inf passes every tap)"
    assert lines["min_history"] == me + "variance_min_history must be at least 1, it is 0"
    assert lines["overlap"] == me + "d_variance_out overlaps d_motion"
    assert lines["denoise_variance"] == "denoise_variance: rt_denoise_variance_fixed: null d_variance"
    assert lines["out"] == "7 7 7 7 7 7"
