"""The register budget of the builds that pass over background pixels (k_paths<PathsBg>, k_paths<PathsChunkedBg>: DESIGN section 5).  No GPU.

They run every BASELINE frame, on the same 128-VGPR budget as the 4-waves-per-SIMD builds of k_paths (tests/test_host_logic.py)
and k_paths<PathsChunked> (tests/test_slot_chunks_host.py): no VGPR spill and 4 waves per SIMD in every 4-wave instance the library
launches.  A build that tips into spills loses 4 - 6 % of the frame and nothing else shows it."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

# mangled names: k_paths<PathsBg, LDS_TABLES, WIDE, 4, DRAW_CIDS, LITERAL, VERIFY>, k_paths<PathsChunkedBg, LDS_TABLES, WIDE, 4, false, ...>
# (the keys stay the builds' short names: they are the test ids)
BUILDS = {
    # both LDS_TABLES x (literal; per-sample, wide and not; default and watertight, wide and not) = 2 x 7
    "k_paths_bg": (r"Function Name: _Z7k_pathsI7PathsBgLb[01]ELb[01]ELi4ELb[01]E", 14),
    # both LDS_TABLES x (literal; default and watertight, wide and not) = 2 x 5
    "k_paths_chunked_bg": (r"Function Name: _Z7k_pathsI14PathsChunkedBgLb[01]ELb[01]ELi4ELb0E", 10),
}


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists("/opt/rocm/bin/hipcc") and not shutil.which("hipcc"):
        pytest.skip("no hipcc in this environment")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "rtcuda_amd", "csrc"), "resource-usage"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout.splitlines()


@pytest.mark.parametrize("kernel", sorted(BUILDS))
def test_background_kernels_do_not_spill_vector_registers(remarks, kernel):
    pattern, expected = BUILDS[kernel]
    found = 0
    for k, line in enumerate(remarks):
        if re.search(pattern, line):
            block = "\n".join(remarks[k:k + 12])
            m_spill, m_occ = re.search(r"VGPRs Spill: (\d+)", block), re.search(r"Occupancy \[waves/SIMD\]: (\d+)", block)
            m_vgpr = re.search(r" VGPRs: (\d+)", block)
            assert m_spill and m_occ and m_vgpr, block
            print(line.split("Function Name: ")[1][:60], "VGPRs", m_vgpr.group(1), "spill", m_spill.group(1), "occupancy", m_occ.group(1))
            assert int(m_spill.group(1)) == 0 and int(m_occ.group(1)) >= 4 and int(m_vgpr.group(1)) <= 128, block
            found += 1
    assert found == expected, f"{found} of the {expected} 4-wave {kernel} builds found in the resource remarks"
