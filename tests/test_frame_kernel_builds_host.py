"""The frame kernels the library holds: exactly the instances of k_paths<BUILD, ...> and k_advance<SRC, ...> that the host's
selection can launch (FrameRun::run_persistent, paths_kernel_of), read from the built library's symbol table.  No GPU.

The two kernels are templates over a build tag and a source type, and a template is instantiated by naming it: a selector that
names one build too many adds a kernel nobody launches (compile time, code object size), one too few is a link error at best.
The table below is the whole set, per tag; the test holds the symbol table to it, no more and no fewer."""
import re
import subprocess

# (WIDE, MIN_WAVES, DRAW_CIDS, LITERAL, VERIFY) of the instances of a tag; each exists with LDS_TABLES = false and true.
#   (w, 4, 0, 0, v)  the full pool, default (v = 1) and RT_FLAG_WATERTIGHT        (w, 2, 0, 0, v)  the same on few blocks
#   (w, 4, 1, 0, 0)  per-sample streams on the full pool: drawn ids               (0, n, 0, 1, 0)  RT_FLAG_REFERENCE_WALK
FULL = [(w, 4, 0, 0, v) for w in (0, 1) for v in (0, 1)]
FEW = [(w, 2, 0, 0, v) for w in (0, 1) for v in (0, 1)]
CAMERA = FULL + FEW + [(w, 4, 1, 0, 0) for w in (0, 1)] + [(0, 4, 0, 1, 0), (0, 2, 0, 1, 0)]
CHUNKED = FULL + [(0, 4, 0, 1, 0)]                              # the 4-waves-per-SIMD reference-mode instances only
RAYS = [(1, n, 0, 0, v) for n in (4, 2) for v in (0, 1)]        # 4-wide tree only, no reference walk
STREAMS = [(1, 4, 1, 0, 0), (1, 2, 0, 0, 0)]                    # per-sample streams only: drawn on the full pool, tied to slots on few blocks
K_PATHS = {
    "11PathsCamera": CAMERA,
    "7PathsBg": CAMERA,
    "12PathsChunked": CHUNKED,
    "14PathsChunkedBg": CHUNKED,
    "9PathsRays": RAYS,
    "10PathsKeyed": STREAMS,
    "11PathsCounts": STREAMS,
}
K_ADVANCE = ["N2rt6CameraE", "8RayTable"]  # the sources whose frames can run on the round pipeline


def expected_symbols():
    """The template-argument heads `_Z7k_pathsI...E` / `_Z9k_advanceI...E` of every instance."""
    out = set()
    for tag, builds in K_PATHS.items():
        for lds in (0, 1):
            for wide, waves, draw, lit, ver in builds:
                out.add(f"_Z7k_pathsI{tag}Lb{lds}ELb{wide}ELi{waves}ELb{draw}ELb{lit}ELb{ver}EE")
    for src in K_ADVANCE:
        for lds in (0, 1):
            out.add(f"_Z9k_advanceI{src}Lb{lds}EE")
    return out


def test_the_table_lists_the_builds_of_every_tag():
    assert {t: 2 * len(b) for t, b in K_PATHS.items()} == {"11PathsCamera": 24, "7PathsBg": 24, "12PathsChunked": 10, "14PathsChunkedBg": 10,
                                                          "9PathsRays": 8, "10PathsKeyed": 4, "11PathsCounts": 4}
    exp = expected_symbols()
    assert len([s for s in exp if "k_paths" in s]) == 84 and len([s for s in exp if "k_advance" in s]) == 4


def test_symbol_table_has_exactly_the_frame_kernels_the_host_selects():
    from rtcuda_amd import api
    api.lib()
    syms = subprocess.run(["nm", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    # every symbol whose name is k_paths or k_advance followed by anything: a kernel of another name (k_paths_more,
    # k_advance_unused) is as much a build too many as another instance of the templates.  A kernel has two symbols in the host
    # library: its handle under the kernel's own name, and the host stub that launches it.
    found, stubs = set(), 0
    for line in syms.splitlines():
        m = re.search(r" \w (_Z\d+(__device_stub__)?k_(?:paths|advance)\w*)$", line)
        if not m:
            continue
        if m.group(2):
            stubs += 1
            continue
        head = re.match(r"(_Z\d+k_(?:paths|advance)I.*?EE)v6DScene", m.group(1))
        found.add(head.group(1) if head else m.group(1))
    assert stubs == len(found), (stubs, len(found))
    exp = expected_symbols()
    assert found - exp == set(), f"frame kernels nobody selects: {sorted(found - exp)}"
    assert exp - found == set(), f"frame kernels missing from the library: {sorted(exp - found)}"
