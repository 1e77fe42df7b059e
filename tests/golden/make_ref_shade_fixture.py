#!/usr/bin/env python3
"""Regenerates tests/golden/ref_shade_fixture.npz from the REFERENCE'S OWN shading functions (only where /root/reference exists).

`make -C oracle _ref_shade` compiles oracle/ref_shade_driver.cpp (own code) against the reference's device headers --
included by path, unmodified, under oracle/ref_shim.h -- into oracle/_ref/ref_shade (git-ignored).  This script writes the
input tables of tests/shade_scenes.py shade_tables() into oracle/_ref/, runs the driver, and stores inputs and outputs as
32-bit patterns: in_<function>, out_<function>.  Numbers only.  Where a row supplies uniforms it holds the RAW 32-bit draws;
the driver is given curand_uniform of them (raw * 2^-32 + 2^-33, so raw 0 is 2^-33 and raw 2^32 - 1 is 1.0).

What the fixture pins: the oracle's restatement of each function, every row, bit for bit (tests/test_ref_shade_pins.py).
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF", "/root/reference")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
UNIFORM_COLUMNS = {1: (11, 13), 3: (19, 21), 5: (9, 11), 12: (0, 2)}   # function id -> the columns that hold raw draws


def make(out_path):
    import shade_scenes as ss
    if not os.path.isdir(REF):
        raise SystemExit(f"{REF} does not exist: the fixture can only be regenerated where the reference is present")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "_ref_shade", f"REF={REF}"], stdout=subprocess.DEVNULL)
    ref = os.path.join(ROOT, "oracle", "_ref")
    tables = ss.shade_tables()
    src, dst = os.path.join(ref, "shade.in.bin"), os.path.join(ref, "shade.out.bin")
    with open(src, "wb") as f:
        for func, rows in tables.items():
            rows = rows.copy()
            if func in UNIFORM_COLUMNS:
                a, b = UNIFORM_COLUMNS[func]
                rows[:, a:b] = ss.uniform_of(rows[:, a:b]).view(np.uint32)
            f.write(np.array([func, len(rows), ss.WORDS_IN[func], ss.WORDS_OUT[func]], "<i4").tobytes())
            f.write(rows.astype("<u4").tobytes())
    subprocess.check_call([os.path.join(ref, "ref_shade"), src, dst])
    b = open(dst, "rb").read()
    off = 0
    store = {}
    for func, rows in tables.items():
        hd = np.frombuffer(b, "<i4", 4, off)
        assert hd.tolist() == [func, len(rows), ss.WORDS_IN[func], ss.WORDS_OUT[func]], hd
        out = np.frombuffer(b, "<u4", len(rows) * ss.WORDS_OUT[func], off + 16).reshape(len(rows), -1).copy()
        off += 16 + out.nbytes
        store["in_" + ss.FUNCTIONS[func]], store["out_" + ss.FUNCTIONS[func]] = rows, out
        nan = int(np.isnan(out.view(np.float32)).any(axis=1).sum())
        print(f"{ss.FUNCTIONS[func]:22s} {len(rows):5d} rows, {nan:4d} with a NaN output")
    assert off == len(b)
    ss.save_npz(out_path, store)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    make(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ref_shade_fixture.npz"))
