#!/usr/bin/env python3
"""Records tests/golden/table_arg_messages.json: what the five ray-table entry points answer to the bad arguments of
tests/test_table_args_host.py (its BAD and PAIRS).  Needs no GPU.

The file pins the messages of the library BEFORE a change to the checks, so run it on the parent commit's build, not on the
one under test:

    make -C rtcuda_amd/csrc            (on the parent commit; keep the result as rtcuda_amd/librtcuda_amd_parent.so)
    RT_LIB_NAME=librtcuda_amd_parent.so python tests/golden/make_table_arg_messages.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_table_args_host as t  # noqa: E402
from rtcuda_amd import api  # noqa: E402


def main():
    L = api.lib()
    out = {}
    for entry in t.ENTRY_POINTS:
        out[entry] = {}
        for name, changed in t.cases(entry):
            rc, msg = t.call(L, entry, **changed)
            assert rc != 0 and msg.startswith(entry + ": "), (entry, name, rc, msg)
            out[entry][name] = msg
    with open(t.GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{t.GOLDEN}: {sum(len(v) for v in out.values())} messages of {api.LIB_PATH} (build {L.rt_build_id().decode()})")


if __name__ == "__main__":
    main()
