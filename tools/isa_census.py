#!/usr/bin/env python3
"""Static instruction census of k_paths by source region (profiles/r05_adv_census.md, profiles/rr_chain.md).

Builds the device code with -DRT_ISA_MARKS (rt_device.h: RT_MARK emits assembler COMMENTS, no instruction), takes the
assembly of one k_paths instantiation and counts vector instructions (by category), scalar instructions and branches per
region.  Regions follow the code layout (the compiler keeps the blocks in source order; instructions it moved across a
comment are counted where they landed), so the numbers are a map of where the block's instructions are, not a trace of
what a lane executes.

    tools/isa_census.py [mangled-name-prefix]      (default: the kernel of bench.py's frame, C2)
    tools/isa_census.py --region BEGIN END [mangled-name-prefix]
                                                   only what lies between RT_MARK(BEGIN) and RT_MARK(END), with its
                                                   instructions and basic blocks listed: "instructions per turn" of a loop
                                                   that sits between two marks, e.g. --region adv.rr.begin adv.rr.end
    tools/isa_census.py --asm FILE ...             count in an assembly file that is already there (one built with
                                                   -DRT_ISA_MARKS and this file's FLAGS) instead of compiling
"""
import collections
import os
import re
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rtcuda_amd", "csrc")
FLAGS = "--offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -fno-fast-math -fno-slp-vectorize -fPIC -Wno-unused-function -Wno-unused-result".split()
DEFAULT = "_Z7k_pathsI14PathsChunkedBgLb1ELb1ELi4ELb0ELb0ELb1EE"   # k_paths<PathsChunkedBg, true, true, 4, false, false, true>

CATS = [
    ("int xor/shift/add/logic (XORWOW, bit tricks, addresses)", r"^v_(xor|lshlrev|lshrrev|ashrrev|add_u32|sub_u32|subrev_u32|add3_u32|lshl_add_u32|xad_u32|and|or|or3|and_or|bfe|bfi|not|mul_u32_u24|mul_lo_u32|mad_u32_u24|mad_u64_u32|mul_hi_u32|add_co|addc_co|sub_co|subb_co|lshl_or|alignbit|perm|min_u32|max_u32|min_i32|max_i32|add_lshl|xor3|mbcnt|bcnt)"),
    ("division / sqrt expansion (div_scale, div_fmas, div_fixup, rcp, rsq, sqrt, ldexp, frexp)", r"^v_(div_scale|div_fmas|div_fixup|rcp|rsq|sqrt|ldexp|frexp)"),
    ("fma (incl. the expansions' Newton steps)", r"^v_(fma_f32|fmac_f32|fmaak|fmamk)"),
    ("mul / add / sub f32", r"^v_(mul_f32|add_f32|sub_f32|subrev_f32|mul_legacy)"),
    ("packed f32", r"^v_pk_"),
    ("min / max / med f32", r"^v_(min|max|med)3?_(f32|num_f32)"),
    ("compare", r"^v_cmp"),
    ("select (cndmask)", r"^v_cndmask"),
    ("move / readlane / writelane", r"^v_(mov|readlane|writelane|readfirstlane|swap|accvgpr)"),
    ("convert / floor / fract / trunc", r"^v_(cvt|floor|fract|trunc|rndne|ceil)"),
]
SKIP = ("VALU", "v_mov", "LDS", "VMEM", "scalar", "branches", "s_waitcnt")
BRANCH = ("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_call")


def is_label(t):
    return t.split(";")[0].strip().endswith(":")


def count(d, op):
    """One instruction into a region's counter.  `scalar` holds the s_ instructions other than branches and s_waitcnt."""
    if op.startswith("v_"):
        cat = next((name for name, pat in CATS if re.match(pat, op)), "other vector: " + op)
        d["VALU"] += 1
        d[cat] += 1
        if op.startswith("v_mov"):
            d["v_mov"] += 1
    elif op.startswith("ds_"):
        d["LDS"] += 1
    elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        d["VMEM"] += 1
    elif op.startswith(BRANCH):
        d["branches"] += 1
    elif op.startswith("s_waitcnt"):
        d["s_waitcnt"] += 1
    elif op.startswith("s_"):
        d["scalar"] += 1


def head(d):
    return (f"VALU {d['VALU']} (v_mov {d['v_mov']}), scalar {d['scalar']}, branches {d['branches']}, LDS {d['LDS']}, VMEM {d['VMEM']}, "
            f"s_waitcnt {d['s_waitcnt']}")


def main():
    args = sys.argv[1:]
    asm, region_only = None, None
    while args and args[0].startswith("--"):
        if args[0] == "--asm":
            asm, args = args[1], args[2:]
        elif args[0] == "--region":
            region_only, args = (args[1], args[2]), args[3:]
        else:
            sys.exit(__doc__)
    want = args[0] if args else DEFAULT
    if asm is None:
        asm = "/tmp/rt_isa_census.s"
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + ["-DRT_ISA_MARKS", "--cuda-device-only", "-S", "-o", asm,
                                                                  os.path.join(CSRC, "rtcuda_amd.hip")], stderr=subprocess.DEVNULL)
    lines = open(asm).read().splitlines()
    start = next((i for i, ln in enumerate(lines) if ln.startswith(want) and ":" in ln.split(";")[0]), None)
    if start is None:
        sys.exit(f"no function whose name starts with {want} in {asm}")
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    print(f"function {want}: assembly lines {start}-{end}")
    if region_only:
        return one_region(lines[start:end], *region_only)
    region = "prologue"
    per, order = {}, []
    for ln in lines[start:end]:
        t = ln.strip()
        m = re.match(r"; RT_MARK (\S+)", t)
        if m:
            region = m.group(1)
            continue
        if not t or t.startswith(";") or t.startswith(".") or is_label(t):
            continue
        d = per.setdefault(region, collections.Counter())
        if region not in order:
            order.append(region)
        count(d, t.split()[0])
    tot = collections.Counter()
    for r in order:
        d = per[r]
        tot.update(d)
        print(f"\n## {r}: {head(d)}")
        for k, v in sorted(d.items(), key=lambda kv: -kv[1]):
            if k not in SKIP:
                print(f"    {v:5d}  {k}")
    print(f"\n## whole kernel: {head(tot)}")
    for k, v in sorted(tot.items(), key=lambda kv: -kv[1]):
        if k not in SKIP:
            print(f"    {v:5d}  {k}")


def one_region(body, begin, end):
    """Every stretch between RT_MARK(begin) and RT_MARK(end) (an inlined function's marks may occur more than once): its basic
    blocks with their instructions, and the counts per block and for the stretch."""
    found, inside = 0, False
    for ln in body:
        t = ln.strip()
        m = re.match(r"; RT_MARK (\S+)", t)
        if m:
            if m.group(1) == begin:
                inside, found = True, found + 1
                blocks, label = [], "(falls in)"
                cur = collections.Counter()
                text = []
            elif m.group(1) == end and inside:
                inside = False
                blocks.append((label, cur, text))
                blocks = [b for b in blocks if sum(b[1].values())]
                tot = collections.Counter()
                print(f"\n## {begin} .. {end}, occurrence {found}: {len(blocks)} basic block(s)")
                for lab, d, tx in blocks:
                    tot.update(d)
                    print(f"\n  block {lab}  {head(d)}")
                    for x in tx:
                        print("      " + x)
                print(f"\n  all blocks: {sum(tot[k] for k in ('VALU', 'scalar', 'branches', 'LDS', 'VMEM'))} instructions = {head(tot)}")
            continue
        fall = re.match(r"; (%bb\.\d+):", t)   # (a block that is only fallen into has no label of its own)
        if not inside or not t or (t.startswith(";") and not fall) or (t.startswith(".") and not is_label(t)):
            continue
        if fall or is_label(t):
            blocks.append((label, cur, text))
            label, cur, text = fall.group(1) if fall else t.split(";")[0].strip(), collections.Counter(), []
            continue
        count(cur, t.split()[0])
        text.append(t.split(";")[0].rstrip())
    if not found:
        sys.exit(f"no RT_MARK {begin} in this function")


if __name__ == "__main__":
    main()
