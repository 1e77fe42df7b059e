#!/usr/bin/env python3
"""Compare the device code of two builds, function by function.

    hipcc --offload-arch=gfx950 <the Makefile's FLAGS> --cuda-device-only -S -o A.s rtcuda_amd.hip     (one commit)
    hipcc ... -o B.s rtcuda_amd.hip                                                                    (another)
    python tools/device_code_diff.py A.s B.s [--rename OLD=NEW ...] [--demangled]

Both assembly files are split per function (from the function's label to its .Lfunc_end), comments and directives are
dropped, and local labels (.LBB..., .Ltmp...) are renumbered in order of appearance, so that what is left of a function is
its instructions and its branch structure.  Prints how many functions and lines were compared and every function that
differs, is missing from B or is new in B; exits 1 if any function differs or is missing (new ones alone are no failure).
--rename OLD=NEW (any number, applied in order): in the NAMES of A's functions every substring OLD becomes NEW before the two
files are matched, so that a kernel whose template parameters changed -- and with them its mangled name -- is compared body
against body with its successor.  The bodies are not touched.
--demangled: after the renames, the functions of both files are matched by their demangled names WITHOUT the parameter list
(c++filt -p: `k_paths<PathsBg, true, true, 4, false, false, true>`).  For a kernel whose parameter types re-mangle although they
did not change -- a parameter that became `typename BUILD::Src` is a substitution in the new name and spelt out in the old --
no substring rename of the whole mangled name exists; a rename of its head (`_Z10k_paths_bgI=_Z7k_pathsI7PathsBg`) is enough
here, since what follows the template arguments is dropped.  Two functions of one file with the same such name are an error.
It compares text: what the lines say is none of its business."""
import re
import subprocess
import sys

LOCAL = re.compile(r"\.L[A-Za-z_$][\w$.]*")


def functions(path):
    """{name: [normalised lines]} of every function (a .type NAME,@function whose label and .Lfunc_end follow)."""
    names, out, cur, body = set(), {}, None, None
    with open(path, errors="replace") as fh:
        lines = fh.read().splitlines()
    for l in lines:
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", l)
        if m:
            names.add(m.group(1))
    for l in lines:
        code = l.split(";", 1)[0].split("//", 1)[0].rstrip()
        s = code.strip()
        if cur is None:
            if s.endswith(":") and s[:-1] in names:
                cur, body = s[:-1], []
            continue
        if s.startswith(".Lfunc_end"):
            out[cur] = renumber(body)
            cur = None
            continue
        if not s or (s.startswith(".") and not s.endswith(":")):  # blank, or a directive (labels end with a colon)
            continue
        body.append(" ".join(s.split()))
    return out


def renumber(body):
    seen = {}

    def sub(m):
        return seen.setdefault(m.group(0), f".L{len(seen)}")

    return [LOCAL.sub(sub, l) for l in body]


def renamed(funcs, pairs):
    out = {}
    for name, body in funcs.items():
        for old, new in pairs:
            name = name.replace(old, new)
        if name in out:
            raise SystemExit(f"--rename maps two functions onto {name}")
        out[name] = body
    return out


def demangled(funcs):
    """The same functions under their demangled names without parameter lists (a name c++filt cannot read is kept)."""
    names = list(funcs)
    res = subprocess.run(["c++filt", "-p"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(res) == len(names)
    out = {}
    for old, new in zip(names, res):
        if new in out:
            raise SystemExit(f"--demangled maps two functions onto {new}")
        out[new] = funcs[old]
    return out


def main(argv):
    pairs = []
    by_demangled = "--demangled" in argv
    argv = [x for x in argv if x != "--demangled"]
    while "--rename" in argv:
        k = argv.index("--rename")
        stop = next((i for i in range(k + 1, len(argv)) if "=" not in argv[i]), len(argv))
        pairs += [tuple(x.split("=", 1)) for x in argv[k + 1:stop]]
        argv = argv[:k] + argv[stop:]
    if len(argv) != 3:
        print(__doc__)
        return 2
    a, b = renamed(functions(argv[1]), pairs), functions(argv[2])
    if by_demangled:
        a, b = demangled(a), demangled(b)
    differ = [n for n in a if n in b and a[n] != b[n]]
    missing = [n for n in a if n not in b]
    new = [n for n in b if n not in a]
    same = len(a) - len(differ) - len(missing)
    lines = sum(len(a[n]) for n in a if n in b)
    print(f"{len(a)} functions of {argv[1]} compared with {argv[2]}: {same} identical ({lines} instruction and label lines compared), "
          f"{len(differ)} differ, {len(missing)} missing, {len(new)} new")
    for what, names in (("differs", differ), ("missing", missing), ("new", new)):
        for n in names:
            extra = ""
            if what == "differs":
                k = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
                extra = f"  (first at line {k} of {len(a[n])} / {len(b[n])})"
            print(f"  {what}: {n}{extra}")
    return 1 if differ or missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
