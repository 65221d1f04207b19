#!/usr/bin/env python3
"""Compare two device assembly files function by function (CPU only, no GPU needed).

Each file is the output of `hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S` for one translation
unit (tools/isa_load_rounds.py --keep writes one).  A function's instruction stream is its lines between its label
and its .Lfunc_end, with comments and directives removed and the function number taken out of local labels
(.LBB12_3 -> .LBB_3).  Functions are matched by demangled name; a trailing template argument that is the default
of a parameter added later (`--drop-default ', false>'` turns `k_buildp<7, true, 1u, 12, false>` into
`k_buildp<7, true, 1u, 12>`) is dropped from the names of the second file, and from the mangled names inside both
streams, so that a new defaulted template parameter does not count as a difference.

--kernarg-shift SIZE:DELTA: the struct every kernel takes by value grew by DELTA bytes at its end (no field moved), so
the arguments after it and the hidden ones sit DELTA bytes later; their scalar loads (and the s_add_u32 that forms the
hidden arguments' address) are compared at the old offsets.

  python tools/asm_compare.py parent.s new.s [--drop-default ', false>'] [--kernarg-shift 0x600:0x70] [--list]
prints: functions in each, identical, different, only in one; exit status 1 when an instruction stream differs.
"""
import argparse
import re
import subprocess
import sys

LABEL = re.compile(r"^([A-Za-z_$][\w.$]*):")


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.split("\n")))


def functions(path):
    """{symbol: [normalized instruction lines]}"""
    with open(path) as fh:
        lines = fh.read().split("\n")
    funcs = set(m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", l) for l in lines) if m)
    out, cur = {}, None
    for l in lines:
        m = LABEL.match(l)
        if m and m.group(1) in funcs:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if re.match(r"\s*\.Lfunc_end", l):
            cur = None
            continue
        t = re.sub(r"\s*(;|//).*$", "", l).strip()
        if not t or t.startswith(".") and not LABEL.match(t) and not t.startswith(".LBB"):
            continue
        t = re.sub(r"\.LBB\d+_", ".LBB_", t)
        out[cur].append(t)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--drop-default", action="append", default=[],
                    help="demangled suffix of the second file's names to drop (repeatable; '<false>' drops a whole "
                         "argument list: a kernel that became a template)")
    ap.add_argument("--list", action="store_true", help="name every function, not only the counts")
    ap.add_argument("--kernarg-shift", default=None, metavar="SIZE:DELTA",
                    help="the by-value struct every kernel takes first grew from SIZE by DELTA bytes at its end: scalar "
                         "loads of the second file at offsets >= SIZE + DELTA (the arguments after it and the hidden "
                         "ones) are compared at offset - DELTA")
    a = ap.parse_args()
    fa, fb = functions(a.a), functions(a.b)
    if a.kernarg_shift:
        size, delta = (int(x, 0) for x in a.kernarg_shift.split(":"))

        def unshift(m):
            off = int(m.group(2), 16)
            hit = off >= size + delta and (m.group(1).startswith("s_load") or off < size + delta + 0x100)
            return m.group(1) + ("0x%x" % (off - delta) if hit else m.group(2))
        for s in fb:
            fb[s] = [re.sub(r"^((?:s_load_\w+ .*|s_add_u32 s\d+, s\d+), )(0x[0-9a-f]+)$", unshift, t) for t in fb[s]]
    da, db = demangle(list(fa)), demangle(list(fb))
    rename = {}  # mangled name of the second file -> the first file's
    by_dem_a = {v: k for k, v in da.items()}
    for dd in a.drop_default:
        for s, dn in list(db.items()):
            if dd in dn:
                short = dn.replace(dd, "" if dd.startswith("<") else ">" if dd.endswith(">") else "")
                if dd.startswith("<") and short.startswith("void "):  # a plain function's name has no return type
                    short = short[5:]
                if short in by_dem_a:
                    rename[s] = by_dem_a[short]
                    db[s] = short
    # a renamed symbol's mangled stem (without the leading _Z / trailing signature) inside instruction operands
    def norm(stream):
        out = []
        for t in stream:
            for new, old in rename.items():
                if new in t:
                    t = t.replace(new, old)
            out.append(t)
        return out
    A = {da[s]: fa[s] for s in fa}
    Bn = {db[s]: norm(fb[s]) for s in fb}
    same = sorted(n for n in A if n in Bn and A[n] == Bn[n])
    diff = sorted(n for n in A if n in Bn and A[n] != Bn[n])
    only_a = sorted(n for n in A if n not in Bn)
    only_b = sorted(n for n in Bn if n not in A)
    print("functions: %d | %d   identical %d   different %d   only in the first %d   only in the second %d"
          % (len(A), len(Bn), len(same), len(diff), len(only_a), len(only_b)))
    for tag, names in (("different", diff), ("only in the first", only_a), ("only in the second", only_b)):
        for n in names:
            print("  %s: %s" % (tag, n[:150]))
    if a.list:
        for n in same:
            print("  identical: %s  (%d instructions)" % (n[:150], len(A[n])))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
