#!/usr/bin/env python3
"""LDS round trips in front of global stores, read from the compiled ISA (CPU only, no GPU needed).

For every kernel whose (demangled) name contains the given substring: the groups of ds_read_* instructions that are in
flight together (a group ends at the first full `s_waitcnt lgkmcnt(0)` after its reads) and whose values go straight
to global memory (the next LDS / global-memory / barrier instruction after that wait is a global_store_*).  A group of
one read is a serial round trip: read, full wait, store, and only then the next read (DESIGN.md section 3 rule 1 on a
store path: a bounds check around a store swallows its load).  k_buildp's expanded partial-row store is such a path:
28 groups of one read before round 13, two groups (16 and 12 reads) after.

  python tools/isa_lds_store_rounds.py kalibr_amd/csrc/kb_build_tu.hip 'k_buildp<7, true, 1u, 12, false>' -DKB_TU_ID=0
  python tools/isa_lds_store_rounds.py --asm saved.s 'k_buildp<7, true, 1u, 12, false>'
"""
import argparse
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_load_rounds import compile_asm, demangle, kernels  # noqa: E402

DSREAD = re.compile(r"^\s*ds_read\w*\s")
MEM = re.compile(r"^\s*(ds_\w+|global_\w+|buffer_\w+|flat_\w+|scratch_\w+|s_barrier)\b")
FULLWAIT = re.compile(r"^\s*s_waitcnt\b.*lgkmcnt\(0\)")


def store_rounds(lines, lo, hi):
    """[(first read line, last read line, reads)] of the read groups whose full wait is followed by a global store"""
    out, cur, closed = [], [], None
    for i in range(lo, hi):
        l = lines[i]
        if DSREAD.match(l):
            closed = None
            cur.append(i + 1)
            continue
        if FULLWAIT.match(l):
            if cur:
                closed, cur = cur, []
            continue
        m = MEM.match(l)
        if m:
            if closed and m.group(1).startswith("global_store"):
                out.append((closed[0], closed[-1], len(closed)))
            closed = None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src", nargs="?", help="translation unit (.hip); omitted with --asm")
    ap.add_argument("kernel", help="substring of the demangled (or mangled) kernel name")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="preprocessor definitions")
    a, extra = ap.parse_known_args()
    defines = ["-D" + x for x in a.defines] + [x for x in extra if x.startswith("-D")]
    path = a.asm
    if not path:
        if not a.src:
            ap.error("a translation unit or --asm is needed")
        path = os.path.join(tempfile.mkdtemp(prefix="isa_"), "tu.s")
        compile_asm(a.src, defines, path)
    with open(path) as fh:
        lines = fh.read().split("\n")
    spans = kernels(lines)
    dm = demangle(list(spans))
    hits = [s for s in spans if a.kernel in dm[s] or a.kernel in s]
    if not hits:
        print("no kernel matches %r" % a.kernel, file=sys.stderr)
        return 1
    for s in hits:
        rs = store_rounds(lines, spans[s][0], spans[s][1])
        print("== %s" % dm[s])
        for first, last, n in rs:
            print("  lines %6d-%6d: %2d LDS read(s), full wait, global store" % (first, last, n))
        print("  %d read group(s) in front of global stores, %d of them a single read behind its own lgkmcnt(0); "
              "%d LDS reads in all" % (len(rs), sum(1 for r in rs if r[2] == 1), sum(r[2] for r in rs)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
