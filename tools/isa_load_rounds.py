#!/usr/bin/env python3
"""Load rounds at the head of a kernel, read from the compiled ISA (CPU only, no GPU needed).

Compiles one translation unit device-only to gfx950 assembly with build.py's flags, then, for every kernel whose
(demangled) name contains the given substring, prints the groups of global_load_* instructions up to the first
s_barrier (or --barriers N of them) and the s_waitcnt vmcnt(n) that ends each group, with the assembly line numbers.
A "round" is a set of loads in flight together: DESIGN.md section 3's rule (at most two dependent rounds per kernel)
can be checked in the time of one compile.  Only loads and waits are inspected.

  python tools/isa_load_rounds.py kalibr_amd/csrc/kb_capi.hip 'k_solve<0>' [--barriers 2]
  python tools/isa_load_rounds.py kalibr_amd/csrc/kb_build_tu.hip 'k_buildp<7, true, 1u, 12>' -DKB_TU_ID=0
  python tools/isa_load_rounds.py --asm saved.s k_colsumx        # an assembly file compiled earlier
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOAD = re.compile(r"^\s*(global_load_\w+|buffer_load_\w+|flat_load_\w+|scratch_load_\w+)\s+(.*?)\s*(?:;.*)?$")
WAIT = re.compile(r"^\s*s_waitcnt\b(.*?)\s*(?:;.*)?$")
VMCNT = re.compile(r"vmcnt\((\d+)\)")
LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")


def compile_asm(src, defines, out):
    from kalibr_amd import build
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [build.HIPCC] + flags + ["--cuda-device-only", "-S"] + list(defines) + ["-o", out, src]
    subprocess.run(cmd, check=True)


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        out = r.stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(lines):
    """{symbol: (first line index, end line index)} of every .amdhsa kernel body in the assembly."""
    kd = set(m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m)
    spans, cur = {}, None
    for i, l in enumerate(lines):
        m = LABEL.match(l)
        if m and m.group(1) in kd:
            cur = m.group(1)
            spans[cur] = [i, len(lines)]
        elif cur and re.match(r"\s*\.Lfunc_end", l):
            spans[cur][1] = i
            cur = None
    return spans


def rounds(lines, lo, hi, barriers):
    """[(loads [(line, text)], wait (line, text, n) | None, label)] up to the barriers-th s_barrier."""
    out, cur, nb = [], [], 0
    for i in range(lo, hi):
        l = lines[i]
        if re.match(r"\s*s_barrier\b", l):
            nb += 1
            out.append((cur, None, "s_barrier #%d (line %d)" % (nb, i + 1)))
            cur = []
            if nb >= barriers:
                return out
            continue
        if re.match(r"\s*s_endpgm\b", l) and not cur:
            continue
        m = LOAD.match(l)
        if m:
            cur.append((i + 1, m.group(1) + " " + m.group(2)))
            continue
        m = WAIT.match(l)
        if m:
            v = VMCNT.search(m.group(1))
            if v and cur:
                out.append((cur, (i + 1, "s_waitcnt" + m.group(1), int(v.group(1))), None))
                cur = []
            elif v:
                out.append(([], (i + 1, "s_waitcnt" + m.group(1), int(v.group(1))), None))
    if cur:
        out.append((cur, None, "end of kernel"))
    return out


def report(name, lines, lo, hi, barriers, verbose, fh):
    rs = rounds(lines, lo, hi, barriers)
    print("== %s  (lines %d-%d)" % (name, lo + 1, hi), file=fh)
    k = 0
    for loads, wait, label in rs:
        if loads:
            k += 1
            kinds = {}
            for _, t in loads:
                kinds[t.split()[0]] = kinds.get(t.split()[0], 0) + 1
            desc = ", ".join("%d %s" % (n, op) for op, n in sorted(kinds.items()))
            print("  round %2d: %3d loads, lines %d-%d (%s)" % (k, len(loads), loads[0][0], loads[-1][0], desc), file=fh)
            if verbose:
                for ln, t in loads:
                    print("      %7d  %s" % (ln, t), file=fh)
        if wait:
            tag = "ends it" if loads else "(no new load)"
            print("            line %d: %s  %s" % (wait[0], wait[1].strip(), tag), file=fh)
        if label:
            print("  -- %s" % label, file=fh)
    print("  %d load group(s) before the %s" % (k, "first barrier" if barriers == 1 else "barrier #%d" % barriers), file=fh)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src", nargs="?", help="translation unit (.hip); omitted with --asm")
    ap.add_argument("kernel", help="substring of the demangled (or mangled) kernel name")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--keep", help="keep the compiled assembly at this path")
    ap.add_argument("--barriers", type=int, default=1, help="stop at the N-th s_barrier (default 1)")
    ap.add_argument("-v", "--verbose", action="store_true", help="list every load")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="preprocessor definitions")
    a, extra = ap.parse_known_args()
    defines = ["-D" + x for x in a.defines] + [x for x in extra if x.startswith("-D")]
    if a.asm:
        path = a.asm
    else:
        if not a.src:
            ap.error("a translation unit or --asm is needed")
        path = a.keep or os.path.join(tempfile.mkdtemp(prefix="isa_"), "tu.s")
        compile_asm(a.src, defines, path)
    with open(path) as fh:
        lines = fh.read().split("\n")
    spans = kernels(lines)
    dm = demangle(list(spans))
    hits = [s for s in spans if a.kernel in dm[s] or a.kernel in s]
    if not hits:
        print("no kernel matches %r; kernels here:" % a.kernel, file=sys.stderr)
        for s in spans:
            print("  " + dm[s], file=sys.stderr)
        return 1
    for s in hits:
        report(dm[s], lines, spans[s][0], spans[s][1], a.barriers, a.verbose, sys.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
