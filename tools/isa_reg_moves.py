#!/usr/bin/env python3
"""Register-file copies in the build kernels, read from the compiled ISA (CPU only, no GPU needed).

A kernel that uses AGPRs has its register budget split between the architectural and the accumulation file.  Values
that do not fit the architectural half are parked in AGPRs and fetched back with v_accvgpr_write_b32 /
v_accvgpr_read_b32: each one a full VALU issue slot, none of them counted by the resource report's "VGPR spill".  For
every k_buildp / k_build instantiation of a build unit this prints the registers and scratch the assembler reports, and
the number of v_accvgpr_*, v_readlane / v_writelane and all instructions in the whole kernel and inside the view loop:
the smallest loop (a label and a later branch back to it) that contains every v_mfma_f64_4x4x4 of the kernel, or every
v_mfma_f64_16x16x4 where the kernel has no 4x4x4 (k_build).

  python tools/isa_reg_moves.py kalibr_amd/csrc/kb_build_tu.hip -DKB_TU_ID=0
  python tools/isa_reg_moves.py kalibr_amd/csrc/kb_build_tu.hip -DKB_TU_ID=0 -DKB_SYRK_DPP --kernel 'k_buildp<7, true'
  python tools/isa_reg_moves.py --asm saved.s
"""
import argparse
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_load_rounds import compile_asm, demangle, kernels  # noqa: E402

INSTR = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+([A-Za-z_.$][\w.$]*)")
CLASSES = (("accvgpr", re.compile(r"^v_accvgpr_")),
           ("lane", re.compile(r"^v_(readlane|writelane)_")),
           ("mfma", re.compile(r"^v_mfma_")),
           ("valu", re.compile(r"^v_")),
           ("salu", re.compile(r"^s_")),
           ("lds", re.compile(r"^ds_")),
           ("vmem", re.compile(r"^(global|buffer|flat|scratch)_")))
META = (("vgprs", re.compile(r"^;\s*NumVgprs:\s*(\d+)")), ("agprs", re.compile(r"^;\s*NumAgprs:\s*(\d+)")),
        ("scratch", re.compile(r"^;\s*ScratchSize:\s*(\d+)")), ("occupancy", re.compile(r"^;\s*Occupancy:\s*(\d+)")))


def opcode(line):
    """the instruction mnemonic of an assembly line, or None (labels, directives, comments, blank lines)"""
    m = INSTR.match(line.split(";")[0])
    return m.group(1) if m else None


def count(lines, lo, hi):
    """{class: instructions} of lines[lo:hi]; "all" counts every instruction, "valu" every v_* one (the copies, the
    lane moves and the MFMAs included)"""
    out = {k: 0 for k, _ in CLASSES}
    out["all"] = 0
    for i in range(lo, hi):
        op = opcode(lines[i])
        if not op:
            continue
        out["all"] += 1
        for k, rx in CLASSES:
            if rx.match(op):
                out[k] += 1
    return out


def loops(lines, lo, hi):
    """[(label line index, branch line index)] of every backward branch in lines[lo:hi]"""
    at, out = {}, []
    for i in range(lo, hi):
        m = LABEL.match(lines[i])
        if m:
            at[m.group(1)] = i
            continue
        m = BRANCH.match(lines[i])
        if m and m.group(1) in at:
            out.append((at[m.group(1)], i))
    return out


def mfma_loop(lines, lo, hi):
    """(first, end) line indices of the smallest loop holding every v_mfma_f64_4x4x4 (else every 16x16x4) of
    lines[lo:hi], the opcode it went by and their number; the loop is None where there is none"""
    for pat in ("v_mfma_f64_4x4x4", "v_mfma_f64_16x16x4"):
        at = [i for i in range(lo, hi) if (opcode(lines[i]) or "").startswith(pat)]
        if at:
            fits = [(b - a, a, b) for a, b in loops(lines, lo, hi) if a <= at[0] and at[-1] <= b]
            if not fits:
                return None, pat, len(at)
            _, a, b = min(fits)
            return (a, b + 1), pat, len(at)
    return None, None, 0


def metadata(lines, end):
    """the assembler's register / scratch figures in the comment block that follows a kernel body"""
    out = {}
    for i in range(end, min(len(lines), end + 60)):
        for k, rx in META:
            m = rx.match(lines[i].strip())
            if m and k not in out:
                out[k] = int(m.group(1))
    return out


def report(name, lines, lo, hi, fh=sys.stdout):
    md = metadata(lines, hi)
    whole = count(lines, lo, hi)
    span, pat, n = mfma_loop(lines, lo, hi)
    print("== %s" % name, file=fh)
    print("  VGPRs %s  AGPRs %s  scratch %s B  occupancy %s" % tuple(md.get(k, "-") for k, _ in META[:3] + META[3:]), file=fh)
    fmt = "  %-11s %5d instructions: %4d v_accvgpr_*, %3d v_readlane/v_writelane, %4d MFMA, %5d VALU in all, %4d scalar, %4d LDS, %3d memory"
    keys = ("all", "accvgpr", "lane", "mfma", "valu", "salu", "lds", "vmem")
    print(fmt % (("whole kernel",) + tuple(whole[k] for k in keys)), file=fh)
    if span:
        inner = count(lines, span[0], span[1])
        print(fmt % (("view loop",) + tuple(inner[k] for k in keys)), file=fh)
        print("              (lines %d-%d, the smallest loop with all %d %s)" % (span[0] + 1, span[1], n, pat), file=fh)
    elif pat:
        print("  no loop holds all %d %s" % (n, pat), file=fh)
    return md, whole, (count(lines, span[0], span[1]) if span else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src", nargs="?", help="translation unit (.hip); omitted with --asm")
    ap.add_argument("--kernel", action="append", default=[], help="substring of the demangled kernel name "
                    "(default: k_buildp< and k_build<)")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--keep", help="keep the compiled assembly at this path")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="preprocessor definitions")
    a, extra = ap.parse_known_args()
    defines = ["-D" + x for x in a.defines] + [x for x in extra if x.startswith("-D")]
    path = a.asm
    if not path:
        if not a.src:
            ap.error("a translation unit or --asm is needed")
        path = a.keep or os.path.join(tempfile.mkdtemp(prefix="isa_"), "tu.s")
        compile_asm(a.src, defines, path)
    with open(path) as fh:
        lines = fh.read().split("\n")
    spans = kernels(lines)
    dm = demangle(list(spans))
    want = a.kernel or ["k_buildp<", "k_build<"]
    hits = sorted((s for s in spans if any(w in dm[s] or w in s for w in want)), key=lambda s: dm[s])
    if not hits:
        print("no kernel matches %r" % want, file=sys.stderr)
        return 1
    for s in hits:
        name = re.sub(r"^void (?:\(anonymous namespace\)::)?(?:kb::)?", "", dm[s]).split("(")[0]
        report(name, lines, spans[s][0], spans[s][1])
    return 0


if __name__ == "__main__":
    sys.exit(main())
