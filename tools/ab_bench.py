#!/usr/bin/env python3
"""A/B of library variants on one bench.py line: plain `python bench.py <line>` runs, alternating between the
variants round by round in one job on one machine, each in a fresh process under its own time limit.  The first
variant is the yardstick (the parent commit's library, built from the parent's sources as libkalibr_hip_<name>.so);
"main" names the tree's default library, every other name a KB_VARIANT_LIB (kalibr_amd/build.py build_variant).

A difference counts when it exceeds the sum of the two run-to-run ranges (max - min of each side's values).

  python tools/ab_bench.py --line "--config 4" --variants parent main --rounds 5 --out ab_c4.json
  python tools/ab_bench.py --line "--config 4" --variants parent main --bitwise 20    # states after 20 passes

The job stops at the first run that fails or runs into its time limit (nothing is started after it).
"""
import argparse
import json
import os
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(variant, line, limit, extra=()):
    env = dict(os.environ)
    env.pop("KB_VARIANT_LIB", None)
    if variant != "main":
        env["KB_VARIANT_LIB"] = variant
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + shlex.split(line) + list(extra)
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        raise SystemExit("%s: bench.py %s ended with %d" % (variant, line, r.returncode))
    return json.loads(r.stdout.strip().split("\n")[-1])


def side(vals):
    s = sorted(vals)
    return {"values": vals, "mean": sum(vals) / len(vals), "median": s[len(s) // 2], "spread": s[-1] - s[0]}


def compare(base, new):
    gain = new["mean"] - base["mean"]
    bar = base["spread"] + new["spread"]
    return {"gain": gain, "gain_rel": gain / base["mean"], "bar": bar, "counts_as_gain": gain > bar,
            "counts_as_loss": -gain > bar}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--line", default="--config 4", help="bench.py arguments of the line")
    ap.add_argument("--variants", nargs="+", default=["parent", "main"], help="the first one is the yardstick")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0, help="time limit of one bench.py run, seconds")
    ap.add_argument("--bitwise", type=int, default=0, metavar="PASSES",
                    help="instead of timing: the state after PASSES timed passes of every variant against the first")
    ap.add_argument("--out", help="write the result JSON here")
    a = ap.parse_args()
    if a.bitwise:
        import numpy as np
        ref = None
        for v in a.variants:
            d = tempfile.mkdtemp(prefix="ab_dump_")
            run_bench(v, a.line, a.limit, ["--steps", str(a.bitwise), "--dump-outputs", d])
            st = np.load(os.path.join(d, "state.npy"))
            if ref is None:
                ref = st
                continue
            same = st.shape == ref.shape and st.tobytes() == ref.tobytes()
            ndiff = int((st.view(np.uint64) != ref.view(np.uint64)).sum()) if st.shape == ref.shape else -1
            print("bench.py %s: state.npy after %d passes, %s vs %s: %s %d %s" % (a.line, a.bitwise, a.variants[0], v, same,
                                                                                 ndiff, st.shape), flush=True)
            if not same:
                return 1
        return 0
    vals = {v: [] for v in a.variants}
    for rnd in range(a.rounds):
        for v in a.variants:
            vals[v].append(float(run_bench(v, a.line, a.limit)["value"]))
            print("round %d %-12s %.1f" % (rnd + 1, v, vals[v][-1]), flush=True)
    res = {"runs": "plain python bench.py %s, alternating in one job on one machine" % a.line, "unit": "GN iterations/s"}
    for v in a.variants:
        res[v] = side(vals[v])
    for v in a.variants[1:]:
        res["gain_" + v] = compare(res[a.variants[0]], res[v])
    res["note"] = "%s = the yardstick; main = this tree's default library; bar = the sum of the two run-to-run ranges" % a.variants[0]
    for v in a.variants[1:]:
        g = res["gain_" + v]
        print("%s vs %s: %+.1f (%+.2f %%), bar %.1f, gain %s loss %s" % (v, a.variants[0], g["gain"], 100 * g["gain_rel"], g["bar"],
                                                                         g["counts_as_gain"], g["counts_as_loss"]))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
