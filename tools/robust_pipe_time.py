"""Weighted build and GN pass of the two robust build modes (kb_set_robust_build) beside their unweighted twins, at a
synthetic config (default configs[3], 8 cameras x 2000 frames), per-corner invR + Huber(2) as tools/robust_time.py.

Four handles over the same problem:
  general   weighted, KB_ROBUST_BUILD_GENERAL: k_build<.., WT = true>, GN through the general five-launch pass
  pipe      weighted, KB_ROBUST_BUILD_PIPE: k_buildp<.., WT = true>, GN fused
  default   unweighted: k_buildp
  k_build   unweighted with KB_BUILD_PIPE=0: k_build

--mode profile (run it under one `rocprofv3 --kernel-trace --stats --output-format csv`): after one warm-up of every
  handle, `--rounds` alternating rounds; in a round every handle runs `--iterations` LM iterations (the GNF = false
  build kernels) and `--iterations` GN passes (pipe / default: kb_run_gn_iterations, the GNF = true kernels; general:
  kb_optimize with the GN policy), convergence tests off.  The host sleeps before each round, so the rounds are
  separated by gaps in the trace.
--trace FILE: summarise the kernel trace CSV of such a run (no GPU needed): per build kernel and round the median over
  the active launches (a launch that returns at its gate takes a few microseconds: active = at least half the longest),
  then over the rounds median, min, max, and for each weighted k_buildp against the weighted k_build whether the
  medians differ by more than the sum of the two ranges.
--mode rate (a plain run, no profiler): `--rounds` alternating rounds of
  pipe / default  GN iterations per second through kb_gn_prepare + kb_gn_launch, as bench.py times the unweighted loop
  general         host wall time per GN pass of kb_optimize with the GN policy (the general pass; polls included)
  with the same verdict rule between pipe and general.
Prints one JSON line."""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HANDLES = ("general", "pipe", "default", "k_build")


def make_handles(a):
    import numpy as np

    from kalibr_amd import capi, synth
    p = synth.make_config(a.config, **({"n_frames": a.frames} if a.frames else {}))
    rng = np.random.default_rng(1)
    n = p.n_corners
    s1, s2, th = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n), rng.uniform(0.2, 1.3, n)
    c, s = np.cos(th), np.sin(th)
    ia, ib = 1.0 / (s1 * s1), 1.0 / (s2 * s2)
    invR = np.stack([ia * c * c + ib * s * s, (ia - ib) * c * s, ia * s * s + ib * c * c], axis=1)
    hs = {}
    for name in HANDLES:
        if name == "k_build":
            os.environ["KB_BUILD_PIPE"] = "0"  # read by kb_create
        else:
            os.environ.pop("KB_BUILD_PIPE", None)
        g = capi.Solver(p)
        if name in ("general", "pipe"):
            g.set_robust_build(name)
            g.set_mestimator("huber", 2.0)
            g.set_corner_invR(invR)
        hs[name] = g
    os.environ.pop("KB_BUILD_PIPE", None)
    return p, hs


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=[round(x, 4) for x in v])


def differ(x, y):
    """the medians differ by more than the sum of the two ranges"""
    return abs(x["median"] - y["median"]) > (x["max"] - x["min"]) + (y["max"] - y["min"])


def gn_general(g, p, n):
    g.set_state(p.state_init)
    t0 = time.perf_counter()
    res = g.optimize(policy="gn", max_iterations=n, eps_x=-1.0, eps_j=-1.0, sync_every=8, use_graph=True)
    return time.perf_counter() - t0, res


def run_profile(a):
    p, hs = make_handles(a)
    out = dict(mode="profile", config=a.config, n_corners=int(p.n_corners), iterations=a.iterations, rounds=a.rounds,
               kernels={k: g.build_kernel_name() for k, g in hs.items()})
    for rnd in range(a.rounds + 1):  # round 0: the warm-up (graph captures)
        time.sleep(a.gap_ms / 1e3)
        for name, g in hs.items():
            g.set_state(p.state_init)
            res = g.optimize(policy="lm", lambda0=10.0, max_iterations=a.iterations, eps_x=-1.0, eps_j=-1.0, sync_every=8,
                             use_graph=True)
            out.setdefault("lm_passes", {})[name] = res["passes"]
            if name == "general":
                gn_general(g, p, a.iterations)
            else:
                g.set_state(p.state_init)
                g.run_gn(a.iterations)
    for g in hs.values():
        g.close()
    print(json.dumps(out))


def run_rate(a):
    p, hs = make_handles(a)
    hs.pop("k_build").close()
    out = dict(mode="rate", config=a.config, n_corners=int(p.n_corners), steps=a.steps, rounds=a.rounds)
    it_s = {"pipe": [], "default": []}
    ms_pass = {"pipe": [], "default": [], "general": []}
    info = {}
    for rnd in range(a.rounds + 1):  # round 0: the warm-up
        for name in ("pipe", "general", "default"):
            g = hs[name]
            if name == "general":
                dt, res = gn_general(g, p, a.steps)
                v = 1e3 * dt / max(res["passes"], 1)
                info[name] = dict(passes=res["passes"], iterations=res["iterations"], J_final=res["J_final"])
                if rnd:
                    ms_pass[name].append(v)
                continue
            g.set_state(p.state_init)
            graphed = g.gn_prepare(a.steps)
            sec = g.gn_launch(a.steps)
            info[name] = dict(graphed=bool(graphed), J_after=g.eval_cost())
            if rnd:
                it_s[name].append(a.steps / sec)
                ms_pass[name].append(1e3 * sec / a.steps)
    out["gn_iterations_per_s"] = {k: spread(v) for k, v in it_s.items()}
    out["ms_per_gn_pass"] = {k: spread(v) for k, v in ms_pass.items()}
    out["info"] = info
    x, y = out["ms_per_gn_pass"]["pipe"], out["ms_per_gn_pass"]["general"]
    out["pipe_vs_general"] = dict(ratio=y["median"] / x["median"], differ_by_more_than_the_ranges=differ(x, y),
                                  pipe_faster=differ(x, y) and x["median"] < y["median"])
    for g in hs.values():
        g.close()
    print(json.dumps(out))


def summarise(a):
    rows = []
    with open(a.trace, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"\bk_build\w*<[^>]*>", r["Kernel_Name"])
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), m.group(0) if m else ""))
    rows.sort()
    rounds, last = [], None
    for s, e, n in rows:  # a new round after every host sleep (a gap of at least half of it)
        if last is None or s - last > 0.5e6 * a.gap_ms:
            rounds.append([])
        last = e
        if n:
            rounds[-1].append((n, (e - s) / 1e3))
    rounds = [r for r in rounds if r][-a.rounds:]  # the warm-up round (and the set-up before it) dropped
    names = sorted(set(n for r in rounds for n, _ in r))
    out = dict(rounds=len(rounds), kernels={})
    for n in names:
        meds, act, tot = [], 0, 0
        for r in rounds:
            d = [us for k, us in r if k == n]
            if not d:
                continue
            live = [us for us in d if us >= 0.5 * max(d)]
            meds.append(statistics.median(live))
            act += len(live)
            tot += len(d)
        out["kernels"][n] = dict(us=spread(meds), active_launches=act, launches=tot)
    ker = out["kernels"]
    ref = [n for n in names if re.match(r"k_build<.*, true>$", n)]
    if len(ref) == 1:
        for n in names:
            if re.match(r"k_buildp<.*, true>$", n):
                out.setdefault("against_weighted_k_build", {})[n] = dict(
                    ratio=ker[ref[0]]["us"]["median"] / ker[n]["us"]["median"],
                    differ_by_more_than_the_ranges=differ(ker[n]["us"], ker[ref[0]]["us"]),
                    faster=differ(ker[n]["us"], ker[ref[0]]["us"]) and ker[n]["us"]["median"] < ker[ref[0]]["us"]["median"])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("profile", "rate"), default="rate")
    ap.add_argument("--config", type=int, default=4, help="synth.make_config index (4: configs[3], C = 106, F = 2000)")
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=10, help="profile: LM iterations and GN passes per handle and round")
    ap.add_argument("--steps", type=int, default=200, help="rate: GN passes per timed run")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gap-ms", type=float, default=300.0, help="profile: host sleep before each round")
    ap.add_argument("--trace", help="kernel trace csv of a profiled run to summarise")
    a = ap.parse_args()
    if a.trace:
        summarise(a)
    elif a.mode == "profile":
        run_profile(a)
    else:
        run_rate(a)


if __name__ == "__main__":
    main()
