"""Dog-leg pass cost at a synthetic config (default configs[3], 8 cameras x 2000 frames) next to the LM pass
(kb_optimize policy 0) from the same state.

Run mode (default): a warm-up run of each policy (captures the pass graphs), then one timed run each from the initial
state; prints one JSON line with the step / accept strings, the passes and the host wall time per pass (between the
call and its final stream sync: loop start, the host's polls every 8 passes and the gated-off passes of the last
batch included).  --past-convergence sets both convergence thresholds to -1, so the loop runs all --iterations
iterations: at the noise floor some steps are rejected, which gives passes that reuse the held system.  Under
`rocprofv3 --kernel-trace --output-format csv` the same run leaves a kernel trace.

--trace FILE: summarise such a kernel trace instead (no GPU needed): the dispatches of every run of each policy are
split into passes at the pass-end kernel (k_dl_policy / k_post); a pass whose longest kernel stayed under --idle-us is
idle (launched after the loop finished: every kernel returns at its gate), another one is built when its build kernel
ran longer than --built-us, else reused (dog-leg) / kept (LM: same system, new lambda).  Per class the median sum of
kernel durations per pass and the median duration of every kernel in a pass of that class."""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(a):
    from kalibr_amd import capi, synth
    p = synth.make_config(a.config, **({"n_frames": a.frames} if a.frames else {}))
    g = capi.Solver(p)
    out = dict(config=a.config, C=g.C, F=(g.ncols - g.C) // 6, max_iterations=a.iterations, delta_init=a.delta_init)
    for policy, kw in (("dogleg", dict(delta_init=a.delta_init)), ("lm", dict(lambda0=10.0))):
        for timed in (False, True):
            g.set_state(p.state_init)
            t0 = time.perf_counter()
            res = g.optimize(policy=policy, max_iterations=a.iterations, eps_x=a.eps_x, eps_j=a.eps_j, sync_every=8,
                             use_graph=True, **kw)
            dt = time.perf_counter() - t0
        o = dict(passes=res["passes"], iterations=res["iterations"], failed_iterations=res["failed_iterations"],
                 J_final=res["J_final"], graphed=res["graphed"], wall_ms_per_pass=1e3 * dt / max(res["passes"], 1),
                 accepted="".join(str(int(x)) for x in res["trace"][:, 3]))
        if policy == "dogleg":
            o["steps"] = "".join("SGD"[int(t)] if t >= 0 else "x" for t in res["dogleg_trace"][:, 1])
        out[policy] = o
    print(json.dumps(out))


def short(name):
    m = re.search(r"\bk_\w+", name)
    return m.group(0) if m else name.split("(")[0]


def summarise(a):
    rows = []
    with open(a.trace, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    out = {}
    for policy, end in (("dogleg", "k_dl_policy"), ("lm", "k_post")):
        # every run of the policy: the dispatches from a loop start (k_pol_init) on, if the run has `end` kernels
        runs = []
        for r in rows:
            if r[2] == "k_pol_init":
                runs.append([])
            elif runs:
                runs[-1].append(r)
        passes = []
        for x in runs:
            if not any(r[2] == end for r in x):
                continue
            acc = []
            for r in x:
                if not r[2].startswith("k_") or (r[2] in ("k_pre", "k_dl_init", "k_cost", "k_reduce_cost") and not acc):
                    continue
                acc.append(r)
                if r[2] == end:
                    passes.append(acc)
                    acc = []
        if not passes:
            continue
        classes = {}
        for ps in passes:
            build = sum((e - s) for s, e, n in ps if n.startswith("k_build"))
            live = max((e - s) for s, e, n in ps) > a.idle_us * 1e3
            if not live:
                key = "idle"  # passes after the loop finished (every kernel returns at its gate)
            elif policy == "dogleg":
                key = "built" if build > a.built_us * 1e3 else "reused"
            else:
                key = "built" if build > a.built_us * 1e3 else "kept"
            classes.setdefault(key, []).append(ps)
        o = {}
        for key, pl in classes.items():
            tot = [sum(e - s for s, e, n in ps) / 1e3 for ps in pl]
            span = [(ps[-1][1] - ps[0][0]) / 1e3 for ps in pl]
            per = {}
            for ps in pl:
                byk = {}
                for s, e, n in ps:
                    byk[n] = byk.get(n, 0.0) + (e - s) / 1e3
                for n, v in byk.items():
                    per.setdefault(n, []).append(v)
            o[key] = dict(passes=len(pl), kernel_us_median=statistics.median(tot), span_us_median=statistics.median(span),
                          kernels_us_median={n: round(statistics.median(v), 2) for n, v in sorted(per.items())})
        out[policy] = o
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=4, help="synth.make_config index (4: configs[3], C = 106, F = 2000)")
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--delta-init", type=float, default=1e-3)
    ap.add_argument("--eps-x", type=float, default=1e-12)
    ap.add_argument("--eps-j", type=float, default=1e-12)
    ap.add_argument("--trace", help="kernel trace csv of a profiled run to summarise")
    ap.add_argument("--built-us", type=float, default=20.0)
    ap.add_argument("--idle-us", type=float, default=8.0)
    ap.add_argument("--past-convergence", action="store_true")
    a = ap.parse_args()
    if a.past_convergence:
        a.eps_x = a.eps_j = -1.0
    summarise(a) if a.trace else run(a)


if __name__ == "__main__":
    main()
