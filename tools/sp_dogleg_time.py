"""Dog-leg pass cost on the spline path at configs[4] (synth.make_spline_config: C = 37, K = 3001, 1001 nodes) next to
its LM pass (kb_sp_optimize policy 0) from the same state.

A warm-up run of each policy, then --runs timed runs each from the initial state.  Dog-leg passes are classed by what
they launched, from the trace alone: "built+solved" (build, SD reduction, GN solve, step dots, step, cost: three
read-backs), "built" (the SD branch was taken: no solve, two read-backs), "reused" (after a rejected step: step and
cost alone, one read-back; "reused+solved" where such a pass is the first to need the GN step).  Per class the median
host wall time per pass (kb_sp_diag_dogleg_pass_ms: the loop body, read-backs included); for LM the run's wall time
over its passes.  --past-convergence sets both thresholds to -1 so that the loop runs all --iterations iterations: at
the noise floor steps are rejected, which gives reused passes.  Prints one JSON line.

Under `rocprofv3 --kernel-trace --stats` the same run leaves the device times of k_sp_dl_sd / k_sp_dl_sum /
k_sp_dl_dots / k_sp_dl_step by name; --stats FILE summarises that CSV (no GPU needed): calls, average and total per
kernel, the new kernels first."""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def classes(res):
    dt, tr = res["dogleg_trace"], res["trace"]
    out, held = [], False
    for k in range(len(dt)):
        built = k == 0 or tr[k - 1, 3] == 1
        if built:
            held = False
        solved = not held and dt[k, 5] != 0.0 or dt[k, 1] < 0
        held = held or solved
        out.append(("built" if built else "reused") + ("+solved" if solved else ""))
    return out


def run(a):
    from kalibr_amd import capi, synth
    p = synth.make_spline_config()
    g = capi.SplineSolver(p)
    L = capi.lib()
    L.kb_sp_diag_dogleg_pass_ms.argtypes = [C.c_void_p, capi.dp, C.c_int]
    opt = dict(max_iterations=a.iterations, eps_x=a.eps_x, eps_j=a.eps_j)
    out = dict(C=g.C, K=g.K, iterations=a.iterations, delta_init=a.delta_init, runs=a.runs)
    per, lm_ms, res = {}, [], None
    for k in range(a.runs + 1):  # run 0 warms up
        g.set_state(p.state_init)
        res = g.optimize(policy="dogleg", delta_init=a.delta_init, **opt)
        ms = capi.np.zeros(len(res["trace"]))
        n = L.kb_sp_diag_dogleg_pass_ms(g.h, capi._d(ms), ms.size)
        assert n == ms.size
        if k:
            for c, v in zip(classes(res), ms):
                per.setdefault(c, []).append(float(v))
    out["dogleg"] = dict(steps="".join("SGD"[int(t)] if t >= 0 else "x" for t in res["dogleg_trace"][:, 1]),
                         accepted="".join(str(int(x)) for x in res["trace"][:, 3]), J_final=res["J_final"],
                         pass_ms_median={c: round(statistics.median(v), 4) for c, v in sorted(per.items())},
                         passes={c: len(v) // a.runs for c, v in sorted(per.items())})
    for k in range(a.runs + 1):
        g.set_state(p.state_init)
        t0 = time.perf_counter()
        res = g.optimize(policy="lm", lambda0=10.0, **opt)
        dt = time.perf_counter() - t0
        if k:
            lm_ms.append(1e3 * dt / max(res["passes"], 1))
    out["lm"] = dict(passes=res["passes"], accepted="".join(str(int(x)) for x in res["trace"][:, 3]),
                     J_final=res["J_final"], pass_ms_median=round(statistics.median(lm_ms), 4))
    print(json.dumps(out))


def summarise(a):
    rows = []
    with open(a.stats, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"].split("(")[0].replace("void ", "").replace("ksp::", "")
            rows.append(dict(kernel=name, calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 2),
                             total_us=round(float(r["TotalDurationNs"]) / 1e3, 1)))
    rows.sort(key=lambda r: (not r["kernel"].startswith("k_sp_dl"), -r["total_us"]))
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--delta-init", type=float, default=0.01)
    ap.add_argument("--eps-x", type=float, default=1e-3)
    ap.add_argument("--eps-j", type=float, default=1e-3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--past-convergence", action="store_true")
    ap.add_argument("--stats", help="kernel stats csv of a profiled run to summarise")
    a = ap.parse_args()
    if a.past_convergence:
        a.eps_x = a.eps_j = -1.0
    summarise(a) if a.stats else run(a)


if __name__ == "__main__":
    main()
