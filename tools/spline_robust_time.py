"""Weighted GN pass of the spline path at configs[4] beside the unweighted one.

Two handles over the same problem (the synthetic configs[4], contaminated in the proportions the tests use -- 3 % of
the corners shifted 20 .. 60 px, 2 % of the gyro and accel samples offset by 100 sigma -- by random draws of its own,
not tests/spline_robust_ref.contaminate_spline's):
  unweighted  k_sp_frames<..>, k_sp_assemble<false>, k_sp_cost_frames<..>
  weighted    Huber on all three families + a per-corner invR: the <.., true> instantiations
Each runs `--passes` captured GN passes from the initial state (one warm-up run captures the graph).  Prints one JSON
line: GN iterations/s of both and the per-kernel event times of kb_sp_kernel_stats.  Under
`rocprofv3 --kernel-trace --stats` the same run gives the device time of every kernel by name.

--stats FILE: summarise the kernel trace of such a run (no GPU needed), rocprofv3's results .db or, with
--output-format csv, its kernel_trace.csv: calls, median and mean device time of k_sp_frames, k_sp_assemble and
k_sp_cost_frames, unweighted against weighted."""
import argparse
import csv
import dataclasses
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def contaminated(p, seed=7):
    import numpy as np
    rng = np.random.default_rng(seed)
    n, M = p.n_corners, p.n_imu
    y = np.array(p.y, dtype=np.float64, copy=True)
    idx = rng.choice(n, size=max(1, int(round(0.03 * n))), replace=False)
    r, th = rng.uniform(20.0, 60.0, idx.size), rng.uniform(0.0, 2.0 * np.pi, idx.size)
    y[idx, 0] += r * np.cos(th)
    y[idx, 1] += r * np.sin(th)
    gy, ac = np.array(p.imu_gyro, copy=True), np.array(p.imu_acc, copy=True)
    for arr, sig in ((gy, p.sigma_gyro), (ac, p.sigma_acc)):
        k = rng.choice(M, size=max(1, int(round(0.02 * M))), replace=False)
        arr[k] += rng.normal(0.0, 100.0 * sig, (k.size, 3))
    return dataclasses.replace(p, y=y, imu_gyro=gy, imu_acc=ac)


def run(a):
    import numpy as np

    from kalibr_amd import capi, synth
    p = contaminated(synth.make_spline_config())
    rng = np.random.default_rng(1)
    n = p.n_corners
    s1, s2, th = rng.uniform(0.2, 0.6, n), rng.uniform(0.2, 0.6, n), rng.uniform(0.2, 1.3, n)
    c, s = np.cos(th), np.sin(th)
    ia, ib = 1.0 / (s1 * s1), 1.0 / (s2 * s2)
    invR = np.stack([ia * c * c + ib * s * s, (ia - ib) * c * s, ia * s * s + ib * c * c], axis=1)
    out = dict(n_corners=int(n), n_imu=int(p.n_imu), passes=a.passes)
    for name in ("unweighted", "weighted"):
        g = capi.SplineSolver(p)
        if name == "weighted":
            g.set_mestimator("reprojection", "huber", 2.5)
            g.set_mestimator("gyro", "huber", 3.0)
            g.set_mestimator("accel", "huber", 3.0)
            g.set_corner_invR(invR)
        for _ in range(2):  # the first run captures the graph and warms up; the second is the timed one
            g.set_state(p.state_init)
            sec = g.run_gn(a.passes)
        g.set_state(p.state_init)
        ks = g.kernel_stats(20)
        out[name] = dict(gn_it_per_s=a.passes / sec, J_after=g.eval_cost(),
                         **{k: float(v) for k, v in ks.items() if k.endswith("_ms")})
        g.close()
    print(json.dumps(out))


PAT = re.compile(r"k_sp_(frames|assemble|cost_frames)<[^>]*>")


def summarise(a):
    import statistics
    if a.stats.endswith(".db"):  # rocprofv3's default output: the rocpd database, one row per dispatch in `kernels`
        import sqlite3
        disp = sqlite3.connect(a.stats).execute("select name, start, end from kernels")
    else:  # --output-format csv: kernel_trace.csv, one row per dispatch
        with open(a.stats, newline="") as f:
            disp = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows = {}
    for name, s, e in disp:
        m = PAT.search(name)
        if m:
            rows.setdefault(m.group(0), []).append((e - s) / 1e3)
    for name, v in sorted(rows.items()):
        print("%-40s calls %5d  median %8.2f us  mean %8.2f us" % (name, len(v), statistics.median(v),
                                                                statistics.mean(v)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--stats", default="")
    a = ap.parse_args()
    summarise(a) if a.stats else run(a)
