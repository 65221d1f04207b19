"""Weighted LM pass at a synthetic config (default configs[3], 8 cameras x 2000 frames) beside the unweighted passes.

Three handles over the same problem run `--iterations` LM iterations from the initial state (convergence tests off,
one warm-up run each to capture the pass graphs):
  weighted   per-corner invR + Huber(2): k_build<.., WT = true>, k_backsub_w, k_cost_w
  k_build    unweighted with KB_BUILD_PIPE=0: k_build<..> (what a weighted handle's build is derived from)
  default    unweighted: k_buildp where the rig has one wave per camera
Prints one JSON line: the build kernel each handle reports, passes and host wall time per pass.  Under
`rocprofv3 --kernel-trace --stats` the same run gives the device time of every kernel by name.

--stats FILE: summarise a rocprofv3 kernel_stats CSV of such a run (no GPU needed): calls, average and total device
time of the build, back-substitution and cost kernels of the three variants."""
import argparse
import csv
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(a):
    import numpy as np

    from kalibr_amd import capi, synth
    p = synth.make_config(a.config, **({"n_frames": a.frames} if a.frames else {}))
    rng = np.random.default_rng(1)
    n = p.n_corners
    s1, s2, th = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n), rng.uniform(0.2, 1.3, n)
    c, s = np.cos(th), np.sin(th)
    ia, ib = 1.0 / (s1 * s1), 1.0 / (s2 * s2)
    invR = np.stack([ia * c * c + ib * s * s, (ia - ib) * c * s, ia * s * s + ib * c * c], axis=1)
    out = dict(config=a.config, n_corners=int(n), iterations=a.iterations)
    for name in ("weighted", "k_build", "default"):
        if name == "k_build":
            os.environ["KB_BUILD_PIPE"] = "0"  # read by kb_create
        else:
            os.environ.pop("KB_BUILD_PIPE", None)
        g = capi.Solver(p)
        if name == "weighted":
            g.set_mestimator("huber", 2.0)
            g.set_corner_invR(invR)
        for timed in (False, True):
            g.set_state(p.state_init)
            t0 = time.perf_counter()
            res = g.optimize(policy="lm", lambda0=10.0, max_iterations=a.iterations, eps_x=-1.0, eps_j=-1.0,
                             sync_every=8, use_graph=True)
            dt = time.perf_counter() - t0
        out[name] = dict(build_kernel=g.build_kernel_name(), passes=res["passes"], iterations=res["iterations"],
                         failed_iterations=res["failed_iterations"], J_final=res["J_final"],
                         wall_ms_per_pass=1e3 * dt / max(res["passes"], 1))
        g.close()
    print(json.dumps(out))


def summarise(a):
    rows = []
    with open(a.stats, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            m = re.search(r"k_\w+(<[^>]*>)?", name)
            if not m or not re.search(r"k_build|k_backsub|k_cost|k_solve|k_colsum|k_colimg|k_schur|k_post", m.group(0)):
                continue
            rows.append((m.group(0), int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e3))
    for name, calls, avg, tot in sorted(rows):
        print("%-40s calls %5d  avg %9.2f us  total %11.1f us" % (name, calls, avg, tot))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=4)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--stats", default="")
    a = ap.parse_args()
    summarise(a) if a.stats else run(a)
