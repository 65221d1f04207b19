"""Host time of kb_covariance (Solver.covariance) at a synthetic config, with and without the Sigma_fc output:
median / min over --calls calls after --warmup, one JSON line.  Under `rocprofv3 --kernel-trace --stats` the same run
gives the device times of k_cov_cam and k_cov_frames (tools/prof_summary.py reads the stats file)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kalibr_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=4, help="synth.make_config index (4: configs[3], C = 106, F = 2000)")
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--conditioner", type=float, default=1.0)
    a = ap.parse_args()
    p = synth.make_config(a.config, **({"n_frames": a.frames} if a.frames else {}))
    g = capi.Solver(p)
    g.set_state(p.state_init)
    g.build()
    g.set_constant_conditioner(a.conditioner)
    F = (g.ncols - g.C) // 6
    res = dict(config=a.config, C=g.C, F=F, calls=a.calls)
    for cross in (False, True):
        out = None
        for _ in range(a.warmup):
            ok, out = g.covariance(cross=cross, out=out)
            assert ok
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            ok, out = g.covariance(cross=cross, out=out)
            ts.append(time.perf_counter() - t0)
        key = "with_Pfc" if cross else "without_Pfc"
        res[key + "_ms_median"] = 1e3 * float(np.median(ts))
        res[key + "_ms_min"] = 1e3 * float(np.min(ts))
    # the solve of the same system, for scale
    ts = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        g.solve()
        ts.append(time.perf_counter() - t0)
    res["kb_solve_ms_median"] = 1e3 * float(np.median(ts))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
