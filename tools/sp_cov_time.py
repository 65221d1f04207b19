"""Host time of kb_sp_covariance (SplineSolver.covariance) at configs[4], with and without the Sigma_s,theta output:
median / min over --calls calls after --warmup, beside kb_sp_solve on the same built system in the same process, and
the full-size residual max |(H + lambda^2 I) [Sigma_tt; Sigma_s,theta] - [I; 0]| formed in numpy from
kb_sp_get_system's blocks by a banded product (the only full-size check: a dense inverse of 18,043 columns is not a
test).  One JSON line.  Under `rocprofv3 --kernel-trace --stats` the same run gives the device times of the k_sp_cov_*
kernels (tools/prof_summary.py reads the stats file)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kalibr_amd import capi, synth  # noqa: E402


def banded_residual(s, lam, Ptt, Pst):
    """max |(H + lam^2 I) [Ptt; Pst] - [I; 0]| with H = [[Hcc, Hsc^T], [Hsc, band]]"""
    C, K = Ptt.shape[0], s["Hband"].shape[0]
    l2 = lam * lam
    top = s["Hcc"] @ Ptt + l2 * Ptt + s["Hsc"].T @ Pst - np.eye(C)
    X = Pst.reshape(K, 6, C)
    Y = (s["Hsc"] @ Ptt).reshape(K, 6, C) + l2 * X
    for d in range(s["Hband"].shape[1]):
        B = s["Hband"][:K - d, d]  # block (k, k + d)
        Y[:K - d] += np.einsum("kab,kbc->kac", B, X[d:])
        if d:
            Y[d:] += np.einsum("kba,kbc->kac", B, X[:K - d])
    return float(max(np.abs(top).max(), np.abs(Y).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=0, help="0: configs[4] as bench.py --config 5 makes it")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--conditioner", type=float, default=10.0)
    a = ap.parse_args()
    p = synth.make_spline_config(**({"n_frames": a.frames} if a.frames else {}))
    g = capi.SplineSolver(p)
    g.set_state(p.state_init)
    g.build()
    g.set_constant_conditioner(a.conditioner)
    res = dict(C=g.C, K=g.K, nodes=(g.K + 2) // 3, calls=a.calls, conditioner=a.conditioner)
    out = None
    for cross in (False, True):
        for _ in range(a.warmup):
            ok, out = g.covariance(cross=cross, out=out)
            assert ok
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            ok, out = g.covariance(cross=cross, out=out)
            ts.append(time.perf_counter() - t0)
        key = "with_Pst" if cross else "without_Pst"
        res[key + "_ms_median"] = 1e3 * float(np.median(ts))
        res[key + "_ms_min"] = 1e3 * float(np.min(ts))
    ts = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        g.solve()
        ts.append(time.perf_counter() - t0)
    res["kb_sp_solve_ms_median"] = 1e3 * float(np.median(ts))
    res["kb_sp_solve_ms_min"] = 1e3 * float(np.min(ts))
    res["residual"] = banded_residual(g.system(), a.conditioner, out["Ptt"], out["Pst"])
    res["max_Ptt"] = float(np.abs(out["Ptt"]).max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
