"""GpuLinearSystemSolver::setRobustBuild of the C++ host layer (tests/cpp/test_host_robust_pipe.cpp).

A weighted solver (Cauchy + per-corner invR) in Pipe mode under Optimizer2::optimizeOnDevice() with the GN policy on
c4_small runs fused on the weighted k_buildp: iterations and state against the numpy restatement (tests/robust_ref.py)
at the project's bars (same iteration counts, J_start rel 1e-12, J_final rel 1e-9, state abs 1e-6).  setRobustBuild(Pipe)
on a rig that builds with k_build throws with the C-ABI's message and leaves the solver as it was."""
import json
import os
import subprocess

import numpy as np
import pytest

from kalibr_amd import build as B

from . import test_gpu_robust as T
from . import test_gpu_robust_pipe as P
from .host_problem import write_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def driver(tmp_path_factory, oracle_mod):
    if not os.path.exists(B.OUT):
        B.build()
    B.build_host()
    out = str(tmp_path_factory.mktemp("host_robust_pipe") / "test_host_robust_pipe")
    ob = os.path.join(ROOT, "oracle", "_build")
    cmd = ["g++", "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "cpp", "test_host_robust_pipe.cpp"),
           "-I", os.path.join(ROOT, "tests", "cpp"),
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kalibr_amd", "host"),
           "-I", os.path.join(ROOT, "oracle"),
           "-L", os.path.join(ROOT, "kalibr_amd"), "-lkalibr_backend", "-lkalibr_hip",
           "-L", ob, "-lkb_oracle", "-lpthread",
           "-Wl,-rpath," + os.path.join(ROOT, "kalibr_amd") + ":" + ob]
    subprocess.run(cmd, check=True)
    return out


def _run(driver, *args):
    r = subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_gn_on_device_runs_fused_in_pipe_mode(driver, oracle_mod, tmp_path):
    case = ("c4_small", "gn", "cauchy", "per_corner", 8)
    st_r, ref = P.opt_reference(oracle_mod, case)  # asserts that no decision is marginal
    p = P.rig(oracle_mod, "c4_small")[0]
    path, ipath = str(tmp_path / "p.bin"), str(tmp_path / "invR.f64")
    write_problem(path, p)
    T.per_corner_invR(p.n_corners).astype(np.float64).tofile(ipath)
    r = _run(driver, "gn-gpu", path, ipath, T.ESTIMATORS["cauchy"][1])
    st = np.array(r["state"])
    print({k: v for k, v in r.items() if k != "state"}, ref["iterations"], ref["J_final"], float(np.abs(st - st_r).max()))
    assert r["kernel"] == "k_buildp" and r["rc_fused"] == 0
    assert r["iterations"] == ref["iterations"] >= 2 and r["failed"] == ref["failed_iterations"]
    assert r["linear_solver_failure"] == 0
    assert abs(r["J_start"] - ref["J_start"]) <= 1e-12 * ref["J_start"]
    assert abs(r["J_final"] - ref["J_final"]) <= 1e-9 * ref["J_final"]
    assert np.abs(st - st_r).max() <= 1e-6
    # General again: k_build, and the fused entry point is refused
    assert r["kernel_general"] == "k_build" and r["rc_general"] < 0 and r["mode"] == 0


def test_pipe_is_refused_on_a_k_build_rig(driver, oracle_mod, tmp_path):
    p = P.rig(oracle_mod, "c1_12")[0]
    path = str(tmp_path / "p.bin")
    write_problem(path, p)
    r = _run(driver, "refuse-gpu", path)
    print(r)
    for m in (r["message"], r["message_init"]):
        assert "kb_set_robust_build" in m and "builds with k_build" in m
    assert r["mode"] == 0 and r["kernel"] == "k_build" and r["cost_same"] == 1
