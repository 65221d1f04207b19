"""DogLegTrustRegionPolicy of the C++ host layer (kalibr_amd/host/kalibr_backend.*, tests/cpp/test_host_dogleg.cpp).

CPU: Optimizer2::optimize() with the policy over the oracle-backed solver (rhsJtJrhs from the arrow blocks) against
the restatement in tests/dogleg_ref.py: equal step / accept sequences, delta, beta and J to rel 1e-12 (the same
arithmetic on the same CPU); name(), requiresAugmentedDiagonal(), revertOnFailure(); a solver whose solveSystem
fails ends with linearSolverFailure and failedIterations == maxIterations.
GPU: the policy over GpuLinearSystemSolver through the host loop and through optimizeOnDevice(): equal sequences,
JFinal rel 1e-9, states abs 1e-6.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from kalibr_amd import build as B
from kalibr_amd import synth

from . import dogleg_ref as R
from .host_problem import write_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory, oracle_mod):
    if not os.path.exists(B.OUT):
        B.build()
    B.build_host()
    out = str(tmp_path_factory.mktemp("host_dogleg") / "test_host_dogleg")
    ob = os.path.join(ROOT, "oracle", "_build")
    cmd = ["g++", "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "cpp", "test_host_dogleg.cpp"),
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


@pytest.fixture(scope="module")
def c1_12(tmp_path_factory):
    p = synth.make_config(1, n_frames=12)
    path = str(tmp_path_factory.mktemp("host_dogleg_p") / "c1_12.bin")
    write_problem(path, p)
    return p, path


# the parameter sets of the device tests: the reference's delta = 0 start, and all three branches
@pytest.mark.parametrize("delta_init,eps_x,eps_j,max_it,steps", [(0.0, 1e-3, 1.0, 25, "DGGG"),
                                                                 (1e-3, 1e-9, 1e-3, 25, "SSSSDDDDDGGG")])
def test_host_policy_matches_the_restatement(driver, oracle_mod, c1_12, delta_init, eps_x, eps_j, max_it, steps):
    p, path = c1_12
    ref = R.run(oracle_mod.Oracle(p), p.state_init, delta_init, eps_x, eps_j, max_it)
    R.assert_not_marginal(ref)
    assert ref["steps"] == steps
    r = _run(driver, "cpu", path, repr(delta_init), repr(eps_x), repr(eps_j), max_it)
    assert r["name"] == "dog_leg" and r["augmented"] == 0 and r["revert"] == 1
    assert "".join(R.STEP[t] for t in r["type"]) == steps
    assert "".join(map(str, r["accepted"])) == ref["accepted"]
    assert r["srv"]["iterations"] == ref["iterations"] and r["srv"]["failedIterations"] == ref["failed_iterations"]
    assert r["srv"]["linearSolverFailure"] == 0
    worst = 0.0
    for k, q in enumerate(ref["passes"]):
        for got, want in ((r["delta"][k], q["delta"]), (r["J"][k], q["J"])) + (
                ((r["beta"][k], q["beta"]),) if q["type"] == R.DL else ()):
            worst = max(worst, abs(got - want) / abs(want))
    print("worst rel", worst)
    assert worst <= 1e-12
    assert abs(r["srv"]["JFinal"] - ref["J_final"]) <= 1e-12 * ref["J_final"]
    assert np.abs(np.array(r["state"]) - ref["state"]).max() <= 1e-9
    # printState as the reference prints it: "DL - delta:<delta>, <type>[, beta:<beta>]"
    last = ref["passes"][-1]
    assert r["print"].startswith("DL - delta:") and r["print"].split(", ")[1] == {0: "SD", 1: "GN", 2: "DL"}[last["type"]]
    assert ("beta:" in r["print"]) == (last["type"] == R.DL)


def test_failing_solver_ends_with_linear_solver_failure(driver, c1_12):
    _, path = c1_12
    r = _run(driver, "fail", path, 7)
    assert r["srv"]["linearSolverFailure"] == 1 and r["srv"]["failedIterations"] == 7
    assert r["srv"]["iterations"] == 0 and r["state_unchanged"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("delta_init,eps_x,eps_j,max_it", [(0.0, 1e-3, 1.0, 25), (1e-3, 1e-9, 1e-3, 13)])
def test_host_loop_and_device_loop_agree(driver, tmp_path, delta_init, eps_x, eps_j, max_it):
    p = synth.make_config(4, n_frames=8, p_view=0.7)  # c4_8
    path = str(tmp_path / "c4_8.bin")
    write_problem(path, p)
    r = _run(driver, "gpu", path, repr(delta_init), repr(eps_x), repr(eps_j), max_it)
    print(r)
    assert r["host_type"] == r["device_type"] and r["host_accepted"] == r["device_accepted"]
    assert r["host"]["iterations"] == r["device"]["iterations"]
    assert r["host"]["failedIterations"] == r["device"]["failedIterations"]
    assert abs(r["host"]["JFinal"] - r["device"]["JFinal"]) <= 1e-9 * r["host"]["JFinal"]
    assert r["state_diff"] <= 1e-6
