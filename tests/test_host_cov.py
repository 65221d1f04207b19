"""Covariance surface of the C++ host layer (kalibr_amd/host/kalibr_backend.*): ProblemLinearSystemSolver::
computeCovarianceBlocks / supportsCovariance, Optimizer2::computeHessian / computeDiagonalCovariances /
computeCovarianceBlocks and CalibrateCamerasResult::parameterStdDev (tests/cpp/test_host_cov.cpp).

CPU: the design-variable pair -> (source, row range, column range) mapping for a pinhole-radtan (4|4), FOV (4|1),
EUCM (6) rig against an independent restatement; a solver without the override reports no support, throws, and
calibrateCameras over it returns normally with parameterStdDev empty.
GPU: Optimizer2::computeDiagonalCovariances(0) equals the C-ABI blocks (kb_covariance), through the DV / term layer
in insertion order and in a shuffled order the same blocks per design variable (the shuffle reorders the frames, so
to rounding: correlation-normalised 1e-8, the bound of tests/test_gpu_covariance.py); computeHessian(lambda) equals
kb_get_normal_blocks + lambda^2 on the diagonal; a pair of two different frames throws.
"""
import json
import os
import subprocess

import pytest

from kalibr_amd import build as B
from kalibr_amd import synth

from .host_problem import write_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory, oracle_mod):
    if not os.path.exists(B.OUT):
        B.build()
    B.build_host()
    out = str(tmp_path_factory.mktemp("host_cov") / "test_host_cov")
    ob = os.path.join(ROOT, "oracle", "_build")
    cmd = ["g++", "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "cpp", "test_host_cov.cpp"),
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


def test_block_index_to_range_mapping(driver):
    r = _run(driver, "ranges")
    # pinhole-radtan 4|4, FOV 4|1, EUCM 6 (one DV), two baselines q|t, three frames q|t
    dims = [4, 4, 4, 1, 6] + [3, 3] * 2 + [3, 3] * 3
    assert r["dims"] == dims
    ncam, F = 9, 3
    col = [sum(dims[:k]) for k in range(ncam)]  # first camera column of each camera DV
    assert col[-1] + dims[ncam - 1] == 4 + 4 + 4 + 1 + 6 + 12
    n = len(dims)
    assert len(r["pairs"]) == n * n
    for i in range(n):
        for j in range(n):
            got = r["pairs"][i * n + j]
            fi, fj = i >= ncam, j >= ncam
            if fi and fj and (i - ncam) // 2 != (j - ncam) // 2:
                assert got == ["throw", 1, 0, 0, 0, 0], (i, j, got)  # two different frames, and the message says so
                continue
            if not fi and not fj:
                want = ["Pcc", -1, col[i], dims[i], col[j], dims[j]]
            elif fi and fj:
                want = ["Pff", (i - ncam) // 2, 3 * ((i - ncam) % 2), 3, 3 * ((j - ncam) % 2), 3]
            elif fi:
                want = ["Pfc", (i - ncam) // 2, 3 * ((i - ncam) % 2), 3, col[j], dims[j]]
            else:
                want = ["PfcT", (j - ncam) // 2, col[i], dims[i], 3 * ((j - ncam) % 2), 3]
            assert got == want, (i, j, got, want)
    assert r["out_of_range_throws"] == 3


def test_solver_without_covariance(driver, tmp_path):
    """the oracle-backed ProblemLinearSystemSolver has no override: no support, the default throws, and the stage
    sequence over it still returns, with no standard deviations"""
    p = synth.make_problem([synth.PINHOLE_RADTAN] * 3, 24, seed=5150)
    path = str(tmp_path / "p.bin")
    write_problem(path, p)
    r = _run(driver, "unsupported", path)
    assert r["supports"] == 0 and r["blocks"] == 0
    assert r["message"] == "computeCovarianceBlocks: not supported by this solver"
    assert r["optimizer_message"] == "computeCovarianceBlocks: not supported by this solver"
    assert r["accepted_batches"] > 0 and r["stats_cams"] == 3  # the calibration itself ran
    assert r["std_dev_size"] == 0


@pytest.mark.gpu
def test_optimizer2_covariances_on_the_device(driver, tmp_path):
    p = synth.make_config(1, n_frames=12)  # c1_small
    path = str(tmp_path / "p.bin")
    write_problem(path, p)
    r = _run(driver, "gpu", path)
    print(r)
    assert r["supports"] == 1 and r["n_dvs"] == 2 + 2 * 12
    assert r["abi_diff"] == 0.0 and r["off_diff"] == 0.0  # the blocks are slices of the C-ABI output
    assert r["hess_diff"] == 0.0
    assert r["cross_throws"] == 1
    assert r["term_insertion_err"] == 0.0  # the same canonical problem on the device
    assert r["frames_reordered"] > 0 and r["term_shuffled_err"] <= 1e-8, r


@pytest.mark.gpu
def test_calibrate_cameras_reports_parameter_std_dev(driver, tmp_path):
    """over the GPU solvers calibrateCameras fills parameterStdDev: one positive finite value per camera column
    (3 x (4 + 4) intrinsics + 2 x 6 baseline columns)"""
    p = synth.make_problem([synth.PINHOLE_RADTAN] * 3, 24, seed=5150)
    path = str(tmp_path / "p.bin")
    write_problem(path, p)
    r = _run(driver, "stddev-gpu", path)
    print(r)
    assert r["accepted_batches"] > 0
    assert r["std_dev_size"] == 3 * 8 + 2 * 6
    assert 0.0 < r["min"] and r["max"] < 1e300  # positive and finite
