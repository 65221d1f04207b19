"""k_solve<0> beyond what test_gpu_solve_widths.py holds (dx, covariance and the loops at C = 65 .. 111 against the oracle
and LAPACK: the yardstick of the left-looking trailing updates): what the waves' hand-offs inside the kernel could break
without moving a result of a single run.

Repeatability, C = 65, 80, 111 (nb = 5, 6, 7): three captured GN passes twice from the same state give the same state
and the same chains in both slots, to the bit, and kb_optimize's GN loop gives that state too.  The update waves
(2, 3, 6, 7, and 5 beside a single factor wave) read tiles other waves factored in earlier panels and write tiles the
next panel reads, with one block barrier per phase between them, and wave 1 waits on an LDS flag of the backsolve
wave: a read that raced its producer would differ from run to run.  On the omni-radtan rig of C = 111 undamped
Gauss-Newton is not defined (tests/solve_width_cases.py): a pass fails its factorisation, run_gn reports it, and the
state it leaves must repeat all the same.

A factorisation that fails inside the fused loop, C = 80 with a frame that lost its corners (W.nonpd_problem): the
update of the candidate state is off for the whole block, so wave 1 neither waits for the backsolve's flag nor builds
chains.  The GPU part runs in a child process under a time limit, so a wave left waiting shows as a failure of this
test and not as a suite that never ends.  The loop reports the failure, the state and both slots' chains are untouched
(the candidate slot of the fresh handle stays all zero), and the next per-call build reproduces the normal equations
taken before the loop.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from . import solve_width_cases as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (65, 80, 111)
CHILD_LIMIT = 120        # seconds; the child's GPU work is a handful of launches
BLOCKS = ("Hff", "Hfc", "gf", "Hcc", "gc")


@pytest.fixture(scope="module")
def capi():
    from kalibr_amd import capi as K
    return K


def _snapshot(g):
    return (g.get_state(),) + g.debug_chains(0) + g.debug_chains(1)


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("C", ROWS)
def test_gn_passes_repeat_to_the_bit(capi, C):
    p = W.problem(C)
    g = capi.Solver(p)
    try:
        assert g.C == C and g.build_kernel_name() == "k_buildp"
        runs, failed = [], []
        for _ in range(2):
            g.set_state(p.state_init)
            try:
                g.run_gn(3)
                failed.append(False)
            except capi.KbError as e:      # undamped GN is not defined on the omni-radtan rig: a pass reports it
                assert "linear solver failures" in str(e), e
                failed.append(True)
            runs.append(_snapshot(g))
        assert failed[0] == failed[1] == (C in W.SINGULAR_ROWS)
        assert _same(runs[0], runs[1])
        g.set_state(p.state_init)
        r = g.optimize(**W.GN)
        assert bool(r["linear_solver_failure"]) == failed[0]
        assert g.get_state().tobytes() == runs[0][0].tobytes(), r
        assert np.isfinite(runs[0][0]).all()
    finally:
        g.close()


CHILD = r"""
import sys
import numpy as np
from kalibr_amd import capi
from tests import solve_width_cases as W

p = W.nonpd_problem(80)
g = capi.Solver(p)
assert g.C == 80 and g.build_kernel_name() == "k_buildp"
out = {}


def take(tag):
    out[tag + "_state"] = g.get_state()
    for which in (0, 1):
        out[f"{tag}_L{which}"], out[f"{tag}_K{which}"] = g.debug_chains(which)


g.set_state(p.state_init)
g.build()
for k, v in g.normal_blocks().items():
    out["before_" + k] = np.asarray(v)
take("before")
r = g.optimize(**W.GN)
out["opt"] = np.array([r["linear_solver_failure"], r["iterations"], r["failed_iterations"], r["passes"]])
take("after_opt")
try:
    g.run_gn(3)
    out["run_failed"] = np.array(0)
except capi.KbError as e:
    assert "linear solver failures" in str(e), e
    out["run_failed"] = np.array(1)
take("after_run")
g.build()
for k, v in g.normal_blocks().items():
    out["after_" + k] = np.asarray(v)
np.savez(sys.argv[1], **out)
"""


def test_failed_factorisation_in_the_fused_loop(tmp_path):
    path = str(tmp_path / "nonpd80.npz")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", CHILD, path]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_LIMIT)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(path)
    lin_fail, iterations, failed, passes = (int(v) for v in z["opt"])
    print(f"fused GN loop on the non-PD row: linear_solver_failure {lin_fail} iterations {iterations} failed {failed} "
          f"passes {passes}")
    assert lin_fail == 1 and iterations == 0 and failed >= 1 and int(z["run_failed"]) == 1
    for tag in ("after_opt", "after_run"):
        assert z[tag + "_state"].tobytes() == z["before_state"].tobytes(), tag
        for which in (0, 1):                                   # slot cur kept, the candidate slot not written
            for q in ("L", "K"):
                assert z[f"{tag}_{q}{which}"].tobytes() == z[f"before_{q}{which}"].tobytes(), (tag, q, which)
    assert not z["before_K1"].any() and not z["before_L1"].any()   # the candidate slot of a fresh handle
    for k in BLOCKS + ("cost",):
        assert z["after_" + k].tobytes() == z["before_" + k].tobytes(), k
