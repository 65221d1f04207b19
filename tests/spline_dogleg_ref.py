"""Restatement of the dog-leg trust-region policy over the spline oracle's primitives (SplineOracle: cost, system,
solve(sys, 0.0), apply_update): the checker of tests/test_gpu_spline_dogleg.py, with its preconditions in
tests/test_spline_dogleg_ref.py.  The policy itself is tests/dogleg_ref.py's (select, assert_not_marginal are imported,
not restated); what is new here is the spline system's g^T H g from its blocks and the Optimizer2 loop over an oracle
whose system is (Hcc, Hsc, Hband, gc, gs) instead of an arrow.  Both deviations of the project's policy are included:
delta_init, and a GN step that counts as held only after a completed solve.
"""
import functools

import numpy as np

from . import spline_cases as SC
from .dogleg_ref import DL, GN, SD, STEP, _norm, _sum, assert_not_marginal, select  # noqa: F401

# the options of every dog-leg run in the spline tests
OPT = dict(eps_x=1e-3, eps_j=1.0, max_iterations=25)

# (case, delta_init): the runs of tests/test_gpu_spline_dogleg.py.  delta_init exceeds eps_x wherever it is not 0 (the
# first SD step would end the loop otherwise).  n2b, n64 and n65 at delta_init = 0 are marginal on their last pass
# (|dJ| / J about 1e-9) and are not run.
RUNS = [("n3", 0.01), ("n33", 0.01), ("c23", 0.01), ("c64", 0.01), ("views", 0.01), ("n17", 0.01), ("n7", 0.0),
        ("n2c", 0.0), ("n4", 0.0), ("imu_dense", 0.01), ("c44", 0.05)]
# The precondition on a run's J_final (rel 1e-9) and state (1e-6) bars, spline_cases.LM_REPRO_MAX's argument: the
# restatement run once more with the oracle's dense solver in place of its band solver must end within those bars of
# itself, or it cannot referee them for a device that eliminates in yet another order.
REPRO_STATE_MAX, REPRO_J_MAX = 1e-6, 1e-9
# Not run for that reason: (n2c, 0.01) -- SDDDDDDDGGGDDGGGGGGGGGGGG, 1111111100011000000000000, not marginal; a 13-frame,
# two-node problem whose GN steps have norm 6 .. 120 and are rejected from pass 8 on.  The oracle's two solvers end
# 3.7e-6 apart in state and 6.9e-7 in J (the device: 2.3e-6 and 2.3e-7 from the band run, every per-pass quantity
# within its bar).  (imu_dense, 0.01) takes its place: all three step types and sixteen rejected passes on one system.
NOT_REPRODUCIBLE = [("n2c", 0.01)]


class Adapter:
    """SplineOracle behind the four primitives the loop needs; system() adds rhs = [gc | gs]"""

    def __init__(self, oracle, nthreads=4):
        self.o = oracle
        self.nthreads = nthreads

    def cost(self, state):
        return self.o.cost(state)

    def system(self, state):
        s = self.o.system(state, nthreads=self.nthreads)
        s["rhs"] = np.concatenate([s["gc"], s["gs"]])
        return s

    def solve(self, sysd, lam=0.0):
        return self.o.solve(sysd, lam)

    def apply_update(self, state, dx):
        return self.o.apply_update(state, dx)


class DenseAdapter(Adapter):
    """the same with the oracle's dense solver (the reproducibility precondition)"""

    def solve(self, sysd, lam=0.0):
        return self.o.solve(sysd, lam, dense=True)


def g_h_g(s):
    """g^T H g of a spline system from its blocks: g_c^T H_cc g_c + 2 g_s^T H_sc g_c + sum_k (g_k^T B_k0 g_k +
    2 sum_d>0 g_k^T B_kd g_(k+d)) with B_kd = Hband[k][d] the block (k, k + d); left-to-right sums."""
    gc, gs = s["gc"], s["gs"]
    K, order = s["Hband"].shape[:2]
    g6 = gs.reshape(K, 6)
    terms = [((gc[:, None] * s["Hcc"]) * gc[None, :]).ravel(), (((2.0 * gs)[:, None] * s["Hsc"]) * gc[None, :]).ravel()]
    for d in range(order):
        n = K - d
        if n <= 0:
            break
        w = 1.0 if d == 0 else 2.0
        terms.append(((w * g6[:n, :, None]) * s["Hband"][:n, d] * g6[d:d + n, None, :]).ravel())
    return _sum(np.concatenate(terms))


def steepest_descent(s):
    """(g, sd_scale, dx_sd, |dx_sd|) of a spline system (DogLegTrustRegionPolicy.cpp:70-75)"""
    g = s["rhs"] if "rhs" in s else np.concatenate([s["gc"], s["gs"]])
    sd_scale = _sum(g * g) / g_h_g(s)
    dx_sd = sd_scale * g
    return g, sd_scale, dx_sd, _norm(dx_sd)


def run(oracle, state0, delta_init=0.0, eps_x=1e-3, eps_j=1.0, max_iterations=25, floors=False):
    """tests/dogleg_ref.py's run (the Optimizer2 loop with the policy) over an Adapter.  Returns dict(passes=[dict per
    pass], iterations, failed_iterations, linear_solver_failure, J_start, J_final, state, steps, accepted).  floors:
    every pass that solves also records the oracle's own error at that system, max|dx_band - dx_dense| / max|dx_dense|
    (spline_cases.solve_floor), from which the per-pass bars are derived."""
    state = np.array(state0, dtype=np.float64)
    J = oracle.cost(state)
    p_J = J
    res = dict(J_start=J, passes=[])
    dX, dJ = eps_x + 1.0, eps_j + 1.0
    prev_failed = lin_fail = False
    it = failed = 0
    pol_J = pol_pJ = last_succ = J
    first = True
    delta, L0, beta, stype = float(delta_init), 0.0, 0.0, None
    sdn = gnn = sd_scale = 0.0
    dx = dx_sd = dx_gn = None
    gn_held = False
    A = None
    while it < max_iterations and failed < max_iterations and ((dX > eps_x and abs(dJ) > eps_j) or lin_fail):
        if prev_failed:
            pol_J = J
        else:
            pol_pJ, last_succ, pol_J = last_succ, J, J
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = float(np.float64(pol_pJ - pol_J) / np.float64(L0))
        rec = dict(rho=None, floor=None)
        if not first:
            rec["rho"] = rho
            if rho > 0.75:
                n3 = 3 * _norm(dx)
                if not delta > n3:
                    delta = n3
            elif 0 < rho < 0.25:
                delta /= 2.0
            elif rho <= 0:
                delta = gnn / 2.0 if stype == GN else delta / 2.0
        rec["built"] = not prev_failed
        if not prev_failed:
            A = oracle.system(state)
            _, sd_scale, dx_sd, sdn = steepest_descent(A)
            gn_held = False
            gnn = 0.0
        first = False
        ok = True
        rec["solved"] = False
        if not (sdn >= delta and delta != 0) and not gn_held:
            ok, sol = oracle.solve(A, 0.0)
            rec["solved"] = True
            if ok:
                dx_gn, gnn, gn_held = sol, _norm(sol), True
                if floors:
                    rec["floor"] = SC.solve_floor(oracle.o, A, 0.0)[2]
        if not ok:  # deviation 2
            prev_failed = lin_fail = True
            failed += 1
            rec.update(type=-1, delta=delta, beta=beta, L0=L0, sdn=sdn, gnn=gnn, J=float("nan"), accepted=0,
                       compared=[], dJ_rel=None)
            res["passes"].append(rec)
            continue
        s = select(delta, J, sd_scale, dx_sd, sdn, dx_gn, gnn)
        delta, L0, stype, dx = s["delta"], s["L0"], s["type"], s["dx"]
        if s["beta"] is not None:
            beta = s["beta"]
        cand, dX = oracle.apply_update(state, dx)
        J = oracle.cost(cand)
        dJ = p_J - J
        rec.update(type=stype, delta=delta, beta=beta, L0=L0, sdn=sdn, gnn=gnn, J=J, compared=s["compared"],
                   dJ_rel=abs(dJ) / p_J, dx_norm=float(np.linalg.norm(dx)), dX=dX)
        if dJ < 0.0:
            failed += 1
            prev_failed = True
            rec["accepted"] = 0
        else:
            state, p_J, prev_failed = cand, J, False
            rec["accepted"] = 1
        it += 1
        res["passes"].append(rec)
    res.update(iterations=it, failed_iterations=failed, linear_solver_failure=int(lin_fail), J_final=p_J, state=state,
               steps="".join(STEP[p["type"]] if p["type"] >= 0 else "x" for p in res["passes"]),
               accepted="".join(str(p["accepted"]) for p in res["passes"]))
    return res


@functools.lru_cache(maxsize=None)
def reference(name, delta_init):
    """the restatement's run of one of RUNS from the case's state_init with OPT, computed once per process and shared
    (read-only); res["worst"] is assert_not_marginal's report, res["bar"] the largest dx_bar over the systems the run
    solved"""
    r = SC.ref(name)
    res = run(Adapter(r.o), r.p.state_init, delta_init, floors=True, **OPT)
    res["worst"] = assert_not_marginal(res)
    fl = [p["floor"] for p in res["passes"] if p["floor"] is not None]
    res["floor"] = max(fl) if fl else 0.0
    res["bar"] = SC.dx_bar(res["floor"])
    res["repro"] = reproducibility(name, delta_init, res)
    return res


def reproducibility(name, delta_init, res=None):
    """(same step and accept strings, max|state difference|, relative J_final difference) of the restatement's run
    with the band solver against the one with the dense solver"""
    r = SC.ref(name)
    a = res if res is not None else run(Adapter(r.o), r.p.state_init, delta_init, **OPT)
    b = run(DenseAdapter(r.o), r.p.state_init, delta_init, **OPT)
    return ((a["steps"], a["accepted"]) == (b["steps"], b["accepted"]), float(np.abs(a["state"] - b["state"]).max()),
            abs(a["J_final"] - b["J_final"]) / b["J_final"])


def unobserved_tail(p, n_last=10):
    """p (an IMU-less problem) without the views of its last n_last frames: the last coefficients then have no term,
    their blocks are exactly zero and the system is singular at lambda = 0"""
    return SC.drop(p, lambda f, c: f < p.n_frames - n_last)
