"""Restatement of the dog-leg trust-region policy (aslam_backend DogLegTrustRegionPolicy.cpp:11-161 inside the
Optimizer2 loop, Optimizer2.cpp:183-273, TrustRegionPolicy.cpp:29-52) over the CPU oracle's primitives (cost, arrow,
solve(A, 0.0), apply_update): the checker of tests/test_gpu_dogleg.py and tests/test_host_dogleg.py.  The oracle itself
has no dog-leg.  Includes the two deviations of the project's policy: delta_init, and a GN step that counts as held
only after a completed solve (a failed solve is retried on the next, again failed, iteration)."""
import math

import numpy as np

SD, GN, DL = 0, 1, 2
STEP = "SGD"  # step string letters by type: S(D), G(N), D(L)


def _sum(v):
    """left-to-right sum (numpy's own sum is pairwise): the order of a plain C++ loop, so that the host class's
    arithmetic is restated to the last bit"""
    v = np.asarray(v, dtype=np.float64).ravel()
    return float(np.cumsum(v)[-1]) if v.size else 0.0


def _norm(v):
    return math.sqrt(_sum(v * v))


def g_h_g(A):
    """g^T (J^T J) g from the arrow blocks: g_c^T H_cc g_c + sum_f (g_f^T H_ff g_f + 2 g_f^T H_fc g_c), summed in
    the order of the test driver's loops (camera block row by row, then per frame row its H_ff and H_fc terms)."""
    gc, gf = A["gc"], A["gf"]
    cc = (gc[:, None] * A["Hcc"]) * gc[None, :]
    ff = (gf[:, :, None] * A["Hff"]) * gf[:, None, :]
    fc = ((2.0 * gf[:, :, None]) * A["Hfc"]) * gc[None, None, :]
    return _sum(np.concatenate([cc.ravel(), np.concatenate([ff, fc], axis=2).ravel()]))


def steepest_descent(A):
    """(g, sd_scale, dx_sd, |dx_sd|) of an arrow system (:70-75)."""
    g = A["rhs"]
    sd_scale = _sum(g * g) / g_h_g(A)
    dx_sd = sd_scale * g
    return g, sd_scale, dx_sd, _norm(dx_sd)


def select(delta, J, sd_scale, dx_sd, sdn, dx_gn, gnn):
    """Step selection (:82-137) for a held system; dx_gn may be None when the SD branch is taken.  Returns
    dict(type, delta, beta, L0, dx, compared=[(norm, delta), ...])."""
    out = dict(beta=None, compared=[])
    if delta != 0:
        out["compared"].append((sdn, delta))
    if sdn >= delta and delta != 0:
        out.update(type=SD, dx=delta / sdn * dx_sd, L0=delta * (2 * sdn - delta) / (2 * sd_scale), delta=delta)
        return out
    if delta == 0:
        delta = _norm(dx_sd + 0.5 * (dx_gn - dx_sd))
    out["compared"].append((gnn, delta))
    if gnn <= delta:
        out.update(type=GN, dx=dx_gn.copy(), L0=J, delta=delta)
        return out
    d = dx_gn - dx_sd
    n2 = _sum(d * d)
    c = _sum(dx_sd * d)
    r = delta * delta - sdn * sdn
    if c <= 0:
        beta = (-c + math.sqrt(c * c + n2 * r)) / n2
    else:
        beta = r / (c + math.sqrt(c * c + n2 * r))
    # the reference's first L0 term carries the integer expression 1/2 = 0 (:134)
    out.update(type=DL, dx=dx_sd + beta * d, L0=beta * (2 - beta) * J, delta=delta, beta=beta)
    return out


def run(oracle, state0, delta_init=0.0, eps_x=1e-3, eps_j=1.0, max_iterations=25):
    """The Optimizer2 loop with the policy.  Returns dict(passes=[dict per pass], iterations, failed_iterations,
    linear_solver_failure, J_start, J_final, state, steps (string), accepted (string))."""
    state = np.array(state0, dtype=np.float64)
    J = oracle.cost(state)
    p_J = J
    res = dict(J_start=J, passes=[])
    dX, dJ = eps_x + 1.0, eps_j + 1.0
    prev_failed = lin_fail = False
    it = failed = 0
    # TrustRegionPolicy / DogLeg state
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
        rec = dict(rho=None)
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
            A = oracle.arrow(state)
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


def assert_not_marginal(res):
    """A test must not hide a marginal decision: on the restatement's own run |dJ| / J >= 1e-7 on every pass, rho at
    least 1e-4 away from 0, 0.25 and 0.75, and |dx_sd|, |dx_gn| at least 1e-3 (relative) away from delta wherever they
    are compared."""
    worst = dict(dJ=float("inf"), rho=float("inf"), norm=float("inf"))
    for k, p in enumerate(res["passes"]):
        if p["dJ_rel"] is not None:
            worst["dJ"] = min(worst["dJ"], p["dJ_rel"])
            assert p["dJ_rel"] >= 1e-7, (k, p["dJ_rel"])
        if p["rho"] is not None and not math.isnan(p["rho"]):
            m = min(abs(p["rho"] - t) for t in (0.0, 0.25, 0.75))
            worst["rho"] = min(worst["rho"], m)
            assert m >= 1e-4, (k, p["rho"])
        for n, d in p["compared"]:
            m = abs(n - d) / d
            worst["norm"] = min(worst["norm"], m)
            assert m >= 1e-3, (k, n, d)
    return worst
