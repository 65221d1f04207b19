"""Restatement of robust reprojection terms (aslam_backend: MEstimatorPolicies.cpp, ErrorTerm.cpp:20-24,
ErrorTerm.hpp(impl):118-127 and 170-192) and of the Optimizer2 loop over them (Optimizer2.cpp:183-273 with
LevenbergMarquardtTrustRegionPolicy.cpp:50-113 and GaussNewtonTrustRegionPolicy.cpp:18-39), in numpy over the CPU
oracle's primitives (dense_jacobian, apply_update): the checker of tests/test_gpu_robust.py.  The oracle itself has no
weights.

A term has the raw squared error s = e^T invR e and the weight w = getWeight(s); the cost is sum w s (always
weighted); the system is H = sum w J^T invR J, rhs = -sum w J^T invR e with the M-estimator factor applied only
under useMEstimator.  The weights are evaluated at the state that is linearised (inside Optimizer2 the reference's
cached squared error is that state's).
"""
import dataclasses
import math

import numpy as np

NONE, HUBER, CAUCHY, GEMAN_MCCLURE, BLAKE_ZISSERMAN = "none", "huber", "cauchy", "geman_mcclure", "blake_zisserman"


def blake_zisserman_epsilon(df, p_cut, w_cut):
    """computeEpsilon (MEstimatorPolicies.cpp:116-119); chi2^-1(p, 2) = -2 ln(1 - p)"""
    assert df == 2
    return (1.0 - w_cut) / w_cut * math.exp(2.0 * math.log(1.0 - p_cut))


def weight(kind, param, s):
    """getWeight(s) of MEstimatorPolicies.cpp, elementwise"""
    s = np.asarray(s, dtype=np.float64)
    if kind in (None, NONE):
        return np.ones_like(s)
    if kind == HUBER:  # :64-66
        with np.errstate(divide="ignore"):
            return np.where(s < param * param, 1.0, param / np.sqrt(s))
    if kind == CAUCHY:  # :46-49
        return 1.0 / (1.0 + s / param)
    if kind == GEMAN_MCCLURE:  # :31-34
        se = param + s
        return param / (se * se)
    if kind == BLAKE_ZISSERMAN:  # :104-106
        ex = np.exp(-s)
        return ex / (ex + param)
    raise ValueError(kind)


def invR_matrices(invR3, n):
    """[n][2][2] from None, one [a, b, c] or [n][3]"""
    if invR3 is None:
        return np.broadcast_to(np.eye(2), (n, 2, 2)).copy()
    a = np.asarray(invR3, dtype=np.float64).reshape(-1, 3)
    if a.shape[0] == 1:
        a = np.broadcast_to(a, (n, 3))
    assert a.shape[0] == n
    R = np.empty((n, 2, 2))
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1] = a[:, 0], a[:, 1], a[:, 1], a[:, 2]
    return R


def contaminate(prob, seed, frac=0.03, lo=20.0, hi=60.0):
    """gross outliers: frac of the corners shifted by lo .. hi px in a random direction (fixed seed)"""
    rng = np.random.default_rng(seed)
    n = prob.n_corners
    idx = rng.choice(n, size=max(1, int(round(frac * n))), replace=False)
    r = rng.uniform(lo, hi, idx.size)
    th = rng.uniform(0.0, 2.0 * math.pi, idx.size)
    y = np.array(prob.y, dtype=np.float64, copy=True)
    y[idx, 0] += r * np.cos(th)
    y[idx, 1] += r * np.sin(th)
    return dataclasses.replace(prob, y=y), np.sort(idx)


class Robust:
    """The weighted problem over one Oracle: estimator (kind, param) and invR3 (None | [a, b, c] | [n][3])."""

    def __init__(self, oracle, kind=NONE, param=0.0, invR3=None, cache=None):
        """cache: a dict shared by the variants over one oracle; it keeps (J, e) of the last two states, so variants
        evaluated at the same state (and a candidate's cost followed by its system) form the Jacobian once"""
        self.o = oracle
        self.cache = cache if cache is not None else {}
        self.kind, self.param = kind, param
        self.n = oracle.prob.n_corners
        self.R = invR_matrices(invR3, self.n)
        self.L = np.linalg.cholesky(self.R)  # invR = L L^T (only invR enters the result)
        self.C, self.F = oracle.C, oracle.prob.n_frames

    def terms(self, state):
        """(J [n][2][ncols], e [n][2], s [n], w [n]) at state"""
        key = np.asarray(state, dtype=np.float64).tobytes()
        if key not in self.cache:
            while len(self.cache) >= 2:
                self.cache.pop(next(iter(self.cache)))
            J, e = self.o.dense_jacobian(state)
            self.cache[key] = (J.reshape(self.n, 2, -1), e.reshape(self.n, 2))
        J, e = self.cache[key]
        s = np.einsum("ni,nij,nj->n", e, self.R, e)
        return J, e, s, weight(self.kind, self.param, s)

    def errors(self, state):
        """(e, s, w) at state"""
        _, e, s, w = self.terms(state)
        return e, s, w

    def cost(self, state):
        """sum w(s) s (ErrorTerm.cpp:20-24)"""
        _, s, w = self.errors(state)
        return float(np.sum(w * s))

    def system(self, state, use_mestimator=True):
        """dict(H dense, rhs, cost, s, w, Hcc, Hfc [F][6][C], Hff [F][6][6], gc, gf) with rows sqrt(w) L^T [J | e]"""
        J, e, s, w = self.terms(state)
        sw = np.sqrt(w) if use_mestimator else np.ones_like(w)
        LT = np.transpose(self.L, (0, 2, 1)) * sw[:, None, None]
        A = np.einsum("nij,njk->nik", LT, J).reshape(2 * self.n, -1)
        b = np.einsum("nij,nj->ni", LT, e).reshape(-1)
        H = A.T @ A
        rhs = -(A.T @ b)
        C, F = self.C, self.F
        Hfc = np.stack([H[C + 6 * f:C + 6 * f + 6, :C] for f in range(F)])
        Hff = np.stack([H[C + 6 * f:C + 6 * f + 6, C + 6 * f:C + 6 * f + 6] for f in range(F)])
        return dict(H=H, rhs=rhs, cost=float(np.sum(w * s)), s=s, w=w, Hcc=H[:C, :C], Hfc=Hfc, Hff=Hff, gc=rhs[:C],
                    gf=rhs[C:].reshape(F, 6))

    @staticmethod
    def solve(sysd, lam):
        """(ok, dx) of (H + lam^2 I) dx = rhs, densely; ok = positive definite (CHOLMOD's failure semantics)"""
        H = sysd["H"] + lam * lam * np.eye(sysd["H"].shape[0])
        try:
            np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            return False, None
        return True, np.linalg.solve(H, sysd["rhs"])

    def optimize(self, state0, policy="lm", lambda0=10.0, max_iterations=200, eps_x=1e-3, eps_j=1.0):
        """Optimizer2::optimize (Optimizer2.cpp:183-273), statement by statement as the oracle's kbo_optimize restates
        it; buildSystem(.., true) / evaluateError(true) as the LM and GN policies call them.  Returns (state, res) with
        res: J_start, J_final, iterations, failed_iterations, linear_solver_failure, trace [n][4] (J, lambda, deltaX,
        accepted) and passes (per pass: rho, dJ, dX for the marginality check)."""
        lm = policy == "lm"
        st = np.array(state0, dtype=np.float64)
        J = self.cost(st)
        p_J = J
        res = dict(J_start=J, iterations=0, failed_iterations=0, linear_solver_failure=0, passes=[])
        dX, dJ = eps_x + 1.0, eps_j + 1.0
        prev_failed = lin_fail = False
        pol_J = pol_pJ = last_succ = J  # optimizationStarting (TrustRegionPolicy.cpp:30-37; LM :38-46)
        first = True
        lam, gamma, beta, mu, pexp = lambda0, 3.0, 2.0, 2.0, 3
        trace = []
        A = dx = None
        while res["iterations"] < max_iterations and res["failed_iterations"] < max_iterations and (
                (dX > eps_x and abs(dJ) > eps_j) or lin_fail):
            if prev_failed:
                pol_J = J
            else:
                pol_pJ, last_succ, pol_J = last_succ, J, J
            rec = dict(rho=None, built=False, lm=lm)
            if lm:  # LevenbergMarquardtTrustRegionPolicy.cpp:50-113
                if first:
                    A = self.system(st, True)
                    rec["built"] = True
                else:
                    d2 = float(np.cumsum(dx * (lam * dx + A["rhs"]))[-1])
                    rho = (pol_pJ - pol_J) / d2
                    rec["rho"] = rho
                    if prev_failed:
                        mu *= 2
                        lam *= mu
                    elif rho <= 0:
                        mu *= 10
                        lam *= mu
                    else:
                        A = self.system(st, True)
                        rec["built"] = True
                        if lam > 1e-16:
                            u1 = 1 / gamma
                            u2 = 1 - (beta - 1) * (2 * rho - 1) ** pexp
                            lam *= u1 if u1 > u2 else u2
                            mu = beta
                        else:
                            lam = 1e-15
                ok, sol = self.solve(A, lam)
                if ok:
                    dx = sol
            else:  # GaussNewtonTrustRegionPolicy.cpp:18-39
                A = self.system(st, True)
                rec["built"] = True
                ok, dx = self.solve(A, 0.0)
            first = False
            accepted = 0
            if not ok:
                prev_failed = lin_fail = True
                res["linear_solver_failure"] = 1
                res["failed_iterations"] += 1
            else:
                cand, dX = self.o.apply_update(st, dx)
                J = self.cost(cand)
                dJ = p_J - J
                rec.update(dJ=dJ, dX=dX, J=J, p_J=p_J)
                if lm and dJ < 0.0:
                    res["failed_iterations"] += 1  # revertLastStateUpdate (Optimizer2.cpp:313-318)
                    prev_failed = True
                else:
                    st, p_J, prev_failed, accepted = cand, J, False, 1
                res["iterations"] += 1
            trace.append([J if ok else float("nan"), lam if lm else 0.0, dX, accepted])
            rec["accepted"] = accepted
            res["passes"].append(rec)
        res.update(J_final=p_J, trace=np.array(trace).reshape(-1, 4))
        return st, res


def assert_not_marginal(res, eps_x, eps_j):
    """No decision of the restatement's own run may be marginal: dJ at least 1e-7 (relative to J) away from 0 (the
    accept test), |dJ| 1e-3 (relative) away from eps_j and dX 1e-3 (relative) away from eps_x (the convergence tests),
    and the LM gain ratio rho at least 1e-4 away from 0 (its branch)."""
    worst = dict(dJ=float("inf"), eps_j=float("inf"), eps_x=float("inf"), rho=float("inf"))
    for k, p in enumerate(res["passes"]):
        if "dJ" in p:
            if p["lm"]:  # the Gauss-Newton policy accepts every step
                worst["dJ"] = min(worst["dJ"], abs(p["dJ"]) / p["p_J"])
            worst["eps_j"] = min(worst["eps_j"], abs(abs(p["dJ"]) - eps_j) / eps_j)
            worst["eps_x"] = min(worst["eps_x"], abs(p["dX"] - eps_x) / eps_x)
        if p["rho"] is not None and math.isfinite(p["rho"]):
            worst["rho"] = min(worst["rho"], abs(p["rho"]))
    assert worst["dJ"] >= 1e-7 and worst["eps_j"] >= 1e-3 and worst["eps_x"] >= 1e-3 and worst["rho"] >= 1e-4, worst
    return worst
