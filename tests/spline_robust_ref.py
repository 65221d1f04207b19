"""Restatement of robust terms on the spline path, in numpy over the CPU oracle's per-term primitives
(SplineOracle.reproj_dense, imu_dense, apply_update): the checker of tests/test_gpu_spline_robust.py.  The oracle itself
has no weights.  tests/robust_ref.Robust with the spline problem's three term families:

  reprojection  one term per corner,           s = e^T invR e,  rows sqrt(w) L^T [J | e]   (invR = L L^T)
  gyro          one 3-row term per IMU sample,  s = |e_g|^2 of the whitened residual, rows sqrt(w) [J | e]
  accel         likewise on rows 3..5 of the sample

each with its own estimator (kind, param); cost = sum w s over the three families; H = A^T A, rhs = -A^T b over the
stacked rows; weights at the state that is linearised.  The motion term and the position priors take no estimator and
are not restated here (the oracle given to SplineRobust has neither): the device test checks that they compose.
"""
import dataclasses
import functools

import numpy as np

from . import robust_ref as RR
from . import spline_cases as SC
from .robust_ref import CAUCHY, HUBER, NONE  # noqa: F401

FAMILIES = ("reprojection", "gyro", "accel")
# the settings of every check: a 0.3 px reprojection sigma, Huber k / Cauchy sigma^2 per family, the contamination seed
INVR = [1.0 / 0.3 ** 2, 0.0, 1.0 / 0.3 ** 2]
HUBER_ALL = {"reprojection": (HUBER, 2.5), "gyro": (HUBER, 3.0), "accel": (HUBER, 3.0)}
CAUCHY_ALL = {"reprojection": (CAUCHY, 9.0), "gyro": (CAUCHY, 16.0), "accel": (CAUCHY, 16.0)}
SEED = 7


def contaminate_spline(p, seed=SEED):
    """gross outliers: 3 % of the corners shifted 20 .. 60 px in a random direction, 2 % of the gyro and of the accel
    samples offset by N(0, (100 sigma)^2) per axis (fixed seed)"""
    q = RR.contaminate(p, seed)[0] if p.n_corners else p
    rng = np.random.default_rng(seed + 1)
    M = p.n_imu
    if M == 0:
        return q
    gy, ac = np.array(p.imu_gyro, dtype=np.float64, copy=True), np.array(p.imu_acc, dtype=np.float64, copy=True)
    for arr, sig in ((gy, p.sigma_gyro), (ac, p.sigma_acc)):
        idx = rng.choice(M, size=max(1, int(round(0.02 * M))), replace=False)
        arr[idx] += rng.normal(0.0, 100.0 * sig, (idx.size, 3))
    return dataclasses.replace(q, imu_gyro=gy, imu_acc=ac)


def random_invR(n, seed=3):
    """[n][3]: correlated SPD 2x2 matrices, principal sigmas in 0.2 .. 0.6 px at a random angle"""
    rng = np.random.default_rng(seed)
    s1, s2, th = rng.uniform(0.2, 0.6, n), rng.uniform(0.2, 0.6, n), rng.uniform(0.2, 1.3, n)
    c, s = np.cos(th), np.sin(th)
    ia, ib = 1.0 / (s1 * s1), 1.0 / (s2 * s2)
    return np.stack([ia * c * c + ib * s * s, (ia - ib) * c * s, ia * s * s + ib * c * c], axis=1)


class SplineRobust(RR.Robust):
    """The weighted spline problem over one SplineOracle: kinds = {family: (kind, param)} (absent: none), invR3 (None |
    [a, b, c] | [n_corners][3]); perm_seed: sum the rows in that random order (the restatement's own reproducibility)."""

    def __init__(self, oracle, kinds=None, invR3=None, cache=None, perm_seed=None):
        assert not oracle.P.motion_W and oracle.P.n_pos == 0
        kinds = dict(kinds or {})
        assert set(kinds) <= set(FAMILIES)
        self.kinds = {f: kinds.get(f, (NONE, 0.0)) for f in FAMILIES}
        super().__init__(oracle, self.kinds["reprojection"][0], self.kinds["reprojection"][1], invR3, cache)
        self.M, self.ncols, self.K = oracle.prob.n_imu, oracle.ncols, oracle.K
        self.invR3, self.perm_seed = invR3, perm_seed

    def _dense(self, state):
        """(Jr [n][2][ncols], er [n][2], Ji [M][6][ncols], ei [M][6]) at state, cached (the last two states)"""
        key = np.asarray(state, dtype=np.float64).tobytes()
        if key not in self.cache:
            while len(self.cache) >= 2:
                self.cache.pop(next(iter(self.cache)))
            p, o = self.o.prob, self.o
            Jr, er = np.zeros((self.n, 2, self.ncols)), np.zeros((self.n, 2))
            for v in range(p.n_views):
                a, b = int(p.view_offset[v]), int(p.view_offset[v + 1])
                for k in range(b - a):
                    er[a + k], Jr[a + k] = o.reproj_dense(state, v, k)
            Ji, ei = np.zeros((self.M, 6, self.ncols)), np.zeros((self.M, 6))
            for m in range(self.M):
                ei[m], Ji[m] = o.imu_dense(state, m)
            self.cache[key] = (Jr, er, Ji, ei)
        return self.cache[key]

    def terms(self, state):
        """per family (J [n][rows][ncols], b [n][rows], s [n], w [n]): J and b are the whitened rows L^T [J | e]
        before the weight"""
        Jr, er, Ji, ei = self._dense(state)
        LT = np.transpose(self.L, (0, 2, 1))
        fam = {"reprojection": (np.einsum("nij,njk->nik", LT, Jr), np.einsum("nij,nj->ni", LT, er)),
               "gyro": (Ji[:, :3], ei[:, :3]), "accel": (Ji[:, 3:], ei[:, 3:])}
        out = {}
        for f, (J, b) in fam.items():
            s = np.einsum("ni,ni->n", b, b)
            out[f] = (J, b, s, RR.weight(self.kinds[f][0], self.kinds[f][1], s))
        return out

    def family_sw(self, state):
        """{family: (s, w)} at state, upload order"""
        return {f: (t[2], t[3]) for f, t in self.terms(state).items()}

    def _order(self, n):
        return np.arange(n) if self.perm_seed is None else np.random.default_rng(self.perm_seed).permutation(n)

    def cost(self, state):
        """sum w(s) s over the three families"""
        ws = np.concatenate([t[3] * t[2] for t in self.terms(state).values()])
        return float(np.sum(ws[self._order(ws.size)]))

    def system(self, state, use_mestimator=True):
        """dict(H dense, rhs, cost, sw {family: (s, w)}, Hcc, Hsc [6K][C], Hband [K][4][6][6], gc, gs)"""
        assert use_mestimator
        T = self.terms(state)
        A = np.concatenate([(np.sqrt(w)[:, None, None] * J).reshape(-1, self.ncols) for J, b, s, w in T.values()])
        b = np.concatenate([(np.sqrt(w)[:, None] * b).reshape(-1) for J, b, s, w in T.values()])
        o = self._order(b.size)
        A, b = A[o], b[o]
        H = A.T @ A
        rhs = -(A.T @ b)
        gabs = np.abs(A).T @ np.abs(b)  # the scale of rhs's summands (rhs itself cancels to ~0 at a converged state)
        C, K = self.C, self.K
        Hband = np.zeros((K, 4, 6, 6))
        for k in range(K):
            for d in range(min(4, K - k)):
                Hband[k, d] = H[C + 6 * k:C + 6 * k + 6, C + 6 * (k + d):C + 6 * (k + d) + 6]
        return dict(H=H, rhs=rhs, cost=self.cost(state), sw={f: (t[2], t[3]) for f, t in T.items()}, Hcc=H[:C, :C],
                    Hsc=H[C:, :C], Hband=Hband, gc=rhs[:C], gs=rhs[C:],
                    gscale=dict(gc=gabs[:C].max(), gs=gabs[C:].max(), rhs=gabs.max()))


def variants(n_corners):
    """(tag, kinds, invR3) of the one-step checks: uniform invR and per-corner correlated invR, Huber and Cauchy on all
    three families, one family at a time"""
    return [("huber+invR", HUBER_ALL, INVR),
            ("cauchy+invR[n]", CAUCHY_ALL, random_invR(n_corners)),
            ("huber reprojection", {"reprojection": HUBER_ALL["reprojection"]}, None),
            ("huber gyro", {"gyro": HUBER_ALL["gyro"]}, None),
            ("cauchy accel", {"accel": CAUCHY_ALL["accel"]}, None)]


# The one-step cases and their three states: 0 state_init, 1 the restatement's converged Huber state, 2 its state after
# two passes of that run (a mixed state: 8 .. 16 % of the corners in Huber's tail, and a real step for every variant).
# Which solves are compared is decided here, from the restatement's own floors (its dx from H against its dx from H summed
# in three permuted orders; measured on n7, views, c51, imu_sparse, imu_none, asserted in tests/test_spline_robust_ref.py):
#   lambda = 10  floors <= 4.2e-9 at states 0 and 2 and, at state 1, <= 1.6e-9 for every variant but huber+invR: compared.
#                huber+invR at state 1 is at its own fixed point: its gradient is 3e-8 .. 5e-4 of its summands
#                (cancels()), dx is rounding noise (floors 8e-9 .. 2.8e-7) and takes no comparison there; state 2 is
#                where that variant's solve is compared.
#   lambda = 0   floors <= 8.4e-9 at state_init: compared where the case has gn.  At states 1 and 2 they lie between
#                4e-9 and 3e-7 for every variant, on either side of spline_cases.FLOOR_MAX from one permutation or BLAS
#                to the next (c51 huber+invR: 6.7e-8 on one machine, 1.4e-6 on another): the precondition of the
#                100 x floor bar is undecided there, so, as with spline_cases.LM_REPRO_MAX, the restatement does not
#                referee it.  The lambda = 0 solves near convergence are covered by the GN runs.
STEP_CASES = ["n7", "views", "c51", "imu_sparse", "imu_none"]
MID_PASSES = 2


def cancels(tag, which):
    """the gradient of variant `tag` at state `which` is what cancellation leaves of its summands (< 1e-3 of their
    scale; everywhere else >= 1e-3: asserted in tests/test_spline_robust_ref.py)"""
    return tag == "huber+invR" and which == 1


def step_lambdas(name, which, tag):
    """the conditioners of the one-step solves of case `name`, variant `tag`, that are compared at state `which`"""
    if which == 0:
        return (10.0, 0.0) if SC.BY_NAME[name].gn else (10.0,)
    return () if cancels(tag, which) else (10.0,)


LM_OPT = dict(lambda0=10.0, max_iterations=20, eps_x=1e-3, eps_j=1.0)  # SplineSolver.optimize's defaults
PERM_SEED = 5
FLOOR_SEEDS = (5, 6, 7)


class Ref:
    """The restatement's side of one case of tests/spline_cases.py on the contaminated problem, computed once per
    process: variants over one Jacobian cache, the three states of the one-step checks and the optimize runs."""

    def __init__(self, name):
        from oracle import oracle as O
        self.case = SC.BY_NAME[name]
        self.clean = SC.problem(name)
        self.p = contaminate_spline(self.clean)
        self.o = O.SplineOracle(self.p)
        self.cache, self._runs, self._states = {}, {}, None

    def robust(self, kinds=None, invR3=None, perm_seed=None):
        return SplineRobust(self.o, kinds, invR3, self.cache, perm_seed)

    def run(self, policy, kinds_name="huber", perm_seed=None):
        """(final state, result) from state_init with Huber or Cauchy on all three families and the uniform INVR: GN
        with spline_cases.OPT, LM with LM_OPT (with eps_j = 1e-3 the restatement's last LM steps have dJ / J of
        1e-9 .. 1e-8, marginal on every case tried)"""
        key = (policy, kinds_name, perm_seed)
        if key not in self._runs:
            kinds = HUBER_ALL if kinds_name == "huber" else CAUCHY_ALL
            opt = LM_OPT if policy == "lm" else SC.OPT
            self._runs[key] = self.robust(kinds, INVR, perm_seed).optimize(self.p.state_init, policy=policy, **opt)
        return self._runs[key]

    def states(self):
        """the three states of every one-step check: state_init, the restatement's converged Huber state (its GN
        run's; its LM run's where the case takes no lambda = 0 solve) and its state after MID_PASSES passes of that run"""
        if self._states is None:
            pol = "gn" if self.case.gn else "lm"
            opt = dict(LM_OPT if pol == "lm" else SC.OPT, max_iterations=MID_PASSES)
            mid, res = self.robust(HUBER_ALL, INVR).optimize(self.p.state_init, policy=pol, **opt)
            assert res["iterations"] == MID_PASSES and res["failed_iterations"] == 0
            self._states = [self.p.state_init, self.run(pol)[0], mid]
        return self._states

    def floors(self, r, state, lams):
        """{lam: (ok, dx, floor)}: the restatement's dx and its own error, the largest difference of that dx from the dx
        of H summed in the permuted orders of FLOOR_SEEDS (relative)"""
        s0 = r.system(state)
        perm = [SplineRobust(self.o, r.kinds, r.invR3, self.cache, seed).system(state) for seed in FLOOR_SEEDS]
        out = {}
        for lam in lams:
            ok, dx = r.solve(s0, lam)
            fl = 0.0
            for sp in perm:
                ok_p, dx_p = r.solve(sp, lam)
                ok = ok and ok_p
                fl = max(fl, SC.rel(dx_p, dx)) if ok else float("inf")
            out[lam] = (ok, dx, fl)
        return out


@functools.lru_cache(maxsize=None)
def ref(name):
    return Ref(name)


def apply_settings(g, kinds=None, invR3=None):
    """the same settings on a capi.SplineSolver"""
    for f in FAMILIES:
        kind, param = (kinds or {}).get(f, (NONE, 0.0))
        g.set_mestimator(f, kind, param)
    g.set_corner_invR(invR3)
