"""The reference side of the spline path's covariance query (kb_sp_covariance / kb_sp_curve_covariance),
shared by test_spline_cov_ref.py (the preconditions, from the oracle alone) and test_gpu_spline_cov.py (the device
against it).

Reference: the dense H + lambda^2 I assembled from SplineOracle.system's blocks, inverted after Jacobi equilibration,
Sigma_ref = D^-1 inv(D^-1 H D^-1) D^-1 with D = sqrt(diag H), symmetrised.  Its own error, `floor`, is the largest
correlation-normalised difference max |A - Sigma_ref|_ij / sqrt(Sigma_ref,ii Sigma_ref,jj) over three other float64
inverses of the same matrix: the equilibrated one under the reversal permutation, plain numpy.linalg.inv, and plain inv
under the permutation (the unscaled ones stand for what an unscaled factorisation such as the device's can lose).  The
bar on the device is spline_cases.dx_bar(floor) = max(1e-8, 100 floor), the project's rule for the spline solves; the
precondition floor <= spline_cases.FLOOR_MAX caps it at 1e-5.

Which (case, state, lambda) are compared is the table below, written out; test_spline_cov_ref.py checks every entry's
preconditions and the table's coverage without a device, and nothing is filtered at run time on the GPU.
"""
import functools

import numpy as np

from . import spline_cases as SC

# ---- the table: (state, lambda) -> the cases compared there ----
# state "init": problem.state_init; "s1": the oracle's state after one GN step from it (spline_cases.Ref.states[1]).
# Left out (the reference's own floor above FLOOR_MAX, or H + lambda^2 I not positive definite):
#   init, 1:  imu_none
#   init, 0:  n2a, c48, n33, imu_none; n2b sits at the limit and is left out rather than tuned for
#   s1, 10:   c23, n33, n35 (and the three cases that take no GN step)
_NOT_L1 = {"imu_none"}
_NOT_L0 = {"n2a", "n2b", "c48", "n33", "imu_none"}
_NOT_S1 = {"c23", "n33", "n35"}
TABLE = {
    ("init", 10.0): tuple(SC.NAMES),
    ("init", 1.0): tuple(n for n in SC.NAMES if n not in _NOT_L1),
    ("init", 0.0): tuple(n for n in SC.NAMES if n not in _NOT_L0),
    ("s1", 10.0): tuple(n for n in SC.GN_NAMES if n not in _NOT_S1),
}
ENTRIES = [(name, which, lam) for (which, lam), names in TABLE.items() for name in names]
COVERAGE = {("init", 10.0): len(SC.NAMES), ("init", 1.0): 26, ("init", 0.0): 22, ("s1", 10.0): 18}


def state_of(r, which):
    return r.p.state_init if which == "init" else r.states[1]


def system_of(r, which):
    return r.sys0 if which == "init" else r.o.system(r.states[1], nthreads=4)


# ---- dense algebra ----
def dense(sysd, lam):
    """H + lambda^2 I, columns [theta (C) | coefficients (6 K)], from the blocks of SplineOracle.system /
    SplineSolver.system (Hband[k][d] = block (k, k + d))"""
    Hcc, Hsc, Hb = sysd["Hcc"], sysd["Hsc"], sysd["Hband"]
    C, K = Hcc.shape[0], Hb.shape[0]
    H = np.zeros((C + 6 * K, C + 6 * K))
    H[:C, :C] = Hcc
    H[C:, :C] = Hsc
    H[:C, C:] = Hsc.T
    for k in range(K):
        for d in range(min(Hb.shape[1], K - k)):
            a, b = C + 6 * k, C + 6 * (k + d)
            H[a:a + 6, b:b + 6] = Hb[k, d]
            if d:
                H[b:b + 6, a:a + 6] = Hb[k, d].T
    return H + lam * lam * np.eye(H.shape[0])


def _sym(A):
    return 0.5 * (A + A.T)


def inv_equilibrated(H, perm=None):
    p = np.arange(H.shape[0]) if perm is None else perm
    Hp = H[np.ix_(p, p)]
    s = 1.0 / np.sqrt(np.diag(Hp))
    Sp = _sym(np.linalg.inv(Hp * np.outer(s, s)) * np.outer(s, s))
    out = np.empty_like(Sp)
    out[np.ix_(p, p)] = Sp
    return out


def inv_plain(H, perm=None):
    p = np.arange(H.shape[0]) if perm is None else perm
    out = np.empty_like(H)
    out[np.ix_(p, p)] = _sym(np.linalg.inv(H[np.ix_(p, p)]))
    return out


def corr_diff(A, ref):
    """max |A - ref|_ij / sqrt(ref_ii ref_jj)"""
    s = np.sqrt(np.diag(ref))
    return float((np.abs(A - ref) / np.outer(s, s)).max())


def is_pd(H):
    try:
        np.linalg.cholesky(H)
        return True
    except np.linalg.LinAlgError:
        return False


def reference(H):
    """(Sigma_ref, floor)"""
    rev = np.arange(H.shape[0])[::-1]
    ref = inv_equilibrated(H)
    floor = max(corr_diff(A, ref) for A in (inv_equilibrated(H, rev), inv_plain(H), inv_plain(H, rev)))
    return ref, floor


@functools.lru_cache(maxsize=None)
def entry(name, which, lam):
    """(pd, Sigma_ref, floor) of one (case, state, lambda), computed once per process and not modified"""
    r = SC.ref(name)
    H = dense(system_of(r, which), lam)
    if not is_pd(H):
        return False, None, np.inf
    ref, floor = reference(H)
    ref.setflags(write=False)
    return True, ref, floor


# ---- the device's outputs, cut from a dense Sigma ----
def blocks(S, C, K):
    """dict(Ptt [C][C], Pst [6K][C], Pband [K][4][6][6]) of a dense Sigma in kb_sp_covariance's layouts"""
    Pband = np.zeros((K, 4, 6, 6))
    for k in range(K):
        for d in range(min(4, K - k)):
            Pband[k, d] = S[C + 6 * k:C + 6 * k + 6, C + 6 * (k + d):C + 6 * (k + d) + 6]
    return dict(Ptt=S[:C, :C].copy(), Pst=S[C:, :C].copy(), Pband=Pband)


def scales(S, C, K):
    """sqrt(Sigma_ii Sigma_jj) of every entry of blocks(S, C, K) (1 where Pband holds a structural zero)"""
    s = np.sqrt(np.diag(S))
    st, ss = s[:C], s[C:].reshape(K, 6)
    Pband = np.ones((K, 4, 6, 6))
    for k in range(K):
        for d in range(min(4, K - k)):
            Pband[k, d] = np.outer(ss[k], ss[k + d])
    return dict(Ptt=np.outer(st, st), Pst=np.outer(s[C:], st), Pband=Pband)


def block_errors(dev, S, C, K):
    """{key: max |dev - ref| / sqrt(ref_ii ref_jj)} over the blocks the device returned (None entries skipped)"""
    ref, sc = blocks(S, C, K), scales(S, C, K)
    return {k: float((np.abs(dev[k] - ref[k]) / sc[k]).max()) for k in ref if dev.get(k) is not None}


def curve_ref(S, C, knots, order, times):
    """([n][6][6], scale [n][6][6]): covariance of the curve value sum_a w_a c_{k0+a} at each time, the weights from the
    oracle's bspline_weights (derivative 0), over the dense Sigma; the scale is sqrt(P_ii P_jj)"""
    from oracle import oracle as O
    P = np.zeros((len(times), 6, 6))
    for q, t in enumerate(times):
        k0, w = O.bspline_weights(order, knots, float(t), 0)
        W = np.zeros((6, S.shape[0]))
        for a in range(order):
            W[:, C + 6 * (k0 + a):C + 6 * (k0 + a) + 6] = w[a] * np.eye(6)
        P[q] = W @ S @ W.T
    d = np.sqrt(np.einsum("nii->ni", P))
    return P, d[:, :, None] * d[:, None, :]


# ---- the recursion of DESIGN.md 10e, restated on a generic arrow system ----
def random_arrow(n, b, C, seed):
    """SPD arrow system [theta (C) | n nodes of b], block-tridiagonal over the nodes, dense"""
    rng = np.random.default_rng(seed)
    N = C + n * b
    J = np.zeros((3 * N, N))
    J[:, :C] = rng.standard_normal((3 * N, C))
    rows = np.array_split(np.arange(3 * N), n)
    for i in range(n):  # rows of "node i" touch nodes i, i + 1 and theta
        hi = min(n, i + 2)
        J[np.ix_(rows[i], np.arange(C + i * b, C + hi * b))] = rng.standard_normal((rows[i].size, (hi - i) * b))
    return J.T @ J + 0.5 * np.eye(N)


def elimination_order(n):
    """[(j, s)]: odd multiples of s = 1, 2, 4, .. below n, as k_sp_bvec's j = s + 2 s b"""
    out, s = [], 1
    while s < n:
        out += [(j, s) for j in range(s, n, 2 * s)]
        s *= 2
    return out


def selected_inverse(H, n, b, C):
    """dict(Ptt, St [n][b][C], D [n][b][b], X [n-1][b][b] = Sigma_i,i+1) by the device's walk: eliminate in
    elimination_order (then node 0, then theta) keeping P_j = L^-T L^-1 and E_j = L^-T Z_j per node, then
      Sigma_tt = S^-1,  Sigma_j,N = -E_j Sigma_NN,  Sigma_jj = P_j + E_j Sigma_NN E_j^T
    top node first, then the strides from the widest down.  Sigma_lr is read from whichever of l, r is the odd
    multiple of 2 s (its Sigma_jr, or its Sigma_jl transposed); the adjacent cross blocks are read as the gather
    kernel reads them (odd i: its Sigma_jr; even i: node i + 1's Sigma_jl transposed)."""
    A = H.copy()
    th = np.arange(C)
    nd = lambda i: np.arange(C + i * b, C + (i + 1) * b)  # noqa: E731
    order = elimination_order(n)
    P, E, Nb = {}, {}, {}
    for j, s in order + [(0, 0)]:
        l, r = j - s, j + s
        hl, hr = s > 0, s > 0 and r < n
        L = np.linalg.cholesky(A[np.ix_(nd(j), nd(j))])
        idx = np.concatenate([nd(l) if hl else [], nd(r) if hr else [], th]).astype(int)
        Z = np.linalg.solve(L, A[np.ix_(nd(j), idx)])
        # the structure the device relies on: node j couples to nothing else that is still active
        rest = np.setdiff1d(np.arange(A.shape[0]), np.concatenate([idx, nd(j)]))
        assert np.abs(A[np.ix_(nd(j), rest)]).max(initial=0.0) == 0.0
        A[np.ix_(idx, idx)] -= Z.T @ Z
        A[nd(j), :] = 0.0
        A[:, nd(j)] = 0.0
        Ej = np.zeros((b, 2 * b + C))
        Ej[:, np.concatenate([np.arange(b) if hl else [], b + np.arange(b) if hr else [], 2 * b + th]).astype(int)] = \
            np.linalg.solve(L.T, Z)
        P[j], E[j], Nb[j] = np.linalg.inv(L @ L.T), Ej, (l, r, hl, hr)
    Ptt = np.linalg.inv(A[np.ix_(th, th)])
    D, Sl, Sr, St = {}, {}, {}, {}
    for j, s in [(0, 0)] + order[::-1]:  # strides descending (within a stride the nodes are independent)
        l, r, hl, hr = Nb[j]
        w = 2 * b + C
        SN = np.zeros((w, w))
        SN[2 * b:, 2 * b:] = Ptt
        if hl:
            SN[:b, :b] = D[l]
            SN[:b, 2 * b:] = St[l]
        if hr:
            SN[b:2 * b, b:2 * b] = D[r]
            SN[b:2 * b, 2 * b:] = St[r]
        if hl and hr:
            SN[:b, b:2 * b] = Sr[l] if (l // (2 * s)) & 1 else Sl[r].T
        SN = np.triu(SN) + np.triu(SN, 1).T
        G = E[j] @ SN
        Sl[j], Sr[j], St[j] = -G[:, :b], -G[:, b:2 * b], -G[:, 2 * b:]
        D[j] = P[j] + G @ E[j].T
    X = [Sr[i] if i & 1 else Sl[i + 1].T for i in range(n - 1)]
    return dict(Ptt=Ptt, St=np.stack([St[i] for i in range(n)]), D=np.stack([D[i] for i in range(n)]),
                X=np.stack(X) if X else np.zeros((0, b, b)))
