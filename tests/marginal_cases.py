"""The camera-block widths at which k_marg (the cyclic two-sided Jacobi SVD behind kb_solve_marginal,
kb_analyze_marginal and kb_optimize_marginal[_analyze]) changes its code path, as small rigs, with LAPACK references of
the solve: shared by
test_marginal_cases.py (the preconditions, from synth, the oracle and numpy alone) and test_gpu_marginal_shapes.py (the
device against both references).  No GPU and no HIP import here.

k_marg selects by C alone (kb_solve_layout.h marg_full / marg_lds_doubles, kMargLdsStage = 19000 doubles;
test_solve_layout.py compares the header's figures with the restatements below at every width):
  full     both triangles of Omega in LDS, C padded to an even m (an odd C has a dummy round-robin index: the padding
           row / column), C <= 96; the warm start V0 is staged in LDS up to C = 78 and read from global memory above
  packed   upper triangle only, 97 <= C <= 112; an odd C guards every read / write of the dummy index; V0 from global
  C > 112  beyond the capacity of k_marg's arrays (kMargMaxC) -- kb_create admits no handle of C > 111, so C = 111 is
           the largest width that runs and C = 112 cannot be reached through the C-ABI
regime() restates those three functions; test_marginal_cases.py asserts every row's regime, so a moved constant fails
there and the table is redone.

Every rig is synth.make_problem(models, n_frames, seed, p_view); C = sum of intrinsics + 6 (N - 1).
"""
import functools
from dataclasses import dataclass

import numpy as np

from kalibr_amd import synth

PR, OR, EU, OM, DS, EQ, FV = (synth.PINHOLE_RADTAN, synth.OMNI_RADTAN, synth.EUCM, synth.OMNI, synth.DS,
                              synth.PINHOLE_EQUI, synth.PINHOLE_FOV)
EPS = float(np.finfo(float).eps)

# ---- kb_solve_layout.h / kb_device.h, restated ----
K_MARG_LDS_STAGE = 19000
K_MARG_MAX_C = 112
K_MARG_FULL_MAX_C = 96
K_MARG_WARM_MAX = 32
FULL_STAGED, FULL_GLOBAL, PACKED, REFUSED = "full + staged V0", "full + V0 from global", "packed", "refused"


def marg_full(C):
    m = C + (C & 1)
    return m * m + C * m + 2 * C <= K_MARG_LDS_STAGE


def marg_lds_doubles(C):
    """(doubles of dynamic LDS, whether V0 is staged in LDS)"""
    m = C + (C & 1)
    base = m * m + C * m + 2 * C if marg_full(C) else C * (C + 1) // 2 + C * C + 2 * C
    stage = base + C * C <= K_MARG_LDS_STAGE
    return (base + C * C if stage else base), stage


# sizeof(ChainLds) (kb_solve_layout.h kChainLdsBytes; a static_assert beside the struct in kb_kernels.hip holds it to
# this): the gated tail's chains take the start of the dynamic LDS
CHAIN_LDS_BYTES = 8 * (16 * 12 + 64 * 12)
# k_marg's own static LDS arrays as declared (doubles: dg, ap 2 x 112 each, wsort, tco 112 each, stat 4, nbase 16 x 7;
# ints: perm 112), and what only full storage keeps (csr 2 x 112 doubles, prodkl, prodsel 64 ints each)
K_MARG_STATIC_MIN = 8 * (4 * 112 + 2 * 112 + 4 + 16 * 7) + 4 * 112
K_MARG_STATIC_FULL_ONLY = 8 * 2 * 112 + 4 * 2 * 64
LDS_BYTES = 160 * 1024                     # per workgroup on gfx950


def marg_lds_bytes(C):
    return max(8 * marg_lds_doubles(C)[0], CHAIN_LDS_BYTES)


def marg_threads(C):
    """one thread per 2 x 2 block of pairs (h (h + 1) / 2, h = ceil(C / 2)) and per (row of V, pair) (C h), in whole
    waves, at most 1024"""
    h = (C + 1) // 2
    return min(-(-(h * (h + 1) // 2 + C * h) // 64) * 64, 1024)


def marg_block(C):
    """k_marg's block: full storage adds wave 0 for the rotations"""
    return min(marg_threads(C) + (64 if marg_full(C) else 0), 1024)


def regime(C):
    if C > K_MARG_MAX_C:
        return REFUSED
    if not marg_full(C):
        return PACKED
    return FULL_STAGED if marg_lds_doubles(C)[1] else FULL_GLOBAL


@dataclass(frozen=True)
class Row:
    C: int
    models: tuple
    n_frames: int
    regime: str
    what: str
    seed: int = 77
    p_view: float = 0.8
    svd_tol: float = 1.0  # variant (c): the fixed tolerance on the unscaled singular values (pixel^2 per unit^2)


ROWS = {r.C: r for r in (
    Row(5, (FV,), 24, FULL_STAGED, "smallest odd C: m = 6, h = 3", p_view=1.0),
    Row(9, (OR,), 24, FULL_STAGED, "odd, a true null direction", p_view=1.0),
    Row(23, (PR, OR), 24, FULL_STAGED, "odd, two cameras"),
    Row(77, (PR, PR, PR, OR, OR, FV), 24, FULL_STAGED, "last odd C with V0 staged"),
    Row(79, (PR,) * 5 + (OR,), 24, FULL_GLOBAL, "first C with V0 read from global memory, odd"),
    Row(87, (PR,) * 4 + (OR, FV, FV), 24, FULL_GLOBAL, "odd, full storage, V0 from global memory"),
    Row(96, (PR,) * 4 + (EU, EU, FV, FV), 24, FULL_GLOBAL, "largest full-storage C"),
    Row(97, (PR,) * 5 + (FV,) * 3, 24, PACKED, "smallest packed C, odd"),
    Row(107, (PR,) * 7 + (OR,), 24, PACKED, "packed, odd"),
    Row(111, (OR,) * 5 + (PR,) * 3, 24, PACKED, "the largest C a handle admits (kb_create), packed, odd"),
)}
# kMargMaxC = 112 cannot be reached through the C-ABI: kb_create admits C <= 111 (the Schur tiles of k_schur), so these
# two rigs are refused there, by that name
K_CREATE_MAX_C = 111
REFUSED_ROWS = {r.C: r for r in (
    Row(112, (OR,) * 6 + (PR, PR), 4, PACKED, "kMargMaxC: refused by kb_create"),
    Row(113, (OR,) * 7 + (PR,), 4, REFUSED, "beyond kMargMaxC: refused by kb_create"),
)}
WARM_ROWS = (23, 79, 107)     # one per regime: 34 alternating calls on one handle
# the device loop (the gated k_marg + marg_tail): C = 79 (full, V0 from global) and C = 97 (packed, odd).  Rigs on which
# the oracle's own GN + marginal loop converges and keeps its rank in every iteration (test_marginal_cases.py)
LOOP_ROWS = {
    79: Row(79, (PR,) * 5 + (OR,), 24, FULL_GLOBAL, "device loop, full storage"),
    97: Row(97, (PR,) * 5 + (FV,) * 3, 24, PACKED, "device loop, packed storage"),
}
LOOP = dict(max_iterations=20, eps_x=1e-3, eps_j=1e-3)
FAIL_C = 9                     # the zero-corner frame: the last frame of the [OR] rig, its one view cut to no corner

DEFAULTS = dict(column_scaling=True, eps_norm=EPS, eps_svd=1e-6, svd_tol=-1.0)
VARIANTS = ("a", "b", "c", "d")
TOL_MARGIN = 1e-3              # the tolerance lies at least this fraction of itself from sv[rank - 1] and sv[rank]
X_SPREAD_TIGHT = 1e-10         # up to here the device's dx takes the existing 1e-8 bar against the oracle
X_SPREAD_MAX = 1e-5            # a row / variant whose two references differ by more does not belong in the table


def problem_of(row):
    return synth.make_problem(list(row.models), row.n_frames, seed=row.seed, p_view=row.p_view,
                              name=f"marginal C = {row.C}")


@functools.lru_cache(maxsize=None)
def problem(C):
    return problem_of(ROWS[C])


@functools.lru_cache(maxsize=None)
def loop_problem(C):
    return problem_of(LOOP_ROWS[C])


def truncate_view(p, v, keep):
    """problem p with view v cut to its first `keep` corners (as test_gpu_edge_cases.py)"""
    import dataclasses
    o = p.view_offset
    idx = np.concatenate([np.arange(o[u], o[u + 1] if u != v else o[u] + keep) for u in range(p.n_views)])
    counts = np.array([(o[u + 1] - o[u]) if u != v else keep for u in range(p.n_views)])
    return dataclasses.replace(p, corner_id=p.corner_id[idx].astype(np.int32), y=p.y[idx].copy(),
                               view_offset=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))


@functools.lru_cache(maxsize=None)
def fail_problem():
    """the FAIL_C rig with the one view of its last frame cut to zero corners: that frame's 6 x 6 block is zero"""
    p = problem(FAIL_C)
    assert p.n_cams == 1 and int(p.view_frame[-1]) == p.n_frames - 1
    return truncate_view(p, p.n_views - 1, 0)


# ---- references in numpy ----
def reduced(blocks):
    """(S, b, diag(Hcc)) of normal blocks: S = Hcc - sum Hfc^T Hff^-1 Hfc, b = gc - sum Hfc^T Hff^-1 gf"""
    Hff, Hfc, gf = blocks["Hff"], blocks["Hfc"], blocks["gf"]
    Y = np.linalg.solve(Hff, Hfc)                    # [F][6][C]
    z = np.linalg.solve(Hff, gf[:, :, None])[:, :, 0]
    S = blocks["Hcc"] - np.einsum("fic,fid->cd", Hfc, Y)
    b = blocks["gc"] - np.einsum("fic,fi->c", Hfc, z)
    return 0.5 * (S + S.T), b, np.diag(blocks["Hcc"]).copy()


def scaling(hdiag, n_rows, opts):
    """G of linalg.cpp:128-152: 1 / column norm, 0 below sqrt(n_rows epsNorm); ones without column scaling"""
    if not opts["column_scaling"]:
        return np.ones_like(hdiag)
    nrm = np.sqrt(hdiag)
    return np.where(nrm < np.sqrt(n_rows * opts["eps_norm"]), 0.0, 1.0 / np.where(nrm > 0, nrm, 1.0))


def rank_stats(sv, C, opts):
    """(tol, rank, gap, log2sum) of singular values sorted descending: rankTol = sv_0 epsSVD C unless svdTol != -1,
    estimateNumericalRank counts down from the back and never below 1, svGap = sv[rank - 1] / sv[rank] (inf at full
    rank), the log2 sum over the kept ones (linalg.cpp:243-282, LinearSolver.cpp:197-201)"""
    tol = opts["svd_tol"] if opts["svd_tol"] != -1.0 else sv[0] * opts["eps_svd"] * C
    rank = C
    for i in range(C - 1, 0, -1):
        if sv[i] > tol:
            break
        rank -= 1
    with np.errstate(divide="ignore"):
        gap = float(sv[rank - 1] / sv[rank]) if rank < C else float("inf")
    return float(tol), rank, gap, float(np.sum(np.log2(sv[:rank])))


def solve_from(V, w, rank, G, b):
    """x = G V_r diag(1 / w) V_r^T G b from an eigen-decomposition (columns of V, signed w, sorted)"""
    Vr = V[:, :rank]
    return G * (Vr @ ((Vr.T @ (G * b)) / w[:rank]))


def ref_solve(S, b, hdiag, n_rows, opts):
    """LAPACK's side: numpy.linalg.eigh of G S G sorted by |w| descending, the rank rule, gap, log2 sum and x"""
    C = S.shape[0]
    G = scaling(hdiag, n_rows, opts)
    Om = G[:, None] * S * G[None, :]
    w, V = np.linalg.eigh(Om)
    order = np.argsort(-np.abs(w), kind="stable")
    w, V = w[order], V[:, order]
    sv = np.abs(w)
    tol, rank, gap, l2 = rank_stats(sv, C, opts)
    return dict(G=G, Omega=Om, w=w, V=V, sv=sv, tol=tol, rank=rank, gap=gap, log2sum=l2,
                x=solve_from(V, w, rank, G, b))


def eig_figures(V, sv, Om):
    """the three figures that do not depend on conditioning: max |V^T V - I|, max off-diagonal |V^T Omega V| / sv_0,
    max ||diag(V^T Omega V)| - sv| / sv_0"""
    C = V.shape[0]
    M = V.T @ Om @ V
    d = np.abs(np.diag(M))
    off = M - np.diag(np.diag(M))
    return (float(np.abs(V.T @ V - np.eye(C)).max()), float(np.abs(off).max() / sv[0]),
            float(np.abs(d - sv).max() / sv[0]))


def margin(sv, tol, rank):
    """min distance of tol from sv[rank - 1] and sv[rank], in units of tol"""
    m = abs(sv[rank - 1] - tol)
    if rank < len(sv):
        m = min(m, abs(sv[rank] - tol))
    return float(m / tol)


def eps_norm_cut(hdiag, n_rows):
    """variant (d): the epsNorm whose cut sqrt(n_rows epsNorm) is the geometric mean of the two weakest neighbouring
    sorted column norms whose ratio is at least 1.01; (eps_norm, number of columns below the cut)"""
    nrm = np.sort(np.sqrt(hdiag))
    for k in range(len(nrm) - 1):
        if nrm[k + 1] >= 1.01 * nrm[k]:
            cut = np.sqrt(nrm[k] * nrm[k + 1])
            return float(cut * cut / n_rows), k + 1
    raise AssertionError("no two neighbouring column norms a factor 1.01 apart")


class Ref:
    """The references of one rig, each part computed once per process and not modified: the oracle's blocks at the
    states "A" (state_init) and "B" (after one step of the oracle's GN + marginal loop), their reduction in numpy, and
    per (state, variant) the oracle's marginal solve, LAPACK's, and the spread between the two."""

    def __init__(self, p):
        from oracle import oracle as O
        self.O = O
        self.p = p
        self.o = O.Oracle(p)
        self.C = p.cam_cols
        self.n_rows = 2 * p.n_corners
        self._state, self._arrow, self._red, self._opts, self._osolve, self._ref, self._fl = {}, {}, {}, {}, {}, {}, {}

    def state(self, which):
        if which not in self._state:
            if which == "A":
                self._state[which] = self.p.state_init.copy()
            else:
                st, r = self.o.optimize(self.p.state_init, policy="gn", max_iterations=1, eps_x=1e-3, eps_j=1e-3,
                                        marg=self.O.marg_opts(self.n_rows))
                assert r["iterations"] == 1 and np.isfinite(st).all()
                self._state[which] = st
        return self._state[which]

    def arrow(self, which):
        if which not in self._arrow:
            self._arrow[which] = self.o.arrow(self.state(which))
        return self._arrow[which]

    def reduced(self, which):
        if which not in self._red:
            self._red[which] = reduced(self.arrow(which))
        return self._red[which]

    def opts(self, variant, which="A"):
        """the LinearSolverOptions of a variant, as a dict of marg_opts' / marginal_options' keywords"""
        key = (which, variant)
        if key not in self._opts:
            o = dict(DEFAULTS)
            if variant == "b":
                o["eps_svd"] = 1e-10
            elif variant == "c":
                o["column_scaling"] = False
                o["svd_tol"] = ROWS[self.C].svd_tol
            elif variant == "d":
                o["eps_norm"] = eps_norm_cut(self.reduced(which)[2], self.n_rows)[0]
            else:
                assert variant == "a"
            self._opts[key] = o
        return self._opts[key]

    def oracle_solve(self, which, variant="a"):
        """(ok, dx, info) of the oracle's marginal solve"""
        key = (which, variant)
        if key not in self._osolve:
            self._osolve[key] = self.o.solve_marginal(self.arrow(which),
                                                      self.O.marg_opts(self.n_rows, **self.opts(variant, which)))
        return self._osolve[key]

    def ref(self, which, variant="a"):
        key = (which, variant)
        if key not in self._ref:
            S, b, hd = self.reduced(which)
            self._ref[key] = ref_solve(S, b, hd, self.n_rows, self.opts(variant, which))
        return self._ref[key]

    def floors(self, which, variant="a"):
        """the reference spread: the oracle against LAPACK (sv, x) and the oracle V's own eig_figures"""
        key = (which, variant)
        if key not in self._fl:
            ok, dx, info = self.oracle_solve(which, variant)
            R = self.ref(which, variant)
            assert ok
            orth, offd, diag = eig_figures(info["V"], info["sv"], R["Omega"])
            self._fl[key] = dict(
                sv=float(np.abs(info["sv"] - R["sv"]).max() / R["sv"][0]),
                x=float(np.abs(dx[: self.C] - R["x"]).max() / np.abs(R["x"]).max()),
                orth=orth, offd=offd, diag=diag)
        return self._fl[key]

    def analyze(self, which):
        """analyzeMarginal's references: the oracle's unscaled SVD of S at the default tolerance, LAPACK's singular
        values, and the bars of the device's eig_figures: 100 times the oracle's own, as bars(), but no oracle figure
        counts as less than one unit roundoff.  A figure is a double-precision expression of terms of the size of sv_0,
        normalised by sv_0: its own evaluation rounds at eps / 2, so a smaller figure is no measurement of the
        reference's error.  On the unscaled, steeply graded S of the one-camera rigs the oracle's off-diagonal figure
        is 0.01 eps (C = 5) and 0.16 eps (C = 9); every other figure of the table is above eps and is not touched"""
        key = (which, "analyze")
        if key not in self._ref:
            S, b, hd = self.reduced(which)
            opts = dict(DEFAULTS, column_scaling=False)
            _, info = self.O.marginal_solve(S, np.zeros(self.C), None, self.O.marg_opts(self.n_rows, **opts))
            L = ref_solve(S, b, hd, self.n_rows, opts)
            self._ref[key] = dict(info=info, sv_ref=L["sv"], rank_ref=L["rank"], S=S,
                                  margin=margin(info["sv"], info["tol"], info["rank"]),
                                  bars=tuple(100.0 * max(x, EPS) for x in eig_figures(info["V"], info["sv"], S)))
        return self._ref[key]

    def bars(self, which, variant="a"):
        """the bars of the device's eig_figures: 100 times the oracle's own for this rig, state and variant (the
        association order differs)"""
        f = self.floors(which, variant)
        return tuple(100.0 * f[k] for k in ("orth", "offd", "diag"))


@functools.lru_cache(maxsize=None)
def ref(C):
    return Ref(problem(C))


@functools.lru_cache(maxsize=None)
def loop_ref(C):
    return Ref(loop_problem(C))


def oracle_loop(R, **kw):
    """Optimizer2::optimize with the GN policy over the marginal solver, from the oracle's primitives, so that the rank
    of every iteration is seen (Oracle.optimize reports the last one only): (iterations, J, state, ranks)"""
    o, kw = R.o, dict(LOOP, **kw)
    st = R.p.state_init.copy()
    J = o.cost(st)
    p_J, dX, dJ, it, ranks = J, kw["eps_x"] + 1, kw["eps_j"] + 1, 0, []
    while it < kw["max_iterations"] and dX > kw["eps_x"] and abs(dJ) > kw["eps_j"]:
        ok, dx, info = o.solve_marginal(o.arrow(st))
        assert ok
        ranks.append(info["rank"])
        st, dX = o.apply_update(st, dx)
        J = o.cost(st)
        dJ, p_J = p_J - J, J
        it += 1
    return it, J, st, ranks
