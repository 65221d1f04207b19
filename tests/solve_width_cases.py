"""The camera-block widths C at which the reduced-system path (kb_solve, kb_covariance and the loops over them) changes
its code, as small rigs with their CPU references: shared by test_solve_width_cases.py (the preconditions, from synth,
the oracle and numpy alone) and test_gpu_solve_widths.py (the device against those references).  No GPU and no HIP
import here.

C = sum of intrinsics + 6 (N - 1) alone selects (kalibr_amd/csrc/kb_solve_layout.h, which kb_create, kb_covariance
and the kernels read; the loops named below are kb_kernels.hip's):
  k_solve<CM> / k_cov_cam<CM>   one-wave register LDL^T on the packed S, CM = 16, 24, 32, 48, 64 for C <= CM;
                                CM = 0 (the k_colimg tile image, blocked ldl_panels on MFMA) for C >= 65
  ldl_panels                    nb = (C + 16) >> 4 tile rows: 5 (65..79), 6 (80..95), 7 (96..111).  Panel 0 has nb - 1
                                tiles below it, four per factor wave: one factor wave at nb = 5, a second one holding
                                one tile at nb = 6 and two at nb = 7.  At C = 80, 96 the appended b row opens a tile row
  k_schur<ms>                   ms = 1, 4, 7 by ceil(lower tiles of [Y | z]^T [Y | z] / 4 waves): C <= 31, 32..79, >= 80
  cov_invert_columns            one column per 16-lane row: 16 columns per round (256 threads, C <= 64), 32 (512
                                threads, C > 64); the rounds step at 16/17, 32/33, 48/49, 64/65 (down) and 96/97
  k_cov_frames                  nks = (C + 3) >> 2 k-steps, nct = (C + 15) >> 4 column tiles, zero-padded operands
  k_build / k_buildp            the pipelined build for rigs of 4 .. 8 cameras
The functions below restate those, independently of the header; test_solve_layout.py compares them with the header's
figures at every admitted shape, and test_solve_width_cases.py asserts every row's selectors against the table, so a
moved constant fails there and the table is redone.

Every rig is synth.make_problem(models, 16, seed=20261200 + C, p_view=0.8).
"""
import dataclasses
import functools
from dataclasses import dataclass

import numpy as np

from kalibr_amd import synth

PR, OR, EU, FV = synth.PINHOLE_RADTAN, synth.OMNI_RADTAN, synth.EUCM, synth.PINHOLE_FOV
N_FRAMES, SEED0, P_VIEW = 16, 20261200, 0.8
LDS_BYTES = 160 * 1024       # per workgroup on gfx950
MAX_C = 111                  # kb_solve_layout.h kMaxC; kb_create: "camera block C > 111 not supported"
MAX_CAMS = 8                 # kb_create: 64 * wpb <= 512 threads of the build block (wpb = N for N >= 4)
K_TS = 17                    # kb_solve_layout.h kTS
K_TILE = 16 * K_TS           # kTileSz
K_X_MAX_RANKS = 64           # kXMaxRanks: per-rank max|dx_f| slots of the image's aux area
K_COV_WAVES = 4              # kCovWaves
K_COV_FRAMES = 2 * K_COV_WAVES


# ---- the selectors, restated ----
def solve_cm(C):
    """the CM of k_solve<CM> / k_cov_cam<CM> (the header's solve_cm); 0: the blocked factorisation"""
    for cm in (16, 24, 32, 48, 64):
        if C <= cm:
            return cm
    return 0


def nb(C):
    """tile rows of the image with the appended b row (rows 0 .. C): also k_schur's nbz and CZ / 16"""
    return (C + 16) >> 4


def schur_ms(C):
    ts = (nb(C) * (nb(C) + 1) // 2 + 3) // 4
    return 1 if ts <= 1 else 4 if ts <= 4 else 7


def solve_threads(C):
    return 256 if C <= 64 else 512


def cov_rounds(C):
    """rounds of cov_invert_columns: one column per 16 threads"""
    ngrp = solve_threads(C) >> 4
    return (C + ngrp - 1) // ngrp


def factor_waves(C):
    """(factor waves of panel 0, tiles held by the second one): ldl_panels' nf = (nb - 1 - q) > 4 ? 2 : 1; the one-wave
    register LDL^T of C <= 64 counts as (1, 0)"""
    if C <= 64:
        return 1, 0
    below = nb(C) - 1
    return (2, below - 4) if below > 4 else (1, 0)


def cov_frames_steps(C):
    """(nks, nct) of k_cov_frames"""
    return (C + 3) >> 2, (C + 15) >> 4


def build_kernel(N):
    """kb_create's build_pipe (kb_build_layout.h pipe_default): one wave per camera (nsplit == 1), at most 8 cameras"""
    return "k_buildp" if max(1, (4 + N - 1) // N) == 1 and N <= 8 else "k_build"


# ---- dynamic LDS, restated (bytes) ----
def lds_schur(C):
    return 8 * 16 * 16 * nb(C)                                  # P, Q [8][CZ], CZ = 16 nb


def lds_camexp(N):
    return 8 * (N * 256 + N * N * 36)                           # Hs [N][256] | T [N][N][36]


def img_n(C):
    return K_TILE * nb(C) * (nb(C) + 1) // 2 + 16 * nb(C) + 2 + K_X_MAX_RANKS   # tiles | aux


def lds_solve(N, C):
    if C <= 64:                                                 # the packed layout
        return 8 * (C * (C + 1) // 2 + 2 * C + 1 + N * 256 + 2 * N * N * 36) + 4 * C
    return 8 * (img_n(C) + 2 + 2 * nb(C) * K_TILE + 16 * nb(C)) + 4 * C     # the image branch


def solve_offsets(N, C):
    """where solve_body<CM> and k_cov_cam<CM> keep their ten regions, in doubles from the start of the dynamic LDS,
    written down region after region from their lengths.  Packed (C <= 64): S [C(C+1)/2] | bv [C + 1] | gl [C] |
    Hs [N][256] | T [N][N][36] | K [N][N][36] | ci; Dfac, Xinv, rDv are not there (they point at ci).  Image (C > 64): the
    tiles | the aux area (bv = gl = Hs = T: g_c [16 nb], cost, rank 0's max|dx_f|) | Dfac [nb][tile] | Xinv [nb][tile] |
    rDv [16 nb] | ci; K is not used (it points N * N * 36 doubles behind T)"""
    if C <= 64:
        S = 0
        bv = S + C * (C + 1) // 2
        gl = bv + (C + 1)
        Hs = gl + C
        T = Hs + N * 256
        K = T + N * N * 36
        ci = K + N * N * 36
        return dict(S=S, bv=bv, gl=gl, Hs=Hs, T=T, K=K, Dfac=ci, Xinv=ci, rDv=ci, ci=ci)
    tiles = K_TILE * nb(C) * (nb(C) + 1) // 2
    Dfac = tiles + 16 * nb(C) + 1 + 1           # g_c slots, the cost, rank 0's max|dx_f|: an even count
    Xinv = Dfac + nb(C) * K_TILE
    rDv = Xinv + nb(C) * K_TILE
    return dict(S=0, bv=tiles, gl=tiles, Hs=tiles, T=tiles, K=tiles + N * N * 36, Dfac=Dfac, Xinv=Xinv, rDv=rDv,
                ci=rDv + 16 * nb(C))


def lds_colimg(N, C):
    return 8 * (N * 256 + 2 * N * N * 36) + 4 * C if C > 64 else 0          # Hs | K, T | ci


def cov_eoff(N, C):
    """doubles before k_cov_cam's second packed triangle (the header's cov_eoff)"""
    if C <= 64:
        return (lds_solve(N, C) + 15) // 16 * 2
    return K_TILE * nb(C) * (nb(C) + 1) // 2 + ((16 * nb(C) + 3) & ~1) + nb(C) * K_TILE


def lds_cov_cam(N, C):
    return max(lds_solve(N, C), 8 * (cov_eoff(N, C) + C * (C + 1) // 2))


def lds_cov_frames(C):
    nct = cov_frames_steps(C)[1]
    return 8 * (C * C + K_COV_WAVES * 16 * (16 * nct + 1))


def admitted_shapes():
    """every (N, C) kb_create admits, as a superset: N <= 8 cameras of 5 .. 9 intrinsics, C <= 111"""
    return [(N, C) for N in range(1, MAX_CAMS + 1) for C in range(11 * N - 6, min(15 * N - 6, MAX_C) + 1)]


def reachable_widths():
    """every C some rig reaches: cameras of 5, 6, 8 or 9 intrinsics (synth.NINTR), N <= 8, C <= 111"""
    sums = {0}
    out = set()
    for N in range(1, MAX_CAMS + 1):
        sums = {s + n for s in sums for n in set(synth.NINTR.values())}
        out |= {s + 6 * (N - 1) for s in sums if s + 6 * (N - 1) <= MAX_C}
    return sorted(out)


# ---- the rigs ----
@dataclass(frozen=True)
class Row:
    C: int
    models: tuple
    cm: int          # k_solve<cm> / k_cov_cam<cm>
    nb: int          # tile rows (C + 16) >> 4
    ms: int          # k_schur<ms>
    rounds: int      # cov_invert_columns
    fw: tuple        # (factor waves of panel 0, tiles of the second)
    what: str

    @property
    def singular(self):
        """omni-radtan rigs: numerically singular at lambda = 0 (Jacobi-scaled cond 1e11 .. 1e15, the two CPU routes
        differ by 1e-6 .. 1e-2), and undamped Gauss-Newton is not defined on them (one accepted step, three failed
        ones in the oracle, as test_gpu_buildp_tail.py notes)"""
        return OR in self.models


ROWS = {r.C: r for r in (
    Row(16, (FV, FV), 16, 2, 1, 1, (1, 0), "last C of CM = 16; one round of cov_invert_columns; k_schur<1>, nbz = 2"),
    Row(17, (FV, EU), 24, 2, 1, 2, (1, 0), "first of CM = 24; C mod 4 = 1"),
    Row(24, (OR, OR), 24, 2, 1, 2, (1, 0), "last of CM = 24"),
    Row(27, (FV,) * 3, 32, 2, 1, 2, (1, 0), "smallest C of k_solve<32> / k_cov_cam<32> (25, 26: no rig)"),
    Row(31, (FV, EU, PR), 32, 2, 1, 2, (1, 0), "last C of k_schur<1>"),
    Row(32, (EU, EU, PR), 32, 3, 4, 2, (1, 0), "last of CM = 32; first of k_schur<4>"),
    Row(33, (FV, PR, PR), 48, 3, 4, 3, (1, 0), "first of CM = 48; third round of the column inversion"),
    Row(48, (PR, PR, PR, EU), 48, 4, 4, 3, (1, 0), "last of CM = 48, regular at lambda = 0"),
    Row(49, (FV,) * 5, 64, 4, 4, 4, (1, 0), "first of CM = 64: k_cov_cam<64>"),
    Row(63, (FV,) * 5 + (PR,), 64, 4, 4, 4, (1, 0), "odd, last lane but one of the one-wave factorisation"),
    Row(64, (PR,) * 5, 64, 5, 4, 4, (1, 0), "every lane of the one-wave factorisation holds a row"),
    Row(65, (FV,) * 3 + (EU,) * 2 + (PR,), 0, 5, 4, 3, (1, 0), "first C of k_solve<0>; nb = 5; row C second of its tile"),
    Row(79, (FV,) * 3 + (EU,) * 2 + (PR,) * 2, 0, 5, 4, 3, (1, 0), "last of nb = 5 and k_schur<4>; row C last of its tile"),
    Row(80, (FV,) * 2 + (PR,) * 2 + (EU,) * 3, 0, 6, 7, 3, (2, 1), "first of nb = 6 and k_schur<7>; row C opens a tile row"),
    Row(81, (PR,) * 3 + (OR,) * 3, 0, 6, 7, 3, (2, 1), "nb = 6, odd"),
    Row(95, (FV,) + (PR,) * 3 + (EU,) * 4, 0, 6, 7, 3, (2, 1), "last of nb = 6"),
    Row(96, (PR,) * 4 + (EU,) * 2 + (FV,) * 2, 0, 7, 7, 3, (2, 2), "first of nb = 7; row C opens a tile row"),
    Row(97, (PR,) * 5 + (FV,) * 3, 0, 7, 7, 4, (2, 2), "fourth round of 32 columns in k_cov_cam<0>"),
    Row(111, (OR,) * 5 + (PR,) * 3, 0, 7, 7, 4, (2, 2), "the widest C kb_create admits; C mod 4 = 3"),
)}
SINGULAR_ROWS = (24, 81, 111)
STATES = ("state_init", "state_truth")
# the (row, lambda) pairs compared, written out so that the list cannot shrink silently: every lambda on the 16
# regular rows, the damped ones on the omni-radtan rows (their lambda = 0 flag hinges on rounding: not asserted either)
PAIRS = (
    (16, 0.0), (16, 1.0), (16, 10.0), (17, 0.0), (17, 1.0), (17, 10.0), (24, 1.0), (24, 10.0),
    (27, 0.0), (27, 1.0), (27, 10.0), (31, 0.0), (31, 1.0), (31, 10.0), (32, 0.0), (32, 1.0), (32, 10.0),
    (33, 0.0), (33, 1.0), (33, 10.0), (48, 0.0), (48, 1.0), (48, 10.0), (49, 0.0), (49, 1.0), (49, 10.0),
    (63, 0.0), (63, 1.0), (63, 10.0), (64, 0.0), (64, 1.0), (64, 10.0), (65, 0.0), (65, 1.0), (65, 10.0),
    (79, 0.0), (79, 1.0), (79, 10.0), (80, 0.0), (80, 1.0), (80, 10.0), (81, 1.0), (81, 10.0),
    (95, 0.0), (95, 1.0), (95, 10.0), (96, 0.0), (96, 1.0), (96, 10.0), (97, 0.0), (97, 1.0), (97, 10.0),
    (111, 1.0), (111, 10.0),
)
GN_ROWS = (16, 17, 27, 31, 32, 33, 48, 49, 63, 64, 65, 79, 80, 95, 96, 97)
GN_LEFT_OUT = {C: "omni-radtan cameras: undamped Gauss-Newton is not defined (the oracle's own passes fail)"
               for C in SINGULAR_ROWS}
SLICE_ROWS = (17, 65, 111)   # again on their first 13 frames: odd F, a short last block of k_cov_frames
SLICE_FRAMES = 13
DIAG_ROWS = (17, 32, 64, 65, 80, 111)
DIAG_LAMBDA = "diag"
NONPD_ROWS = (27, 80)        # one width per factorisation: the register LDL^T and ldl_panels
LM = dict(policy="lm", lambda0=10.0, max_iterations=6, eps_x=1e-3, eps_j=1.0)
GN = dict(policy="gn", max_iterations=3)

# bars.  The references' own spread (test_solve_width_cases.py asserts it) is 10 x under the device's bars, which are
# those of test_gpu_parity.py and test_gpu_covariance.py
REF_DX = 1e-9
REF_COV = 1e-9
REF_STATE = 1e-8
DEV_DX = 1e-8
DEV_RESID = 1e-9
DEV_COV = 1e-8
DEV_J = 1e-9
DEV_STATE = 1e-6


def lambdas(C):
    return tuple(lam for c, lam in PAIRS if c == C)


def diagonal(ncols):
    return np.random.default_rng(7).uniform(0.5, 20.0, ncols)


@functools.lru_cache(maxsize=None)
def problem(C):
    r = ROWS[C]
    return synth.make_problem(list(r.models), N_FRAMES, seed=SEED0 + C, p_view=P_VIEW, name=f"solve width C = {C}")


@functools.lru_cache(maxsize=None)
def slice_problem(C):
    return problem(C).frame_slice(0, SLICE_FRAMES)


def truncate_view(p, v, keep):
    """problem p with view v cut to its first `keep` corners (as test_gpu_edge_cases.py)"""
    o = p.view_offset
    idx = np.concatenate([np.arange(o[u], o[u + 1] if u != v else o[u] + keep) for u in range(p.n_views)])
    counts = np.array([(o[u + 1] - o[u]) if u != v else keep for u in range(p.n_views)])
    return dataclasses.replace(p, corner_id=p.corner_id[idx].astype(np.int32), y=p.y[idx].copy(),
                               view_offset=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))


def nonpd_frame(C):
    """the frame of row C that loses its corners: the first of those seen by the fewest cameras"""
    p = problem(C)
    return int(np.argmin(np.bincount(p.view_frame, minlength=p.n_frames)))


@functools.lru_cache(maxsize=None)
def nonpd_problem(C):
    """row C with every view of nonpd_frame(C) cut to no corner (its only view, where one camera saw it): that frame's
    6 x 6 block, its H_fc and g_f are 0"""
    p = problem(C)
    for v in np.nonzero(p.view_frame == nonpd_frame(C))[0]:
        p = truncate_view(p, int(v), 0)
    return p


# ---- references in numpy ----
def dense_H(A, lam):
    """the dense (C + 6F)^2 normal matrix of arrow blocks + lam^2 I, or + diag(lam^2) for an array lam"""
    C, F = A["Hcc"].shape[0], A["Hff"].shape[0]
    n = C + 6 * F
    H = np.zeros((n, n))
    H[:C, :C] = A["Hcc"]
    for f in range(F):
        o = C + 6 * f
        H[o:o + 6, o:o + 6] = A["Hff"][f]
        H[o:o + 6, :C] = A["Hfc"][f]
        H[:C, o:o + 6] = A["Hfc"][f].T
    return H + np.diag(np.broadcast_to(np.asarray(lam, dtype=float) ** 2, (n,)))


def blocks_of(P, C):
    """(Pcc, Pff, Pfc) of a dense (C + 6F)^2 matrix"""
    F = (P.shape[0] - C) // 6
    Pff = np.stack([P[C + 6 * f:C + 6 * f + 6, C + 6 * f:C + 6 * f + 6] for f in range(F)])
    Pfc = np.stack([P[C + 6 * f:C + 6 * f + 6, :C] for f in range(F)])
    return P[:C, :C], Pff, Pfc


def cov_errs(out, P_ref, C):
    """test_gpu_covariance.py's metric: the worst |P - P_ref|_ij / sqrt(P_ref,ii P_ref,jj) of each block"""
    sd = np.sqrt(np.diag(P_ref))
    cc, ff, fc = blocks_of(P_ref, C)
    F = ff.shape[0]
    sc, sf = sd[:C], sd[C:].reshape(F, 6)
    return dict(Pcc=float((np.abs(out["Pcc"] - cc) / np.outer(sc, sc)).max()),
                Pff=float((np.abs(out["Pff"] - ff) / (sf[:, :, None] * sf[:, None, :])).max()),
                Pfc=float((np.abs(out["Pfc"] - fc) / (sf[:, :, None] * sc[None, None, :])).max()))


def schur_cov(A, lam):
    """the second CPU route: the Schur formulas kb_covariance evaluates, in numpy.  Sigma_cc = S^-1,
    Sigma_fc = -A_f Sigma_cc, Sigma_ff = (H_ff + D_f)^-1 + A_f Sigma_cc A_f^T"""
    C, F = A["Hcc"].shape[0], A["Hff"].shape[0]
    d2 = np.broadcast_to(np.asarray(lam, dtype=float) ** 2, (C + 6 * F,))
    Hff = A["Hff"] + np.stack([np.diag(d2[C + 6 * f:C + 6 * f + 6]) for f in range(F)])
    Af = np.linalg.solve(Hff, A["Hfc"])                    # [F][6][C]; a product with inv(H_ff) loses a digit at lambda = 0
    S = A["Hcc"] + np.diag(d2[:C]) - np.einsum("fic,fid->cd", A["Hfc"], Af)
    Scc = np.linalg.inv(S)
    return dict(Pcc=Scc, Pfc=-Af @ Scc, Pff=np.linalg.inv(Hff) + Af @ Scc @ Af.transpose(0, 2, 1))


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


class Ref:
    """The references of one problem, each computed once per process and not modified: the oracle's blocks at the two
    states, and per (state, lambda) the dense H, LAPACK's dx and inverse, the oracle's Schur solve, the numpy Schur
    covariance and the spread between the routes.  lambda is a number or DIAG_LAMBDA (the diagonal conditioner)."""

    def __init__(self, p):
        from oracle import oracle as O
        self.O = O
        self.p = p
        self.o = O.Oracle(p)
        self.C = p.cam_cols
        self._arrow, self._H, self._dx, self._odx, self._P, self._fl, self._loop = {}, {}, {}, {}, {}, {}, {}

    def arrow(self, sname):
        if sname not in self._arrow:
            self._arrow[sname] = self.o.arrow(getattr(self.p, sname))
        return self._arrow[sname]

    def lam(self, lam):
        return diagonal(self.p.total_cols) if lam == DIAG_LAMBDA else lam

    def H(self, sname, lam):
        if (sname, lam) not in self._H:
            self._H[sname, lam] = dense_H(self.arrow(sname), self.lam(lam))
        return self._H[sname, lam]

    def dense_dx(self, sname, lam):
        if (sname, lam) not in self._dx:
            self._dx[sname, lam] = np.linalg.solve(self.H(sname, lam), self.arrow(sname)["rhs"])
        return self._dx[sname, lam]

    def oracle_dx(self, sname, lam):
        """(ok, dx) of the oracle's Schur solve; the diagonal conditioner enters as blocks with d^2 on their diagonals"""
        if (sname, lam) not in self._odx:
            A = self.arrow(sname)
            if lam == DIAG_LAMBDA:
                O, C, F = self.O, self.C, self.p.n_frames
                d2 = diagonal(self.p.total_cols) ** 2
                B = {k: A[k].copy() for k in ("Hff", "Hfc", "Hcc", "gf", "gc")}
                B["Hcc"] += np.diag(d2[:C])
                for f in range(F):
                    B["Hff"][f] += np.diag(d2[C + 6 * f:C + 6 * f + 6])
                B["_A"] = O._Arrow(C, F, O._d(B["Hff"]), O._d(B["Hfc"]), O._d(B["Hcc"]), O._d(B["gf"]), O._d(B["gc"]),
                                   A["cost"])
                self._odx[sname, lam] = self.o.solve(B, 0.0)
            else:
                self._odx[sname, lam] = self.o.solve(A, lam)
        return self._odx[sname, lam]

    def P(self, sname, lam):
        """numpy.linalg.inv of the dense H"""
        if (sname, lam) not in self._P:
            self._P[sname, lam] = np.linalg.inv(self.H(sname, lam))
        return self._P[sname, lam]

    def floors(self, sname, lam):
        """the references' own spread: the oracle's dx against LAPACK's (of max|dx|), its residual, and the two
        covariance routes in cov_errs' metric"""
        if (sname, lam) not in self._fl:
            ok, dx = self.oracle_dx(sname, lam)
            ref = self.dense_dx(sname, lam)
            rhs = self.arrow(sname)["rhs"]
            e = cov_errs(schur_cov(self.arrow(sname), self.lam(lam)), self.P(sname, lam), self.C)
            self._fl[sname, lam] = dict(ok=ok, dx=rel(dx, ref), cov=max(e.values()),
                                        resid=float(np.linalg.norm(self.H(sname, lam) @ ref - rhs) / np.linalg.norm(rhs)))
        return self._fl[sname, lam]

    def loop(self, kind, nthreads=1):
        """(state, result) of the oracle's LM (six iterations) or GN (three passes) from state_init"""
        if (kind, nthreads) not in self._loop:
            self._loop[kind, nthreads] = self.o.optimize(self.p.state_init, nthreads=nthreads,
                                                         **(LM if kind == "lm" else GN))
        return self._loop[kind, nthreads]


@functools.lru_cache(maxsize=None)
def ref(C):
    return Ref(problem(C))


@functools.lru_cache(maxsize=None)
def slice_ref(C):
    return Ref(slice_problem(C))


@functools.lru_cache(maxsize=None)
def nonpd_ref(C):
    return Ref(nonpd_problem(C))
