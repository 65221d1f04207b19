"""The preconditions of the camera-block width sweep (tests/solve_width_cases.py), from synth, the oracle and numpy
alone: every rig synthesises with its row's C, N and F and no empty view; the restated selectors give what the table
records and the rows hold both ends of every bucket; the references agree among themselves 10 x below the device's bars
(the oracle's Schur solve against LAPACK's dense solve, numpy.linalg.inv against the Schur formulas in numpy), so that
no reference can decide a GPU test; the oracle's LM and GN loops do not depend on its thread count.  One check reads the
built library: static (from the code object's metadata) + dynamic LDS of k_solve, k_cov_cam, k_schur (every
instantiation), k_cov_frames, k_colimg and k_camexpand within a workgroup's 160 KB at every (N, C) kb_create admits.

Measured (worst over both states and the admitted lambdas of a row; dx of max|dx|, cov in test_gpu_covariance.py's
metric; the LM / GN columns are max|state(1 thread) - state(8 threads)|):

    C     dx       cov      LM it / failed  LM spread  GN spread
    16    2.2e-11  8.0e-12  5 / 0           1.8e-12    3.4e-13
    17    1.6e-11  7.3e-12  6 / 0           3.9e-12    2.3e-13
    24    6.2e-12  1.5e-12  6 / 0           3.3e-12    -
    27    9.9e-12  5.0e-12  6 / 0           2.3e-12    2.8e-13
    31    9.5e-12  1.1e-11  6 / 0           1.3e-11    2.4e-12
    32    1.9e-11  3.6e-11  6 / 3           2.5e-12    3.0e-11
    33    6.7e-12  5.8e-12  6 / 0           4.5e-12    3.4e-13
    48    3.5e-11  5.2e-12  6 / 1           2.7e-11    1.5e-12
    49    3.9e-11  1.4e-11  6 / 0           2.7e-11    5.7e-12
    63    3.1e-11  1.6e-11  6 / 0           6.3e-12    1.4e-12
    64    1.2e-11  1.2e-11  6 / 0           1.8e-11    1.5e-12
    65    1.5e-11  2.7e-11  6 / 0           1.3e-11    4.5e-13
    79    2.0e-11  2.3e-11  6 / 2           1.4e-11    2.8e-12
    80    6.2e-11  1.3e-10  6 / 2           1.1e-11    1.0e-11
    81    1.8e-10  1.8e-10  6 / 0           7.7e-12    -
    95    6.8e-11  2.6e-11  6 / 2           2.5e-10    8.8e-12
    96    1.5e-11  3.1e-11  6 / 2           1.2e-11    3.2e-11
    97    3.1e-11  1.8e-11  6 / 0           4.8e-11    3.3e-11
    111   1.9e-10  4.6e-10  6 / 0           4.3e-10    -

13-frame slices (17, 65, 111): <= 5.6e-10.  Diagonal conditioner (17, 32, 64, 65, 80, 111): dx <= 1.3e-11, cov <=
6.2e-11, Jacobi-scaled cond 2.3e4 .. 7.1e5.  LDS, the worst static + dynamic sum of each kernel over the admitted
shapes: k_cov_frames 158,728 B at C = 111 (5,112 B to spare), k_cov_cam<0> 127,712 B, k_solve<0> 119,996 B.
"""
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from . import solve_width_cases as W
from .test_solve_layout import header_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICE_CASES = [(C, lam) for C in W.SLICE_ROWS for lam in W.lambdas(C)]


# ---- the table ----
@pytest.mark.parametrize("C", list(W.ROWS))
def test_rig_synthesises(C):
    r, p = W.ROWS[C], W.problem(C)
    assert (p.n_cams, p.n_frames, p.cam_cols) == (len(r.models), W.N_FRAMES, C) and r.C == C
    assert p.cam_model.tolist() == list(r.models)
    assert sum(W.synth.NINTR[m] for m in r.models) + 6 * (len(r.models) - 1) == C
    assert np.all(np.diff(p.view_offset) > 0)                                   # no empty view
    assert np.array_equal(np.unique(p.view_frame), np.arange(p.n_frames))      # every frame seen
    assert np.array_equal(np.unique(p.view_cam), np.arange(p.n_cams))          # every camera sees
    assert p.n_corners < 20000


@pytest.mark.parametrize("C", W.SLICE_ROWS)
def test_slice_synthesises(C):
    s = W.slice_problem(C)
    assert (s.n_frames, s.cam_cols, s.n_cams) == (W.SLICE_FRAMES, C, W.problem(C).n_cams)
    assert np.all(np.diff(s.view_offset) > 0)
    assert np.array_equal(np.unique(s.view_frame), np.arange(W.SLICE_FRAMES))
    assert np.array_equal(np.unique(s.view_cam), np.arange(s.n_cams))
    # what the slice is there for: an odd F, a short last block of k_cov_frames, one frame in its last wave
    assert s.n_frames % 2 == 1 and s.n_frames % W.K_COV_FRAMES not in (0, W.K_COV_FRAMES - 1)


def test_selection():
    for C, r in W.ROWS.items():
        got = (W.solve_cm(C), W.nb(C), W.schur_ms(C), W.cov_rounds(C), W.factor_waves(C))
        assert got == (r.cm, r.nb, r.ms, r.rounds, r.fw), (C, got)
        assert r.singular == (C in W.SINGULAR_ROWS)
    # the thresholds themselves
    assert [W.solve_cm(C) for C in (16, 17, 24, 25, 32, 33, 48, 49, 64, 65, 111)] == \
        [16, 24, 24, 32, 32, 48, 48, 64, 64, 0, 0]
    assert [W.nb(C) for C in (65, 79, 80, 95, 96, 111)] == [5, 5, 6, 6, 7, 7]
    assert [W.schur_ms(C) for C in (5, 31, 32, 79, 80, 111)] == [1, 1, 4, 4, 7, 7]
    assert [W.cov_rounds(C) for C in (16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 111)] == [1, 2, 2, 3, 3, 4, 4, 3, 3, 4, 4]
    assert [W.factor_waves(C) for C in (64, 65, 79, 80, 95, 96, 111)] == \
        [(1, 0), (1, 0), (1, 0), (2, 1), (2, 1), (2, 2), (2, 2)]
    assert [W.cov_frames_steps(C) for C in (16, 17, 111)] == [(4, 1), (5, 2), (28, 7)]
    assert [W.build_kernel(N) for N in (1, 2, 3, 4, 8, 9)] == ["k_build"] * 3 + ["k_buildp"] * 2 + ["k_build"]
    # the written-out pairs: all three lambdas on the regular rows, the damped two on the omni-radtan rows
    want = [(C, lam) for C in W.ROWS for lam in ((1.0, 10.0) if C in W.SINGULAR_ROWS else (0.0, 1.0, 10.0))]
    assert list(W.PAIRS) == want and len(W.PAIRS) == 16 * 3 + 3 * 2
    assert sorted(W.GN_ROWS + tuple(W.GN_LEFT_OUT)) == sorted(W.ROWS) and all(W.GN_LEFT_OUT.values())
    assert set(W.SLICE_ROWS) | set(W.DIAG_ROWS) | set(W.NONPD_ROWS) <= set(W.ROWS)
    assert [W.ROWS[C].cm for C in W.NONPD_ROWS] == [32, 0]


# the smallest reachable width, a one-camera pinhole-FOV rig (C = 5, the lower end of CM = 16, k_schur<1> and the
# one-round inversion), is no row: test_gpu_parity.py, test_gpu_covariance.py and test_gpu_model_sets.py hold the
# one-camera rigs per call
HELD_ELSEWHERE = {5}


def test_rows_hold_both_ends_of_every_bucket():
    reach = W.reachable_widths()
    assert reach[0] == 5 and reach[-1] == W.MAX_C and 25 not in reach and 26 not in reach and 27 in reach
    selectors = dict(solve_cm=W.solve_cm, nb=lambda C: W.nb(C) if C > 64 else 0, schur_ms=W.schur_ms,
                     cov_rounds=lambda C: (W.solve_threads(C), W.cov_rounds(C)), factor_waves=W.factor_waves)
    for name, sel in selectors.items():
        buckets = {}
        for C in reach:
            buckets.setdefault(sel(C), []).append(C)
        for key, cs in buckets.items():
            ends = {min(cs), max(cs)} - HELD_ELSEWHERE
            assert ends <= set(W.ROWS), (name, key, sorted(ends - set(W.ROWS)))
    # the first width of the next bucket, and every multiple of 16: k_schur's row stride CZ steps there, and at 80 and
    # 96 the b row opens a tile row of the image
    assert {17, 33, 49, 65} <= set(W.ROWS) and {16, 32, 48, 64, 80, 96} <= set(W.ROWS)
    assert {C % 4 for C in W.ROWS} == {0, 1, 3} and any(C % 16 == 0 for C in W.ROWS)


# ---- the references ----
def _check_floors(R, sname, lam, tag):
    f = R.floors(sname, lam)
    print(f"{tag} {sname} lambda {lam}: oracle dx vs LAPACK {f['dx']:.1e}, inv vs Schur formulas {f['cov']:.1e}, "
          f"LAPACK's residual {f['resid']:.1e}")
    assert f["ok"]
    assert f["dx"] <= W.REF_DX and f["cov"] <= W.REF_COV
    assert f["resid"] <= 0.1 * W.DEV_RESID


@pytest.mark.parametrize("C,lam", W.PAIRS)
def test_reference_floors(C, lam):
    for sname in W.STATES:
        _check_floors(W.ref(C), sname, lam, f"C = {C}")


@pytest.mark.parametrize("C,lam", SLICE_CASES)
def test_reference_floors_of_the_slices(C, lam):
    for sname in W.STATES:
        _check_floors(W.slice_ref(C), sname, lam, f"C = {C}, {W.SLICE_FRAMES} frames")


@pytest.mark.parametrize("C", W.DIAG_ROWS)
def test_reference_floors_under_the_diagonal_conditioner(C):
    R = W.ref(C)
    _check_floors(R, "state_init", W.DIAG_LAMBDA, f"C = {C}, diagonal conditioner")
    d = W.diagonal(R.p.total_cols)
    assert d.min() >= 0.5 and d.max() <= 20.0 and np.ptp(d) > 15.0
    H = R.H("state_init", W.DIAG_LAMBDA)
    assert np.array_equal(np.diag(H) - np.diag(W.dense_H(R.arrow("state_init"), 0.0)) > 0, np.ones(len(d), bool))
    s = 1.0 / np.sqrt(np.diag(H))
    cond = np.linalg.cond(H * np.outer(s, s))
    print(f"C = {C}: Jacobi-scaled cond {cond:.1e}")
    assert cond < 1e7


@pytest.mark.parametrize("C", list(W.ROWS))
def test_lm_reference_does_not_depend_on_threads(C):
    R = W.ref(C)
    (s1, r1), (s8, r8) = R.loop("lm", 1), R.loop("lm", 8)
    spread = float(np.abs(s1 - s8).max())
    print(f"C = {C}: LM {r1['iterations']} iterations, {r1['failed_iterations']} failed, spread {spread:.1e}")
    assert r1["iterations"] == r8["iterations"] and r1["failed_iterations"] == r8["failed_iterations"]
    assert np.array_equal(r1["trace"][:, 3], r8["trace"][:, 3])
    assert 1 <= r1["iterations"] <= W.LM["max_iterations"] and np.isfinite(s1).all()
    assert spread <= W.REF_STATE
    assert abs(r1["J_final"] - r8["J_final"]) <= 0.1 * W.DEV_J * r1["J_final"]


def test_lm_reference_runs_the_revert_path():
    failed = {C: W.ref(C).loop("lm", 1)[1]["failed_iterations"] for C in W.ROWS}
    assert {C for C, n in failed.items() if n} >= {32, 48, 79, 80, 95, 96}, failed
    assert any(W.ROWS[C].cm and n for C, n in failed.items()) and any(not W.ROWS[C].cm and n for C, n in failed.items())


@pytest.mark.parametrize("C", W.GN_ROWS)
def test_gn_reference(C):
    R = W.ref(C)
    (s1, r1), (s8, r8) = R.loop("gn", 1), R.loop("gn", 8)
    spread = float(np.abs(s1 - s8).max())
    print(f"C = {C}: GN spread {spread:.1e}")
    for r in (r1, r8):
        assert r["iterations"] == 3 and r["failed_iterations"] == 0
    assert np.isfinite(s1).all() and spread <= W.REF_STATE
    assert abs(r1["J_final"] - r8["J_final"]) <= 0.1 * W.DEV_J * r1["J_final"]


@pytest.mark.parametrize("C", W.NONPD_ROWS)
def test_zero_corner_frame_in_the_oracle(C):
    R, f = W.nonpd_ref(C), W.nonpd_frame(C)
    p, h = R.p, W.problem(C)
    assert (p.n_frames, p.n_views) == (h.n_frames, h.n_views) and p.n_corners < h.n_corners
    A = R.arrow("state_init")
    assert not A["Hff"][f].any() and not A["Hfc"][f].any() and not A["gf"][f].any()
    assert all(A["Hff"][g].any() for g in range(p.n_frames) if g != f)
    assert not R.o.solve(A, 0.0)[0] and not R.o.solve(A, 0.0, dense=True)[0]
    _check_floors(R, "state_init", 10.0, f"C = {C}, frame {f} without corners")
    ok, dx = R.oracle_dx("state_init", 10.0)
    assert ok and not dx[C + 6 * f:C + 6 * f + 6].any()
    P = W.blocks_of(R.P("state_init", 10.0), C)
    assert np.abs(P[1][f] - np.eye(6) / 100.0).max() <= 1e-15 and np.abs(P[2][f]).max() <= 1e-15


# ---- LDS, from the built library ----
KERNELS = {"k_solve": r"7k_solveILi(\d+)E", "k_cov_cam": r"9k_cov_camILi(\d+)E", "k_schur": r"7k_schurILi(\d+)E",
           "k_cov_frames": r"12k_cov_framesE()", "k_colimg": r"8k_colimgE()", "k_camexpand": r"11k_camexpandE()"}


def _static_lds(tmp_path):
    """{(kernel, template argument or None): group_segment_fixed_size} from the gfx950 code objects of the built
    library (the metadata notes list a kernel's fields in alphabetical order: the size precedes the name); a kernel
    compiled into several translation units counts with its largest size"""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    lib = shutil.copy(os.path.join(ROOT, "kalibr_amd", "libkalibr_hip.so"), str(tmp_path))
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", lib], check=True, capture_output=True,
                   cwd=str(tmp_path))
    out = {}
    for f in glob.glob(os.path.join(str(tmp_path), "*gfx950*")):
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", f], check=True, capture_output=True,
                               text=True).stdout
        size = None
        for line in notes.split("\n"):
            m = re.match(r"\s*\.group_segment_fixed_size:\s*(\d+)", line)
            if m:
                size = int(m.group(1))
            m = re.match(r"\s*\.name:\s*(\S+)", line)
            if m:
                for k, pat in KERNELS.items():
                    t = re.search(r"kb" + pat, m.group(1))
                    if t:
                        key = (k, int(t.group(1)) if t.group(1) else None)
                        out[key] = max(out.get(key, 0), size)
    return out


def test_solve_and_covariance_kernels_fit_the_lds_at_every_width(tmp_path):
    """static + dynamic LDS within the 160 KB of a workgroup for every N and C a handle admits (beyond 160 KB
    hipFuncSetAttribute refuses the launch), and each kernel's static LDS within the bound that kb_create and
    kb_covariance add to the dynamic size (kb_solve_layout.h)"""
    st = _static_lds(tmp_path)
    print("static LDS:", {f"{k}<{a}>" if a is not None else k: v for (k, a), v in sorted(st.items(), key=str)})
    cms = (0, 16, 24, 32, 48, 64)
    assert set(st) == ({("k_solve", c) for c in cms} | {("k_cov_cam", c) for c in cms}
                       | {("k_schur", m) for m in (1, 4, 7)}
                       | {("k_cov_frames", None), ("k_colimg", None), ("k_camexpand", None)}), sorted(st, key=str)
    # the parse took these kernels' own figures: at least the arrays they declare
    chain = 8 * (16 * 12 + 64 * 12)                          # sizeof(ChainLds)
    for c in cms:
        assert chain + 8 * 16 * 7 <= st["k_solve", c] <= 32 * 1024            # chl, nbase and the back-substitution's
        declared = 8 * (c or 112) + (4 * 3 * 16 if c else 0)                  # rdl; ctab (the packed path alone)
        assert declared <= st["k_cov_cam", c] <= declared + 64
    assert st["k_solve", 0] >= st["k_solve", 64] + 8 * 128                    # xb
    assert 8 * W.K_COV_WAVES * 2 * 36 <= st["k_cov_frames", None] <= 8 * W.K_COV_WAVES * 2 * 36 + 64  # hinv
    shapes = W.admitted_shapes()
    assert (8, W.MAX_C) in shapes and (1, 5) in shapes and (5, 64) in shapes and (6, 64) in shapes
    worst = {}
    for N, C in shapes:
        cm, ms = W.solve_cm(C), W.schur_ms(C)
        total = {f"k_solve<{cm}>": st["k_solve", cm] + W.lds_solve(N, C),
                 f"k_cov_cam<{cm}>": st["k_cov_cam", cm] + W.lds_cov_cam(N, C),
                 f"k_schur<{ms}>": st["k_schur", ms] + W.lds_schur(C),
                 "k_cov_frames": st["k_cov_frames", None] + W.lds_cov_frames(C),
                 "k_colimg": st["k_colimg", None] + W.lds_colimg(N, C),
                 "k_camexpand": st["k_camexpand", None] + W.lds_camexp(N)}
        for k, v in total.items():
            if v > worst.get(k, (0,))[0]:
                worst[k] = (v, N, C)
    for k, (v, N, C) in sorted(worst.items()):
        print(f"{k}: {v} B at N = {N}, C = {C} ({W.LDS_BYTES - v} B to spare)")
        assert v <= W.LDS_BYTES, (k, v, N, C)
    assert len(worst) == 6 + 6 + 3 + 3
    # kb_create and kb_covariance add kb_solve_layout.h's static bounds to the dynamic sizes: each kernel's real static
    # LDS is within its family's bound
    k = header_constants(tmp_path)
    for (kern, arg), size in sorted(st.items(), key=str):
        bound = k["st_" + kern[2:]]
        print(f"{kern}<{arg}>: static {size} B, bound {bound} B")
        assert size <= bound, (kern, arg)
    # the figure this check was asked for: k_cov_frames at the widest C
    assert W.lds_cov_frames(111) == 156424


# The host's formulas and selectors (kb_create, kb_covariance) are kb_solve_layout.h's, compared value by value with the
# restatements in test_solve_layout.py.  What the kernels alone decide stays held to their text: the loops of
# ldl_panels and cov_invert_columns, and k_buildp's camera count (kTS, kTileSz, kCovWaves and k_cov_frames' nct / nks
# moved into the header: compared as numbers there)
SOURCE_TEXT = {
    "kb_kernels.hip": (
        "constexpr int kBuildpMaxCams = 8;",
        "const int nf = (nb - 1 - q) > 4 ? 2 : 1;",                                           # factor_waves
        "const int ti = q + 1 + 4 * fw + t;",
        "const int tid = threadIdx.x, grp = tid >> 4, r = tid & 15, ngrp = nth >> 4;",        # cov_rounds
        "for (int j0 = 0; j0 < C; j0 += ngrp) {",
    ),
}


@pytest.mark.parametrize("name", list(SOURCE_TEXT))
def test_restated_formulas_are_the_sources(name):
    with open(os.path.join(ROOT, "kalibr_amd", "csrc", name)) as f:
        src = re.sub(r"//[^\n]*", "", f.read())
    src = " ".join(src.split())
    for text in SOURCE_TEXT[name]:
        assert " ".join(text.split()) in src, text
