"""The preconditions of the k_marg shape sweep (tests/marginal_cases.py), from synth, the oracle and numpy alone: every
rig synthesises with the camera-block width and the k_marg regime its row records; for every row and option variant the
oracle's rank tolerance stands clear of the singular values on either side of it and the oracle and LAPACK
(numpy.linalg.eigh) agree on the rank; the eps_norm variant zeroes columns; the device-loop rigs converge and keep their
rank in the oracle; the zero-corner frame fails in the oracle -- so a case the references cannot referee is a failure
here, never a skip on the GPU.  One check reads the built library: k_marg's static LDS (from the code object's metadata)
plus its dynamic LDS stays within a workgroup's 160 KB at every width a handle admits.

Variants: (a) defaults (column scaling, epsSVD 1e-6), (b) epsSVD 1e-10, (c) no column scaling with svdTol = 1,
(d) an epsNorm that zeroes the weakest column(s).

The reference spread, oracle against LAPACK at state_init (the floors the GPU bars of test_gpu_marginal_shapes.py rest
on; asserted below as bounds): |sv - sv_ref| / sv_0, |x - x_ref| / max|x_ref| per variant, and the oracle V's own
max|V^T V - I|, max off-diagonal |V^T Omega V| / sv_0 (worst over the variants).  Measured:

    C    rank a / b / c / d   margin (min)  sv       x (a)    x (b)    x (c)    x (d)    V^T V-I  off-diag
    5      5 /   5 /   2 /  4   0.32        9.8e-15  2.0e-12  2.0e-12  6.1e-13  1.5e-12  1.1e-15  3.2e-15
    9      8 /   8 /   6 /  8   0.42        6.0e-15  8.3e-13  8.3e-13  2.4e-12  6.3e-13  2.0e-15  8.6e-15
    23    22 /  22 /  18 / 22   0.036       1.2e-15  1.4e-12  1.4e-12  4.9e-10  3.3e-13  7.8e-15  6.1e-16
    77    62 /  75 /  72 / 61   0.089       1.9e-15  8.1e-13  8.5e-12  2.6e-07  4.8e-13  4.2e-14  7.0e-16
    79    66 /  78 /  73 / 66   0.0085      1.4e-15  6.9e-13  9.6e-12  7.2e-07  4.8e-13  4.3e-14  1.3e-15
    87    71 /  86 /  77 / 71   0.011       2.0e-15  1.7e-12  8.6e-12  4.9e-07  8.4e-13  4.8e-14  1.0e-15
    96    77 /  96 /  80 / 76   0.014       3.0e-15  6.3e-13  1.6e-11  1.3e-07  2.4e-13  5.3e-14  8.6e-16
    97    81 /  97 /  88 / 79   0.030       2.6e-15  7.5e-13  9.8e-12  1.2e-06  6.9e-13  5.4e-14  1.1e-15
    107   88 / 106 /  94 / 88   0.041       2.2e-15  4.7e-13  7.6e-12  1.1e-06  5.0e-13  6.2e-14  1.4e-15
    111   84 / 106 /  96 / 84   0.025       3.4e-15  2.3e-12  7.8e-11  1.6e-07  2.1e-12  6.7e-14  2.6e-15

C = 111 stands where kMargMaxC = 112 (the capacity of k_marg's arrays) would: kb_create admits no handle of C > 111, so
112 cannot run (the two refused rigs of the table, C = 112 and 113, are refused there; the marginal entry points
refuse no width themselves).

At the state after one GN step (the warm chains' second state, variant (a); C = 23, 79, 107): ranks 22, 66, 88, margins
0.41, 0.18, 0.24, x spread 2.7e-13 .. 8.8e-13.  The device-loop rigs (C = 79, 97): 4 iterations each, ranks 66 and 81 in
every iteration.
"""
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

from . import marginal_cases as MC
from .test_solve_layout import header_constants

# bounds on the reference spread, a factor 10 or so above the table in the docstring: the oracle and LAPACK are the two
# referees of the GPU module, and its bars assume they agree to this
SV_SPREAD_MAX = 1e-13
X_SPREAD_MAX = {"a": 1e-10, "b": 1e-10, "c": MC.X_SPREAD_MAX, "d": 1e-10}
CASES = [(C, v) for C in MC.ROWS for v in MC.VARIANTS]


def test_table_covers_the_regimes():
    for C, r in MC.ROWS.items():
        assert MC.regime(C) == r.regime, C
        assert sum(MC.synth.NINTR[m] for m in r.models) + 6 * (len(r.models) - 1) == C
    # the restated constants: the last staged C, the largest full-storage C, the largest C
    assert MC.regime(78) == MC.FULL_STAGED and MC.regime(79) == MC.FULL_GLOBAL
    assert MC.regime(MC.K_MARG_FULL_MAX_C) == MC.FULL_GLOBAL and MC.regime(MC.K_MARG_FULL_MAX_C + 1) == MC.PACKED
    assert MC.regime(MC.K_MARG_MAX_C) == MC.PACKED and MC.regime(MC.K_MARG_MAX_C + 1) == MC.REFUSED
    assert list(MC.REFUSED_ROWS) == [112, 113] and MC.regime(113) == MC.REFUSED
    assert max(MC.ROWS) == MC.K_CREATE_MAX_C < min(MC.REFUSED_ROWS) and MC.regime(MC.K_CREATE_MAX_C) == MC.PACKED
    odd = [C for C in MC.ROWS if C & 1]
    assert {MC.ROWS[C].regime for C in odd} == {MC.FULL_STAGED, MC.FULL_GLOBAL, MC.PACKED}
    assert {96, 97, 111} <= set(MC.ROWS) and 77 in MC.ROWS and 79 in MC.ROWS
    assert [MC.ROWS[C].regime for C in MC.WARM_ROWS] == [MC.FULL_STAGED, MC.FULL_GLOBAL, MC.PACKED]
    assert [MC.LOOP_ROWS[C].regime for C in MC.LOOP_ROWS] == [MC.FULL_GLOBAL, MC.PACKED]
    assert all(MC.regime(C) == r.regime and C == r.C for C, r in MC.LOOP_ROWS.items())


def _k_marg_static_lds(tmp_path):
    """{kFull: group_segment_fixed_size} of the two k_marg instantiations, from the gfx950 code objects of the built
    library (the metadata notes list a kernel's fields in alphabetical order: the size precedes the name)"""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    lib = shutil.copy(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kalibr_amd",
                                   "libkalibr_hip.so"), str(tmp_path))
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
            m = re.match(r"\s*\.name:\s*\S*k_margILb([01])E", line)
            if m:
                out[bool(int(m.group(1)))] = size
    return out


def test_k_marg_fits_the_lds_at_every_width(tmp_path):
    """static + dynamic LDS of k_marg within the 160 KB of a workgroup at every C a handle admits -- beyond it
    hipFuncSetAttribute refuses the launch (C = 95, 96 and 111, while the gated tail's chains were a static array)"""
    static = _k_marg_static_lds(tmp_path)
    print(f"k_marg static LDS: full {static[True]} B, packed {static[False]} B")
    # the parse took k_marg's own figures: the declared arrays and at most a few scalars beside them (a neighbouring
    # kernel's size, or the tail's chains back in a static array, falls outside)
    assert set(static) == {True, False}, static
    assert 0 <= static[False] - MC.K_MARG_STATIC_MIN <= 256, static
    assert 0 <= static[True] - MC.K_MARG_STATIC_MIN - MC.K_MARG_STATIC_FULL_ONLY <= 256, static
    for C in range(1, MC.K_CREATE_MAX_C + 1):
        assert MC.marg_lds_bytes(C) + static[MC.marg_full(C)] <= MC.LDS_BYTES, C
    # as wide as the kernel's own limit, which no handle reaches
    assert MC.marg_lds_bytes(MC.K_MARG_MAX_C) + static[False] <= MC.LDS_BYTES
    # kb_solve_layout.h's marg_fits adds this bound to the dynamic size: both instances are within it
    bound = header_constants(tmp_path)["st_marg"]
    assert max(static.values()) <= bound, (static, bound)


@pytest.mark.parametrize("C", list(MC.ROWS) + list(MC.REFUSED_ROWS))
def test_rig_synthesises(C):
    r = MC.ROWS[C] if C in MC.ROWS else MC.REFUSED_ROWS[C]
    p = MC.problem(C) if C in MC.ROWS else MC.problem_of(r)
    assert (p.n_cams, p.n_frames, p.cam_cols) == (len(r.models), r.n_frames, C)
    assert p.cam_model.tolist() == list(r.models)
    assert p.n_views > 0 and np.all(np.diff(p.view_offset) > 0)
    assert p.n_corners < 20000  # "a few thousand corners": one k_marg block, a build of a few blocks


def test_reduction_matches_the_oracle():
    """reduced() (numpy, LAPACK's solves of the frame blocks) against the oracle's Schur reduction"""
    for C in (23, 97):
        R = MC.ref(C)
        S, b, hd = R.reduced("A")
        A = R.arrow("A")
        ok, So, bo = R.o.schur_partial(A, 0.0, 0, R.p.n_frames)
        assert ok
        assert np.abs(S - (A["Hcc"] - So)).max() <= 1e-12 * np.abs(S).max()
        assert np.abs(b - (A["gc"] - bo)).max() <= 1e-10 * np.abs(b).max()
        assert np.array_equal(hd, np.diag(A["Hcc"]))


@pytest.mark.parametrize("C,variant", CASES)
def test_tolerance_margin_rank_and_spread(C, variant):
    R = MC.ref(C)
    ok, dx, info = R.oracle_solve("A", variant)
    L = R.ref("A", variant)
    f = R.floors("A", variant)
    mg = MC.margin(info["sv"], info["tol"], info["rank"])
    print(f"C = {C} ({variant}): rank {info['rank']} margin {mg:.3g} gap {info['gap']:.3g} sv {f['sv']:.1e} "
          f"x {f['x']:.1e} V^T V - I {f['orth']:.1e} off-diagonal {f['offd']:.1e} diagonal {f['diag']:.1e}")
    assert ok and np.isfinite(dx).all()
    assert mg >= MC.TOL_MARGIN                      # a condition of the case, not a measurement
    assert MC.margin(L["sv"], L["tol"], L["rank"]) >= MC.TOL_MARGIN
    assert info["rank"] == L["rank"]
    assert info["tol"] == pytest.approx(L["tol"], rel=1e-12)
    assert f["sv"] <= SV_SPREAD_MAX and f["x"] <= X_SPREAD_MAX[variant]
    assert max(f["orth"], f["offd"], f["diag"]) <= 1e-12
    # the statistics: the oracle's against rank_stats on its own singular values
    tol, rank, gap, l2 = MC.rank_stats(info["sv"], C, R.opts(variant))
    assert rank == info["rank"] and info["log2sum"] == pytest.approx(l2, rel=1e-12)
    assert info["gap"] == gap if np.isinf(gap) else info["gap"] == pytest.approx(gap, rel=1e-12)
    # what the variant is there for
    if variant == "a" and C >= 77:
        assert info["rank"] < C                     # truncation is the normal regime of the large rigs
    if variant == "b":
        assert info["rank"] >= R.oracle_solve("A", "a")[2]["rank"] and info["rank"] >= C - 6
    if variant == "c":
        assert not R.opts("c")["column_scaling"] and info["tol"] == MC.ROWS[C].svd_tol and info["rank"] < C
        assert np.all(L["G"] == 1.0)
    if variant == "d":
        zero = L["G"] == 0.0
        eps_norm, n_cut = MC.eps_norm_cut(R.reduced("A")[2], R.n_rows)
        assert zero.sum() == n_cut >= 1 and eps_norm > MC.EPS
        assert np.all(dx[:C][zero] == 0.0) and np.all(L["x"][zero] == 0.0)
        assert np.all(info["sv"][C - n_cut:] == 0.0)
    else:
        assert np.all(L["G"] > 0.0)


@pytest.mark.parametrize("C", list(MC.ROWS))
def test_analyze_margin_and_rank(C):
    """analyzeMarginal (unscaled, rankTol = sv_0 1e-6 C) under the same conditions, at both states of a warm row"""
    R = MC.ref(C)
    for which in ("A", "B") if C in MC.WARM_ROWS else ("A",):
        A = R.analyze(which)
        print(f"C = {C} ({which}): analyze rank {A['info']['rank']} margin {A['margin']:.3g}")
        assert A["margin"] >= MC.TOL_MARGIN and A["info"]["rank"] == A["rank_ref"]
        assert np.abs(A["info"]["sv"] - A["sv_ref"]).max() <= SV_SPREAD_MAX * A["sv_ref"][0]


def test_one_view_rig():
    """the one-frame rig of test_gpu_marginal.py::test_one_view_is_rank_deficient: rank-deficient in the oracle, its
    tolerance clear of the singular values, LAPACK agreeing on the rank and on x"""
    p = MC.synth.make_config(1, n_frames=1)
    R = MC.Ref(p)
    ok, dx, info = R.oracle_solve("A")
    L, f = R.ref("A"), R.floors("A")
    print(f"one view: rank {info['rank']} of {R.C}, margin {MC.margin(info['sv'], info['tol'], info['rank']):.3g}, "
          f"x spread {f['x']:.1e}")
    assert ok and info["rank"] == L["rank"] < R.C
    assert MC.margin(info["sv"], info["tol"], info["rank"]) >= MC.TOL_MARGIN
    assert f["sv"] <= SV_SPREAD_MAX and f["x"] <= MC.X_SPREAD_TIGHT


def test_null_direction_of_the_omni_radtan_rig():
    """C = 9: one direction of the scaled system is null to rounding (the gap at the defaults is ~1e10)"""
    info = MC.ref(9).oracle_solve("A", "a")[2]
    assert info["rank"] == 8 and info["gap"] > 1e8


@pytest.mark.parametrize("C", MC.WARM_ROWS)
def test_warm_chain_states(C):
    """the second state of the warm chains (one step of the oracle's GN + marginal loop) meets the same conditions and
    is a different system of the same rank"""
    R = MC.ref(C)
    ok, dx, info = R.oracle_solve("B")
    L, f = R.ref("B"), R.floors("B")
    assert ok and info["rank"] == L["rank"] == R.oracle_solve("A")[2]["rank"]
    assert MC.margin(info["sv"], info["tol"], info["rank"]) >= MC.TOL_MARGIN
    assert f["sv"] <= SV_SPREAD_MAX and f["x"] <= MC.X_SPREAD_TIGHT
    assert np.abs(R.state("B") - R.state("A")).max() > 1e-3
    assert np.abs(info["sv"] - R.oracle_solve("A")[2]["sv"]).max() > 1e-6 * info["sv"][0]


@pytest.mark.parametrize("C", list(MC.LOOP_ROWS))
def test_device_loop_rigs_converge_and_keep_their_rank(C):
    R = MC.loop_ref(C)
    it, J, st, ranks = MC.oracle_loop(R)
    st_o, r_o = R.o.optimize(R.p.state_init, policy="gn", marg=O.marg_opts(R.n_rows), **MC.LOOP)
    print(f"C = {C}: {it} iterations, ranks {ranks}")
    assert it == r_o["iterations"] and 2 <= it < MC.LOOP["max_iterations"]
    assert r_o["failed_iterations"] == 0 and not r_o["linear_solver_failure"]
    assert np.array_equal(st, st_o) and J == r_o["J_final"]
    assert len(set(ranks)) == 1 and ranks[-1] == r_o["solve_info"]["rank"] < C


def test_zero_corner_frame_fails_in_the_oracle():
    p = MC.fail_problem()
    h = MC.problem(MC.FAIL_C)
    assert p.n_frames == h.n_frames and p.n_views == h.n_views and p.n_corners < h.n_corners
    assert p.view_offset[-1] == p.view_offset[-2]
    o = O.Oracle(p)
    ok, _, _ = o.solve_marginal(o.arrow(p.state_init))
    assert not ok
    # without that frame the rig is healthy again
    sub = p.frame_slice(0, p.n_frames - 1)
    os_ = O.Oracle(sub)
    ok, dx, info = os_.solve_marginal(os_.arrow(sub.state_init))
    assert ok and np.isfinite(dx).all()
    assert MC.margin(info["sv"], info["tol"], info["rank"]) >= MC.TOL_MARGIN
