"""k_marg through the C-ABI at the camera-block widths where it changes its code path (tests/marginal_cases.py): odd C
in full and in packed storage, the boundaries C = 96 / 97 and the largest C a handle admits (111), warm starts with V0
staged in LDS and read from global memory over a whole chain of kMargWarmMax calls and the cold restart after it,
analyzeMarginal's own warm buffer, the device loop in both storages, the options, a non-positive-definite frame block.

Two references: the oracle (the same Jacobi algorithm in the same round-robin order) and LAPACK (numpy.linalg.eigh of
the same scaled matrix, marginal_cases.ref_solve); and three figures that depend on neither and not on conditioning,
evaluated in numpy on the device's own V and sv with Omega rebuilt from the device's normal blocks.  The preconditions
(rank-tolerance margin, equal ranks of the two references, their spread) are asserted on the CPU by
test_marginal_cases.py.

Bars (FP64):
  rank                                              exact against both references
  tol                                               rel 1e-12
  gap, log2sum from the device's own sv             rel 1e-12 (marginal_cases.rank_stats; gap inf at full rank)
  gap, log2sum against the oracle                   what |sv - sv_oracle| <= 1e-11 sv_0 allows, propagated
  sv against the oracle, against LAPACK             1e-11 sv_0
  max|V^T V - I|                                    100 x the oracle V's own figure for the row, x the chain length of
                                                    a warm-started call (drift adds per warm start)
  max off-diagonal |V^T Omega V| / sv_0             100 x the oracle's own
  max ||diag(V^T Omega V)| - sv| / sv_0             100 x the oracle's own
                                                    (each per rig, state and option variant)
  solve stage: dx[:C] against G V_r diag(1/w) V_r^T G b in numpy from the device's V, signed diagonal and rank
                                                    (1e-12 + (sv_0 / sv[rank - 1]) C eps) max|dx[:C]|
  dx against the oracle                             1e-8 max|dx| where the references' own spread is <= 1e-10,
                                                    else (variant (c): unscaled, cond ~1e9) 100 x that spread
  dx on columns zeroed by eps_norm                  exactly 0.0
  projector of the kept subspace against the oracle 1e-8, where gap >= 10
  cold restart (call 33 of a chain)                 sv, V, dx bitwise those of the handle's first (cold) solve there
  device loop                                       iterations equal, J_final rel 1e-9, state 1e-6, rank equal, fused
                                                    analyze bitwise; per-call loop: same iterations, state within 1e-9

Worst measured value / bar (MI355X; the 61 cases of this module and the 12 of test_gpu_marginal.py take 3.8 s; every
figure is printed before it is asserted and the worst ratios at the module's end, under -s):
  sv against the oracle 0.021, against LAPACK 0.021        log2sum against the oracle 1.1e-4
  solves (kb_solve_marginal, cold and chained): V^T V - I 0.015     off-diagonal 0.032     diagonal 0.050
  solve stage 0.29    dx against the oracle 0.022 (unscaled: 4.6e-5 of 100 x the references' spread)
  projector 0.0032    device loop: state 2.5e-5 of 1e-6, per-call loop 0.0019 of 1e-9
  kb_analyze_marginal (the same three figures on the unscaled S, bars of marginal_cases.Ref.analyze: 100 x the oracle's
  own, an oracle figure counting as no less than one unit roundoff): V^T V - I 0.010, off-diagonal 0.19, diagonal 0.14.
  The unit-roundoff clause matters on one row: at C = 9 the oracle's off-diagonal figure is 3.5e-17 = 0.16 eps and the
  device's 4.1e-15 (18 eps of sv_0 after ~12 rotations per entry, the usual backward error of Jacobi sweeps), 1.17 of
  100 x the oracle's figure as it stands and 0.19 of 100 eps; at C = 5 (oracle 0.01 eps) the device's is 3.6e-17.

What the sweep found: at C = 95, 96 and 111 every marginal entry point failed with "invalid argument" from
hipFuncSetAttribute -- the gated tail's chains (7.5 KB) were a static LDS array beside k_marg's own, and static +
dynamic LDS passed 160 KB.  They now take the start of the dynamic LDS (marg_lds_bytes); the CPU check of the sizes is
test_marginal_cases.py::test_k_marg_fits_the_lds_at_every_width.  kMargMaxC = 112 is the capacity of k_marg's arrays
and no refusal of its own (kb_solve_layout.h asserts that it holds every admitted width): kb_create admits C <= 111, so
the rigs of C = 112 and 113 are refused there.

Not covered (no rig through the C-ABI produces them): marg_rot_wide, M1 = 1, kMargMaxSweeps exhaustion, KB_MARG_COLD
(read once per process).  The cold restart after a non-finite result is: the zero-corner frame produces one.
"""
import ctypes

import numpy as np
import pytest

from . import marginal_cases as MC
from .test_gpu_marginal import _gn_marginal_loop

pytestmark = pytest.mark.gpu

SV_BAR = 1e-11
WORST = {}


@pytest.fixture(scope="module")
def capi():
    from kalibr_amd import capi as K
    yield K
    print("\nworst value / bar: " + ", ".join(f"{k} {v:.2g}" for k, v in sorted(WORST.items())))


def _within(name, value, bar, where):
    """value <= bar, printed before it is asserted, the ratio recorded for the module docstring"""
    print(f"{where}: {name} {value:.3e} of {bar:.3e}")
    ratio = float(value) / bar if bar > 0 else (0.0 if value == 0 else float("inf"))
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    assert value <= bar, f"{where}: {name} {value:.3e} > {bar:.3e}"


def _handle(capi, p, state):
    g = capi.Solver(p)
    g.set_state(state)
    g.build()
    return g


def _options(capi, opts):
    return capi.marginal_options(**opts)


def _solve_into(capi, g, dx, opts=None):
    """kb_solve_marginal into the caller's dx (Solver.solve_marginal allocates its own)"""
    opts = opts or capi.marginal_options()
    sv, V = np.zeros(g.C), np.zeros((g.C, g.C))
    ok, inf = ctypes.c_int(0), capi.MarginalInfo()
    capi._check(capi.lib().kb_solve_marginal(g.h, ctypes.byref(opts), capi._d(dx), ctypes.byref(ok),
                                             ctypes.byref(inf), capi._d(sv), capi._d(V)))
    return bool(ok.value), g._minfo(inf, sv, V)


def _check_eig(info, Om, bars, chain, where):
    orth, offd, diag = MC.eig_figures(info["V"], info["sv"], Om)
    _within("V^T V - I", orth, bars[0] * chain, where)
    _within("off-diagonal", offd, bars[1], where)
    _within("diagonal", diag, bars[2], where)


def _check_solve(R, which, variant, ok, dx, info, blocks, chain=1):
    """every bar of a solve against the references of (state, variant); chain: the call's number in its warm chain"""
    C, opts, where = R.C, R.opts(variant, which), f"C = {R.C} ({which}, {variant}, chain {chain})"
    ok_o, dx_o, io = R.oracle_solve(which, variant)
    L, f = R.ref(which, variant), R.floors(which, variant)
    sv, V, rank = info["sv"], info["V"], info["rank"]
    assert ok and ok_o, where
    assert np.isfinite(dx).all() and np.isfinite(sv).all() and np.isfinite(V).all(), where
    assert np.all(np.diff(sv) <= 0.0), where
    assert rank == io["rank"] == L["rank"], where
    assert info["tol"] == pytest.approx(io["tol"], rel=1e-12), where
    # the statistics as formulas of the device's own singular values
    tol_s, rank_s, gap_s, l2_s = MC.rank_stats(sv, C, opts)
    assert rank_s == rank and info["tol"] == pytest.approx(tol_s, rel=1e-12), where
    if np.isinf(gap_s):
        assert info["gap"] == gap_s, where
    else:
        assert info["gap"] == pytest.approx(gap_s, rel=1e-12), where
    assert info["log2sum"] == pytest.approx(l2_s, rel=1e-12), where
    # singular values
    so, e = io["sv"], SV_BAR * io["sv"][0]
    _within("sv (oracle)", np.abs(sv - so).max(), e, where)
    _within("sv (LAPACK)", np.abs(sv - L["sv"]).max(), SV_BAR * L["sv"][0], where)
    # gap and log2sum against the oracle: what the sv bar allows
    if rank < C:
        assert info["gap"] >= (so[rank - 1] - e) / (so[rank] + e), where
        if so[rank] > e:
            assert info["gap"] <= (so[rank - 1] + e) / (so[rank] - e), where
    else:
        assert np.isinf(info["gap"]) and np.isinf(io["gap"]), where
    l2_bar = 1.01 * np.sum(e / so[:rank]) / np.log(2.0) + 1e-12 * abs(io["log2sum"])
    _within("log2sum (oracle)", abs(info["log2sum"] - io["log2sum"]), l2_bar, where)
    # the three figures that do not depend on conditioning, with Omega from the device's own blocks
    S, b, hd = MC.reduced(blocks)
    G = MC.scaling(hd, R.n_rows, opts)
    assert np.array_equal(G == 0.0, L["G"] == 0.0), where
    Om = G[:, None] * S * G[None, :]
    _check_eig(info, Om, R.bars(which, variant), chain, where)
    # the solve stage alone
    w = np.sign(np.diag(V.T @ Om @ V)) * sv
    x = MC.solve_from(V, w, rank, G, b)
    cond = sv[0] / sv[rank - 1]
    _within("solve stage", np.abs(dx[:C] - x).max(), (1e-12 + cond * C * MC.EPS) * np.abs(dx[:C]).max(), where)
    # dx, camera and frame parts, against the oracle
    assert f["x"] <= MC.X_SPREAD_MAX, where
    rel = 1e-8 if f["x"] <= MC.X_SPREAD_TIGHT else 100.0 * f["x"]
    _within("dx (oracle)" if rel == 1e-8 else "dx (oracle, unscaled)", np.abs(dx - dx_o).max(),
            rel * np.abs(dx_o).max(), where)
    zero = G == 0.0
    assert np.all(dx[:C][zero] == 0.0), where
    if variant == "d":
        assert zero.any(), where
    if io["gap"] >= 10.0:
        Vo = io["V"]
        _within("projector", np.abs(V[:, :rank] @ V[:, :rank].T - Vo[:, :rank] @ Vo[:, :rank].T).max(), 1e-8, where)


@pytest.mark.parametrize("C,variant", [(C, v) for C in MC.ROWS for v in MC.VARIANTS])
def test_cold_solve(capi, C, variant):
    R = MC.ref(C)
    g = _handle(capi, R.p, R.state("A"))
    assert g.C == C
    blocks = g.normal_blocks()
    ok, dx, info = g.solve_marginal(_options(capi, R.opts(variant)))
    _check_solve(R, "A", variant, ok, dx, info, blocks)
    g.close()


@pytest.mark.parametrize("C", list(MC.ROWS))
def test_cold_analyze(capi, C):
    """kb_analyze_marginal: the unscaled SVD at the default tolerance, its statistics included"""
    R = MC.ref(C)
    g = _handle(capi, R.p, R.state("A"))
    S = MC.reduced(g.normal_blocks())[0]
    ai, A = g.analyze_marginal(), R.analyze("A")
    where = f"C = {C} (analyze)"
    _within("sv (oracle)", np.abs(ai["sv"] - A["info"]["sv"]).max(), SV_BAR * A["info"]["sv"][0], where)
    _within("sv (LAPACK)", np.abs(ai["sv"] - A["sv_ref"]).max(), SV_BAR * A["sv_ref"][0], where)
    _check_eig(ai, S, A["bars"], 1, where)
    tol, rank, gap, l2 = MC.rank_stats(ai["sv"], C, dict(MC.DEFAULTS, column_scaling=False))
    assert ai["rank"] == rank == A["info"]["rank"] and ai["tol"] == pytest.approx(tol, rel=1e-12)
    assert ai["log2sum"] == pytest.approx(l2, rel=1e-12)
    assert ai["gap"] == gap if np.isinf(gap) else ai["gap"] == pytest.approx(gap, rel=1e-12)
    g.close()


N_CHAIN = MC.K_MARG_WARM_MAX + 2  # 34 calls: 1 cold, 2 .. 32 warm, 33 cold again, 34 warm


def _chain_length(k):
    """the number of the k-th call (from 1) in its warm chain: a cold call is 1"""
    return k if k <= MC.K_MARG_WARM_MAX else k - MC.K_MARG_WARM_MAX


def _check_chain_sweeps(sweeps):
    cold = sweeps[0]
    assert all(s < cold for s in sweeps[1:MC.K_MARG_WARM_MAX]), sweeps        # calls 2 .. 32 are warm
    assert sweeps[MC.K_MARG_WARM_MAX] == cold and sweeps[MC.K_MARG_WARM_MAX + 1] < cold, sweeps


@pytest.mark.parametrize("C", MC.WARM_ROWS)
def test_warm_chain(capi, C):
    """34 solves on one handle, alternating two states: every call meets the cold bars against its state's references,
    the warm calls take fewer sweeps, and the 33rd is the cold solve again, bit for bit"""
    R = MC.ref(C)
    g = capi.Solver(R.p)
    blocks, calls = {}, []
    for k in range(1, N_CHAIN + 1):
        which = "A" if k & 1 else "B"
        g.set_state(R.state(which))
        g.build()
        if which not in blocks:
            blocks[which] = g.normal_blocks()
        ok, dx, info = g.solve_marginal()
        _check_solve(R, which, "a", ok, dx, info, blocks[which], chain=_chain_length(k))
        calls.append((dx, info))
    _check_chain_sweeps([i["sweeps"] for _, i in calls])
    # call 33 (state A again) restarts from V = I: the first call of this handle was a fresh handle's first solve at A
    (dx1, i1), (dx33, i33) = calls[0], calls[MC.K_MARG_WARM_MAX]
    assert np.array_equal(i1["sv"], i33["sv"]) and np.array_equal(i1["V"], i33["V"]) and np.array_equal(dx1, dx33)
    # and a warm call is not that: same system, another start
    assert not np.array_equal(calls[2][1]["V"], i1["V"])
    g.close()


@pytest.mark.parametrize("C", MC.WARM_ROWS)
def test_analyze_chain_has_its_own_warm_start(capi, C):
    """the same chain for kb_analyze_marginal (a handle that only analyzes), and on a second handle a solve before
    every analyze, on that same handle, changes nothing in what its analyze chain returns"""
    R = MC.ref(C)

    def run(interleave):
        g, out = capi.Solver(R.p), []
        for k in range(1, N_CHAIN + 1):
            g.set_state(R.state("A" if k & 1 else "B"))
            g.build()
            if interleave:
                assert g.solve_marginal()[0]
            out.append(g.analyze_marginal())
        g.close()
        return out

    alone, mixed = run(False), run(True)
    for k, (a, m) in enumerate(zip(alone, mixed), 1):
        assert np.array_equal(a["sv"], m["sv"]) and np.array_equal(a["V"], m["V"]), k
        assert all(a[q] == m[q] for q in ("rank", "sweeps", "tol", "gap", "log2sum")), k
        A = R.analyze("A" if k & 1 else "B")
        where = f"C = {C} (analyze, call {k})"
        assert a["rank"] == A["info"]["rank"], where
        _within("sv (oracle)", np.abs(a["sv"] - A["info"]["sv"]).max(), SV_BAR * A["info"]["sv"][0], where)
        _within("sv (LAPACK)", np.abs(a["sv"] - A["sv_ref"]).max(), SV_BAR * A["sv_ref"][0], where)
        _check_eig(a, A["S"], A["bars"], _chain_length(k), where)
    _check_chain_sweeps([a["sweeps"] for a in alone])
    first, again = alone[0], alone[MC.K_MARG_WARM_MAX]
    assert np.array_equal(first["sv"], again["sv"]) and np.array_equal(first["V"], again["V"])


@pytest.mark.parametrize("C", list(MC.LOOP_ROWS))
def test_device_loop(capi, C):
    """kb_optimize_marginal_analyze (the gated k_marg, which sums the stage-1 column-sum rows itself, and marg_tail)
    against the oracle's GN + marginal loop at the bars of test_device_loop_with_fused_analyze, then the per-call loop
    from the same start"""
    R = MC.loop_ref(C)
    p = R.p
    st_o, r_o = R.o.optimize(p.state_init, policy="gn", marg=R.O.marg_opts(R.n_rows), **MC.LOOP)
    out = []
    for fused in (True, False):
        g = capi.Solver(p)
        assert g.C == C
        g.set_state(p.state_init)
        sol, info, ai = g.optimize_marginal(analyze=fused, **MC.LOOP)
        if not fused:
            ai = g.analyze_marginal()
        out.append((sol, info, ai, g.get_state()))
        g.close()
    (s1, i1, a1, x1), (s2, i2, a2, x2) = out
    assert s1["iterations"] == s2["iterations"] == r_o["iterations"]
    assert np.array_equal(x1, x2)
    assert abs(s1["J_final"] - r_o["J_final"]) <= 1e-9 * r_o["J_final"]
    _within("loop state", np.abs(x1 - st_o).max(), 1e-6, f"C = {C} (device loop)")
    assert i1["rank"] == i2["rank"] == r_o["solve_info"]["rank"]
    assert np.array_equal(a1["sv"], a2["sv"]) and np.array_equal(a1["V"], a2["V"]) and a1["rank"] == a2["rank"]
    assert np.abs(a1["sv"] - r_o["analyze_info"]["sv"]).max() <= 1e-9 * r_o["analyze_info"]["sv"][0]
    g = capi.Solver(p)
    g.set_state(p.state_init)
    it, J, info = _gn_marginal_loop(g, **MC.LOOP)
    assert it == s1["iterations"] and info["rank"] == i1["rank"]
    _within("per-call loop state", np.abs(g.get_state() - x1).max(), 1e-9, f"C = {C} (per-call loop)")
    g.close()


def test_zero_corner_frame_fails_and_the_handle_recovers(capi):
    """a frame without a corner: its 6 x 6 block is zero, kb_solve_marginal reports ok = 0 and leaves the caller's dx
    alone.  What that call leaves behind, read from the kernels: frame_gj divides by the zero pivot, 0 * inf = NaN goes
    through the Schur sums into every entry of S, no pair passes marg_big, the singular values are NaN and k_marg
    records chain 0 (info[5], "a non-finite result restarts cold").  So with that frame dropped the handle's next solve
    starts from V = I, bitwise a fresh handle's first solve, and the one after it is warm from that V"""
    p = MC.fail_problem()
    g = _handle(capi, p, p.state_init)
    dx = np.full(g.ncols, 7.25)
    ok, failed = _solve_into(capi, g, dx)
    assert not ok and np.all(dx == 7.25)
    assert np.isnan(failed["sv"][0])  # the largest "singular value": every entry of S was NaN
    sub = p.frame_slice(0, p.n_frames - 1)
    R = MC.Ref(sub)
    fresh = _handle(capi, sub, sub.state_init)
    dx_f = np.full(fresh.ncols, 7.25)
    ok_f, info_f = _solve_into(capi, fresh, dx_f)
    fresh.close()
    g.drop_last_frames(1)
    g.set_state(sub.state_init)
    sweeps = []
    for call in (1, 2):
        g.build()
        blocks = g.normal_blocks()
        dx = np.full(g.ncols, 7.25)
        ok, info = _solve_into(capi, g, dx)
        _check_solve(R, "A", "a", ok, dx, info, blocks, chain=call)
        sweeps.append(info["sweeps"])
        if call == 1:  # the cold restart
            assert ok_f and np.array_equal(info["sv"], info_f["sv"]) and np.array_equal(info["V"], info_f["V"])
            assert np.array_equal(dx, dx_f)
    assert sweeps[0] == info_f["sweeps"] and sweeps[1] < sweeps[0], (sweeps, info_f["sweeps"])
    g.close()


@pytest.mark.parametrize("C", list(MC.REFUSED_ROWS))
def test_widths_beyond_the_handle_are_refused_by_name(capi, C):
    """kMargMaxC = 112 is out of reach (the marginal entry points have no width refusal of their own): kb_create admits
    C <= 111"""
    with pytest.raises(capi.KbError, match="C > 111"):
        capi.Solver(MC.problem_of(MC.REFUSED_ROWS[C]))
