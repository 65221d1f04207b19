"""Robust terms on the pipelined build and the fused GN pass: kb_set_robust_build(h, KB_ROBUST_BUILD_PIPE) keeps a
weighted handle on kb_create's k_buildp layout (the weighted k_buildp instantiations) and brings the fused GN entry
points back.  Checked against the numpy restatement tests/robust_ref.py, against a fresh unweighted handle (identity
factors through the weighted kernel: bitwise) and against the KB_ROBUST_BUILD_GENERAL handle (k_build<.., WT>) on a rig
too large for the dense restatement.

Bounds (the project's bars, as tests/test_gpu_robust.py): cost rel 1e-12; blocks, rhs and rhs^T H rhs rel 1e-10 of the
block max; build cost rel 1e-11; optimizer runs: the same iteration counts and accept column, J_final rel 1e-9, J_start
rel 1e-12, state abs 1e-6.  Device against device (PIPE against GENERAL) twice those, since each kernel carries one
bar against the exact answer.  Bitwise where stated: a factor of identity matrices scales by sqrt(1) * 1 (exact), and
1 * x + 0 * y is exact under FMA contraction."""
import numpy as np
import pytest

from kalibr_amd import synth

from . import robust_ref as R
from . import test_gpu_robust as T

pytestmark = pytest.mark.gpu

BLOCKS = T.BLOCKS
COMBOS = T.COMBOS
OPT = T.OPT
# rigs of this file beside tests/test_gpu_robust.py's (c4_small, c4_7, c6_small, c1_12, c2_small come from there)
MORE_RIGS = {
    "c3_small": lambda: synth.make_config(3, n_frames=40, p_view=0.8),  # N = 4, omni-radtan + EUCM, C = 48: 8-wave unit
    # 150 build blocks of 2 frames: the smallest size at which the next-frame prefetch inside a block runs
    "c4_300": lambda: synth.make_config(4, n_frames=300, p_view=0.7),
}
_more = {}


@pytest.fixture(scope="module")
def capi():
    from kalibr_amd import capi as K
    return K


def rig(oracle_mod, name):
    """(contaminated problem, oracle | None, Jacobian cache, clean problem); c4_300 gets no oracle (device only)"""
    if name in T.RIGS:
        return T.rig(oracle_mod, name)
    if name not in _more:
        clean = MORE_RIGS[name]()
        p, _ = R.contaminate(clean, T.SEED)
        _more[name] = (p, oracle_mod.Oracle(p) if name != "c4_300" else None, {}, clean)
    return _more[name]


def variant(oracle_mod, name, est, inv):
    p, o, cache, _ = rig(oracle_mod, name)
    kind, param = T.ESTIMATORS[est]
    return R.Robust(o, kind, param, T.invR_of(inv, p.n_corners), cache=cache)


def solver(capi, p, est, inv, mode="pipe", mode_first=True):
    g = capi.Solver(p)
    kind, param = T.ESTIMATORS[est]
    if mode_first:
        g.set_robust_build(mode)
    g.set_mestimator(kind, param)
    g.set_corner_invR(T.invR_of(inv, p.n_corners))
    if not mode_first:
        g.set_robust_build(mode)
    return g


_rel = T._rel


# ---------------------------------------------------------------- the rigs are what the cases need
def test_c4_small_covers_the_view_shapes(oracle_mod):
    p = rig(oracle_mod, "c4_small")[0]
    n = np.diff(np.asarray(p.view_offset, dtype=np.int64))
    present = np.zeros((p.n_frames, p.n_cams), dtype=bool)
    present[np.asarray(p.view_frame), np.asarray(p.view_cam)] = True
    print(p.n_cams, p.n_frames, int(present.sum()), int(n.min()), int(n.max()))
    assert p.n_cams == 8 and int(present.sum()) == 131 and p.n_frames * p.n_cams == 192
    assert np.any(n <= 64) and np.any(n > 64) and not present.all()  # a one-pass view, two-pass views, an absent view
    assert n.min() >= 32 and n.max() <= 120


# ---------------------------------------------------------------- 1. cost, weights, blocks
@pytest.mark.parametrize("name", ["c4_small", "c4_7", "c3_small", "c6_small"])
def test_cost_weights_and_blocks(capi, oracle_mod, name):
    p = rig(oracle_mod, name)[0]
    for est, inv in COMBOS:
        ref = variant(oracle_mod, name, est, inv)
        S1 = ref.system(p.state_init, True)
        S0 = ref.system(p.state_init, False)
        g = solver(capi, p, est, inv)
        assert g.build_kernel_name() == "k_buildp"
        g.set_state(p.state_init)
        J = g.eval_cost()
        w, s = g.mestimator_weights()
        assert abs(J - S1["cost"]) <= 1e-12 * S1["cost"]
        assert T._close(s, S1["s"], 1e-12) and T._close(w, S1["w"], 1e-12)
        g.build(True)
        B = g.normal_blocks()
        print(name, est, inv, J, S1["cost"], B["cost"], {k: _rel(B[k], S1[k]) for k in BLOCKS})
        for k in BLOCKS:
            assert _rel(B[k], S1[k]) < 1e-10, (est, inv, k, _rel(B[k], S1[k]))
        assert _rel(g.rhs(), S1["rhs"]) < 1e-10
        assert abs(B["cost"] - S1["cost"]) <= 1e-11 * S1["cost"]  # H[15][15] = sum w s
        want = float(S1["rhs"] @ S1["H"] @ S1["rhs"])
        assert abs(g.rhs_jtj_rhs() - want) <= 1e-10 * abs(want)
        g.build(False)  # the invR-only system, while the cost stays weighted
        B0 = g.normal_blocks()
        for k in BLOCKS:
            assert _rel(B0[k], S0[k]) < 1e-10, (est, inv, k, "invR only", _rel(B0[k], S0[k]))
        assert abs(g.eval_cost() - S1["cost"]) <= 1e-12 * S1["cost"]
        assert g.build_kernel_name() == "k_buildp"
        g.close()


# ---------------------------------------------------------------- 2. identity through the weighted kernel
@pytest.mark.parametrize("name", ["c4_small", "c4_300"])
def test_identity_factors_are_bitwise_the_unweighted_handle(capi, oracle_mod, name):
    p = rig(oracle_mod, name)[0]

    def outputs(g):
        g.set_state(p.state_init)
        g.build()
        B = g.normal_blocks()
        out = [B[k] for k in BLOCKS] + [np.array([B["cost"]]), g.rhs()]
        g.run_gn(3)
        out.append(g.get_state())
        g.set_state(p.state_init)
        r = g.optimize(policy="lm", max_iterations=4)
        out += [r["trace"], g.get_state()]
        return out

    a = capi.Solver(p)
    g = capi.Solver(p)
    g.set_robust_build("pipe")
    g.set_corner_invR(np.tile([1.0, 0.0, 1.0], (p.n_corners, 1)))
    assert a.build_kernel_name() == "k_buildp" and g.build_kernel_name() == "k_buildp"
    names = list(BLOCKS) + ["build cost", "rhs", "state after run_gn(3)", "LM trace", "state after 4 LM iterations"]
    for what, x, y in zip(names, outputs(a), outputs(g)):
        print(name, what, float(np.nanmax(np.abs(np.asarray(x) - np.asarray(y)))) if np.asarray(x).size else 0.0)
        assert np.array_equal(x, y, equal_nan=True), what
    a.close()
    g.close()


# ---------------------------------------------------------------- 3. multi-frame blocks: PIPE against GENERAL
def test_multi_frame_blocks_against_the_general_build(capi, oracle_mod):
    p = rig(oracle_mod, "c4_300")[0]
    assert p.n_corners == 196165
    out = {}
    for mode in ("general", "pipe"):
        g = solver(capi, p, "huber", "per_corner", mode=mode)
        assert g.build_kernel_name() == ("k_buildp" if mode == "pipe" else "k_build")
        g.set_state(p.state_init)
        J = g.eval_cost()
        g.build()
        B = g.normal_blocks()
        rhs = g.rhs()
        res = g.optimize(policy="gn", max_iterations=4, **OPT)
        out[mode] = dict(J=J, B=B, rhs=rhs, res=res, st=g.get_state())
        g.close()
    a, b = out["general"], out["pipe"]
    # no decision of the GENERAL run is marginal (GN accepts every step: the convergence tests only)
    tr = a["res"]["trace"]
    Js = np.concatenate([[a["res"]["J_start"]], tr[:, 0]])
    dJ, dX = np.abs(Js[:-1] - Js[1:]), tr[:, 2]
    print("general trace", tr.tolist(), dJ.tolist())
    assert np.all(np.abs(dJ - OPT["eps_j"]) >= 1e-3 * OPT["eps_j"]) and np.all(np.abs(dX - OPT["eps_x"]) >= 1e-3 * OPT["eps_x"])
    assert a["J"] == b["J"]  # both k_cost_w
    for k in BLOCKS:
        print(k, _rel(b["B"][k], a["B"][k]))
        assert _rel(b["B"][k], a["B"][k]) < 2e-10, k
    print("rhs", _rel(b["rhs"], a["rhs"]), "build cost", a["B"]["cost"], b["B"]["cost"])
    assert _rel(b["rhs"], a["rhs"]) < 2e-10
    assert abs(b["B"]["cost"] - a["B"]["cost"]) <= 2e-11 * a["B"]["cost"]
    ra, rb = a["res"], b["res"]
    print(ra["iterations"], rb["iterations"], ra["J_final"], rb["J_final"], float(np.abs(a["st"] - b["st"]).max()))
    assert ra["iterations"] == rb["iterations"] and ra["failed_iterations"] == rb["failed_iterations"]
    assert np.array_equal(ra["trace"][:, 3], rb["trace"][:, 3])
    assert abs(rb["J_final"] - ra["J_final"]) <= 2e-9 * ra["J_final"]
    assert np.abs(a["st"] - b["st"]).max() <= 2e-6


# ---------------------------------------------------------------- 4. optimizer against the restatement
OPT_CASES = [
    ("c4_small", "gn", "cauchy", "per_corner", 8),
    ("c4_small", "gn", "huber", "iso", 8),
    ("c6_small", "gn", "cauchy", "per_corner", 8),
    ("c6_small", "gn", "huber", "iso", 8),
    ("c4_7", "gn", "cauchy", "per_corner", 8),
    ("c4_small", "lm", "huber", "per_corner", 30),
    ("c3_small", "lm", "huber", "per_corner", 30),
    ("c6_small", "lm", "huber", "per_corner", 30),
]
_opt_cache = {}


def opt_reference(oracle_mod, case):
    if case in T.OPT_CASES:  # shared with tests/test_gpu_robust.py (computed once)
        return T.opt_reference(oracle_mod, case)
    if case not in _opt_cache:
        name, policy, est, inv, max_it = case
        p = rig(oracle_mod, name)[0]
        st, res = variant(oracle_mod, name, est, inv).optimize(p.state_init, policy=policy, max_iterations=max_it, **OPT)
        res["worst"] = R.assert_not_marginal(res, OPT["eps_x"], OPT["eps_j"])
        _opt_cache[case] = (st, res)
    return _opt_cache[case]


@pytest.mark.parametrize("case", OPT_CASES, ids=lambda c: "-".join(map(str, c[:4])))
def test_optimize_matches_the_restatement(capi, oracle_mod, case):
    name, policy, est, inv, max_it = case
    st_r, r = opt_reference(oracle_mod, case)
    p = rig(oracle_mod, name)[0]
    runs = []
    for use_graph, sync_every in ((True, 4), (False, 1), (True, 4)):
        g = solver(capi, p, est, inv)
        g.set_state(p.state_init)
        res = g.optimize(policy=policy, max_iterations=max_it, use_graph=use_graph, sync_every=sync_every, **OPT)
        assert g.build_kernel_name() == "k_buildp"
        runs.append((res, g.get_state()))
        g.close()
    res, st = runs[0]
    print(case, res["iterations"], res["failed_iterations"], res["J_final"], r["J_final"], r["worst"],
          float(np.abs(st - st_r).max()))
    assert res["iterations"] == r["iterations"] and res["failed_iterations"] == r["failed_iterations"]
    assert r["iterations"] >= 2 and res["linear_solver_failure"] == 0
    assert np.array_equal(res["trace"][:, 3], r["trace"][:, 3])
    assert abs(res["J_final"] - r["J_final"]) <= 1e-9 * r["J_final"]
    assert abs(res["J_start"] - r["J_start"]) <= 1e-12 * r["J_start"]
    assert np.abs(st - st_r).max() <= 1e-6
    for res2, st2 in runs[1:]:  # graph and eager runs, and two runs, are bitwise equal
        assert np.array_equal(st, st2) and res2["J_final"] == res["J_final"]
        assert np.array_equal(res2["trace"], res["trace"], equal_nan=True)


# ---------------------------------------------------------------- 5. fixed-count fused GN
def test_fixed_count_fused_gn(capi, oracle_mod):
    p = rig(oracle_mod, "c4_small")[0]
    est, inv = "cauchy", "per_corner"
    st_r, r = variant(oracle_mod, "c4_small", est, inv).optimize(p.state_init, policy="gn", max_iterations=3, **OPT)
    assert r["iterations"] == 3  # stopped by the count, as kb_run_gn_iterations is
    g = solver(capi, p, est, inv)
    g.set_state(p.state_init)
    g.run_gn(3)
    st = g.get_state()
    print(float(np.abs(st - st_r).max()))
    assert np.abs(st - st_r).max() <= 1e-6
    g.set_state(p.state_init)
    g.gn_prepare(3)
    g.gn_launch(3)
    assert np.array_equal(g.get_state(), st)
    g.close()


# ---------------------------------------------------------------- 6. mode semantics
@pytest.mark.parametrize("name", ["c1_12", "c2_small"])
def test_pipe_is_refused_on_k_build_rigs(capi, oracle_mod, name):
    p = rig(oracle_mod, name)[0]
    g = T.solver(capi, p, "huber", "per_corner")
    g.set_state(p.state_init)
    J0 = g.eval_cost()
    with pytest.raises(capi.KbError, match="kb_set_robust_build.*builds with k_build"):
        g.set_robust_build("pipe")
    assert g.build_kernel_name() == "k_build" and g.eval_cost() == J0
    with pytest.raises(capi.KbError, match="not available on a weighted handle"):
        g.run_gn(2)
    g.set_robust_build("general")  # the default is always accepted
    g.close()
    f = capi.Solver(p)  # an unweighted handle of the rig is refused as well
    with pytest.raises(capi.KbError, match="kb_set_robust_build"):
        f.set_robust_build("pipe")
    assert capi.lib().kb_set_robust_build(f.h, 2) < 0 and b"kb_set_robust_build: unknown mode" in capi.lib().kb_last_error()
    f.close()


def test_pipe_is_refused_on_a_sharded_handle(capi, oracle_mod):
    p = rig(oracle_mod, "c4_7")[0]
    s = capi.Solver(p)
    s.comm_init(capi.comm_unique_id(), 1, 0)
    s.set_state(p.state_init)
    J0 = s.eval_cost()
    with pytest.raises(capi.KbError, match="kb_set_robust_build.*unsharded"):
        s.set_robust_build("pipe")
    assert s.build_kernel_name() == "k_buildp" and s.eval_cost() == J0
    s.close()


def test_mode_and_weights_in_either_order_and_back(capi, oracle_mod):
    p = rig(oracle_mod, "c4_small")[0]
    outs = []
    for mode_first in (True, False):
        g = solver(capi, p, "huber", "per_corner", mode_first=mode_first)
        assert g.build_kernel_name() == "k_buildp"
        g.set_state(p.state_init)
        g.build()
        B = g.normal_blocks()
        outs.append([B[k] for k in BLOCKS] + [np.array([B["cost"]])])
        if mode_first:
            g.close()
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    # back to GENERAL: k_build and the refusal again, the system within the device-against-device bars
    g.run_gn(2)
    g.set_robust_build("general")
    assert g.build_kernel_name() == "k_build"
    with pytest.raises(capi.KbError, match="kb_run_gn_iterations: not available on a weighted handle"):
        g.run_gn(2)
    g.set_state(p.state_init)
    g.build()
    B = g.normal_blocks()
    for k, y in zip(BLOCKS, outs[0]):
        assert _rel(B[k], y) < 2e-10, k
    # the mode survives clearing the settings
    g.set_robust_build("pipe")
    g.set_mestimator("none")
    g.set_corner_invR(None)
    g.set_mestimator("cauchy", 4.0)
    assert g.build_kernel_name() == "k_buildp"
    g.run_gn(1)
    g.close()


def test_still_refused_paths_leave_the_handle_usable(capi, oracle_mod):
    p = rig(oracle_mod, "c4_7")[0]
    want = variant(oracle_mod, "c4_7", "huber", "none").cost(p.state_init)
    g = solver(capi, p, "huber", "none")
    g.set_state(p.state_init)
    g.build()
    refused = {
        "dog-leg": lambda: g.optimize(policy="dogleg", max_iterations=2),
        "kb_dogleg_step": lambda: g.dogleg_step(1.0),
        "kb_solve_marginal": lambda: g.solve_marginal(),
        "kb_analyze_marginal": lambda: g.analyze_marginal(),
        "kb_optimize_marginal": lambda: g.optimize_marginal(max_iterations=2),
        "kb_drop_last_frames": lambda: g.drop_last_frames(1),
        "kb_comm_init": lambda: g.comm_init(capi.comm_unique_id(), 1, 0),
        "kb_comm_init_local": lambda: capi.comm_init_local([g]),
    }
    for what, call in refused.items():
        with pytest.raises(capi.KbError, match="not available on a weighted handle") as ei:
            call()
        assert what in str(ei.value), (what, str(ei.value))
        J = g.eval_cost()  # still usable
        assert abs(J - want) <= 1e-12 * want
    rc = capi.lib().kb_append_frames(g.h, 1, 0, 0, None, None, None, None, None, None)
    assert rc < 0 and b"kb_append_frames: not available on a weighted handle" in capi.lib().kb_last_error()
    assert g.build_kernel_name() == "k_buildp"
    g.run_gn(2)  # and the fused entry points are there
    g.close()


def test_cleared_pipe_handle_is_bitwise_a_fresh_one(capi, oracle_mod):
    p = rig(oracle_mod, "c4_small")[0]

    def outputs(g):  # the outputs of tests/test_gpu_robust.py's test_cleared_handle_is_bitwise_a_fresh_one
        g.set_state(p.state_init)
        out = [np.array([g.eval_cost()])]
        g.build()
        B = g.normal_blocks()
        out += [B[k] for k in BLOCKS] + [np.array([B["cost"]])]
        g.set_constant_conditioner(1.0)
        ok, dx = g.solve()
        assert ok
        out.append(dx)
        r = g.optimize(policy="lm", max_iterations=4)
        out += [g.get_state(), r["trace"]]
        g.set_state(p.state_init)
        g.run_gn(3)
        out.append(g.get_state())
        return out

    fresh = capi.Solver(p)
    a = outputs(fresh)
    g = solver(capi, p, "huber", "per_corner")
    g.set_state(p.state_init)
    g.build()
    g.optimize(policy="lm", max_iterations=2)
    g.optimize(policy="gn", max_iterations=2)
    g.set_mestimator("none")
    g.set_corner_invR(None)
    assert g.build_kernel_name() == "k_buildp"
    for x, y in zip(a, outputs(g)):
        assert np.array_equal(x, y, equal_nan=True)
    fresh.close()
    g.close()
