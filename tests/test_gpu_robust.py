"""Robust reprojection terms on the device (kb_set_mestimator, kb_set_corner_invR, kb_get_mestimator_weights and the
weighted cost / build / optimizer paths) against the numpy restatement tests/robust_ref.py over the CPU oracle's
primitives (the oracle itself has no weights).

Bounds (the project's bars): cost rel 1e-12; s and w 1e-12 relative to max(1, |value|) (s reaches ~1e4 at the gross
outliers, where an absolute 1e-12 is below one ulp); normal-equation blocks, rhs and rhs^T H rhs rel 1e-10 of the block
max; solves rel 1e-8 of max|dx|; optimizer runs: same iteration counts and accept trace, J_final rel 1e-9, state abs
1e-6; covariance blocks correlation-normalised 1e-8.

The observations are contaminated with a fixed seed (3 % of the corners shifted by 20 - 60 px), so both Huber branches
and small weights occur; this is asserted on the restatement.  Every optimizer case first asserts on the restatement's
own run that no decision is marginal (robust_ref.assert_not_marginal)."""
import math

import numpy as np
import pytest

from kalibr_amd import synth

from . import robust_ref as R

pytestmark = pytest.mark.gpu

SEED = 11  # contamination and per-corner invR
RIGS = {
    "c1_12": lambda: synth.make_config(1, n_frames=12),  # C = 8
    "c2_small": lambda: synth.make_config(2, n_frames=60),  # C = 22
    "c6_small": lambda: synth.make_config(6, n_frames=40, p_view=0.8),  # C = 42, four camera models
    "c4_small": lambda: synth.make_config(4, n_frames=24, p_view=0.7),  # N = 8, C = 106: k_build feeding k_solve<0>
    # frame counts that are no multiple of the 4 frames per k_backsub block (the clamped tail)
    "c1_5": lambda: synth.make_config(1, n_frames=5),
    "c4_7": lambda: synth.make_config(4, n_frames=7, p_view=0.7),
}
ESTIMATORS = {
    "none": (R.NONE, 0.0),
    "huber": (R.HUBER, 2.0),
    "cauchy": (R.CAUCHY, 4.0),
    "geman_mcclure": (R.GEMAN_MCCLURE, 9.0),
    "blake_zisserman": (R.BLAKE_ZISSERMAN, R.blake_zisserman_epsilon(2, 0.999, 0.1)),
}
SIGMA = 0.5
# (estimator, invR setting): every estimator and every invR setting on every rig
COMBOS = [("huber", "none"), ("cauchy", "iso"), ("geman_mcclure", "per_corner"), ("blake_zisserman", "per_corner"),
          ("none", "iso"), ("none", "per_corner"), ("huber", "per_corner")]


def per_corner_invR(n, seed=SEED):
    """anisotropic positive definite matrices with a non-zero off-diagonal: principal sigmas in [0.5, 1.5] px at a
    random angle kept away from the axes"""
    rng = np.random.default_rng(seed + 1000)
    s1, s2 = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
    th = rng.uniform(0.2, math.pi / 2 - 0.2, n)
    c, s = np.cos(th), np.sin(th)
    a, b = 1.0 / (s1 * s1), 1.0 / (s2 * s2)
    out = np.stack([a * c * c + b * s * s, (a - b) * c * s, a * s * s + b * c * c], axis=1)
    out[np.abs(out[:, 1]) < 1e-3, 1] = 0.05  # keep the off-diagonal away from zero (still PD: |0.05| << diag)
    return np.ascontiguousarray(out)


def invR_of(setting, n):
    if setting == "none":
        return None
    if setting == "iso":
        return np.array([[1.0 / SIGMA ** 2, 0.0, 1.0 / SIGMA ** 2]])
    return per_corner_invR(n)


@pytest.fixture(scope="module")
def capi():
    from kalibr_amd import capi as K
    return K


_rigs = {}


def rig(oracle_mod, name):
    """(contaminated problem, oracle, shared Jacobian cache, clean problem); built once"""
    if name not in _rigs:
        clean = RIGS[name]()
        p, idx = R.contaminate(clean, SEED)
        _rigs[name] = (p, oracle_mod.Oracle(p), {}, clean)
    return _rigs[name]


def variant(oracle_mod, name, est, inv):
    p, o, cache, _ = rig(oracle_mod, name)
    kind, param = ESTIMATORS[est]
    return R.Robust(o, kind, param, invR_of(inv, p.n_corners), cache=cache)


def solver(capi, p, est, inv):
    g = capi.Solver(p)
    kind, param = ESTIMATORS[est]
    g.set_mestimator(kind, param)
    g.set_corner_invR(invR_of(inv, p.n_corners))
    return g


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def _close(a, b, tol):
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


BLOCKS = ("Hff", "Hfc", "gf", "Hcc", "gc")


# ---------------------------------------------------------------- 1, 2. cost, weights, blocks
@pytest.mark.parametrize("name", list(RIGS))
def test_cost_weights_and_blocks(capi, oracle_mod, name):
    p = rig(oracle_mod, name)[0]
    for est, inv in COMBOS:
        ref = variant(oracle_mod, name, est, inv)
        S1 = ref.system(p.state_init, True)
        S0 = ref.system(p.state_init, False)
        if est == "huber":  # both branches and small weights occur
            k2 = ESTIMATORS[est][1] ** 2
            assert np.any(S1["s"] < k2) and np.any(S1["s"] >= k2) and S1["w"].min() < 0.1
        g = solver(capi, p, est, inv)
        g.set_state(p.state_init)
        J = g.eval_cost()
        w, s = g.mestimator_weights()
        print(name, est, inv, J, S1["cost"], float(np.abs(s - S1["s"]).max()), float(np.abs(w - S1["w"]).max()))
        assert abs(J - S1["cost"]) <= 1e-12 * S1["cost"]
        assert _close(s, S1["s"], 1e-12) and _close(w, S1["w"], 1e-12)
        g.build(True)
        B = g.normal_blocks()
        for k in BLOCKS:
            assert _rel(B[k], S1[k]) < 1e-10, (est, inv, k, _rel(B[k], S1[k]))
        assert _rel(g.rhs(), S1["rhs"]) < 1e-10
        assert abs(B["cost"] - S1["cost"]) <= 1e-11 * S1["cost"]  # H[15][15] = sum w s
        want = float(S1["rhs"] @ S1["H"] @ S1["rhs"])
        assert abs(g.rhs_jtj_rhs() - want) <= 1e-10 * abs(want)
        # use_mestimator = 0 (Optimizer2::computeHessian): the invR-only system, while the cost stays weighted
        g.build(False)
        B0 = g.normal_blocks()
        for k in BLOCKS:
            assert _rel(B0[k], S0[k]) < 1e-10, (est, inv, k, "invR only")
        assert abs(g.eval_cost() - S1["cost"]) <= 1e-12 * S1["cost"]
        assert g.build_kernel_name() == "k_build"
        g.close()


# ---------------------------------------------------------------- 3. identity
@pytest.mark.parametrize("name", ["c4_small", "c2_small"])
def test_cleared_handle_is_bitwise_a_fresh_one(capi, oracle_mod, name):
    p = rig(oracle_mod, name)[0]
    pipe = "k_buildp" if name == "c4_small" else "k_build"

    def outputs(g):
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
    assert fresh.build_kernel_name() == pipe
    a = outputs(fresh)
    g = solver(capi, p, "huber", "per_corner")
    assert g.build_kernel_name() == "k_build"
    g.set_state(p.state_init)
    g.build()
    g.optimize(policy="lm", max_iterations=2)
    g.set_mestimator("none")
    assert g.build_kernel_name() == "k_build"  # still weighted: the invR
    g.set_corner_invR(None)
    assert g.build_kernel_name() == pipe
    b = outputs(g)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    fresh.close()
    g.close()


@pytest.mark.parametrize("name", ["c4_small", "c1_5"])
def test_identity_invR_through_the_weighted_kernel(capi, oracle_mod, name):
    p = rig(oracle_mod, name)[0]
    a = capi.Solver(p)
    a.set_state(p.state_init)
    a.build()
    A = a.normal_blocks()
    g = capi.Solver(p)
    g.set_corner_invR(np.tile([1.0, 0.0, 1.0], (p.n_corners, 1)))
    assert g.build_kernel_name() == "k_build"
    g.set_state(p.state_init)
    g.build()
    B = g.normal_blocks()
    for k in BLOCKS:
        assert _rel(B[k], A[k]) <= 1e-12, k
    assert abs(g.eval_cost() - a.eval_cost()) <= 1e-12 * a.eval_cost()
    w, s = g.mestimator_weights()
    assert np.all(w == 1.0)
    a.close()
    g.close()


# ---------------------------------------------------------------- 4. solve
@pytest.mark.parametrize("name", list(RIGS))
def test_solve_against_the_dense_solve(capi, oracle_mod, name):
    p = rig(oracle_mod, name)[0]
    est, inv = ("huber", "per_corner") if name != "c6_small" else ("cauchy", "iso")
    S = variant(oracle_mod, name, est, inv).system(p.state_init, True)
    g = solver(capi, p, est, inv)
    g.set_state(p.state_init)
    g.build()
    for lam in (0.0, 1.0, 10.0):
        ok_r, dx_r = R.Robust.solve(S, lam)
        if lam == 0.0 and (not ok_r or np.linalg.cond(S["H"]) > 1e12):
            continue  # lambda = 0 only where the system is (numerically) positive definite
        g.set_constant_conditioner(lam)
        ok, dx = g.solve()
        print(name, lam, ok, _rel(dx, dx_r))
        assert ok and ok_r and _rel(dx, dx_r) < 1e-8, (name, lam)
    g.close()


def test_pcg_schur_on_a_weighted_system(capi, oracle_mod):
    p = rig(oracle_mod, "c2_small")[0]
    g = solver(capi, p, "cauchy", "per_corner")
    g.set_state(p.state_init)
    g.build()
    g.set_constant_conditioner(1.0)
    ok, dx = g.solve()
    # max_iterations = -1 would cap the run at C iterations (LinearSolverPCG's default), short of the tolerance
    g.set_linear_solver("pcg_schur", tolerance=1e-24, max_iterations=4000, absolute_tolerance=False)
    ok2, dx2 = g.solve()
    print(g.pcg_info(), _rel(dx2, dx))
    assert ok and ok2 and _rel(dx2, dx) < 1e-8
    g.close()


# ---------------------------------------------------------------- 5. optimizer
# (rig, policy, estimator, invR, max_iterations); chosen on the CPU so that no decision of the restatement is marginal
OPT_CASES = [
    ("c1_12", "lm", "huber", "per_corner", 30),
    ("c1_12", "gn", "cauchy", "iso", 8),
    ("c1_12", "lm", "geman_mcclure", "iso", 30),  # every step rejected (the weighted cost of the revert path)
    ("c2_small", "lm", "cauchy", "none", 30),
    ("c6_small", "lm", "huber", "iso", 30),
    ("c4_7", "lm", "huber", "per_corner", 30),
    ("c4_7", "gn", "cauchy", "per_corner", 8),
    ("c1_5", "lm", "huber", "iso", 30),
]
OPT = dict(lambda0=10.0, eps_x=1e-3, eps_j=1.0)
_opt_cache = {}


def opt_reference(oracle_mod, case):
    if case not in _opt_cache:
        name, policy, est, inv, max_it = case
        p = rig(oracle_mod, name)[0]
        ref = variant(oracle_mod, name, est, inv)
        st, res = ref.optimize(p.state_init, policy=policy, max_iterations=max_it, **OPT)
        res["worst"] = R.assert_not_marginal(res, OPT["eps_x"], OPT["eps_j"])
        _opt_cache[case] = (st, res)
    return _opt_cache[case]


@pytest.mark.parametrize("case", OPT_CASES, ids=lambda c: "-".join(map(str, c[:4])))
def test_optimize_matches_the_restatement(capi, oracle_mod, case):
    name, policy, est, inv, max_it = case
    st_r, r = opt_reference(oracle_mod, case)
    p = rig(oracle_mod, name)[0]
    x0 = p.state_init  # the perturbed start
    runs = []
    for use_graph, sync_every in ((True, 4), (False, 1), (True, 4)):
        g = solver(capi, p, est, inv)
        g.set_state(x0)
        res = g.optimize(policy=policy, max_iterations=max_it, use_graph=use_graph, sync_every=sync_every, **OPT)
        runs.append((res, g.get_state()))
        g.close()
    res, st = runs[0]
    print(case, res["iterations"], res["failed_iterations"], res["J_final"], r["J_final"], r["worst"])
    assert res["iterations"] == r["iterations"] and res["failed_iterations"] == r["failed_iterations"]
    assert r["iterations"] >= 2 and res["linear_solver_failure"] == 0
    assert np.array_equal(res["trace"][:, 3], r["trace"][:, 3])
    assert abs(res["J_final"] - r["J_final"]) <= 1e-9 * r["J_final"]
    assert abs(res["J_start"] - r["J_start"]) <= 1e-12 * r["J_start"]
    assert np.abs(st - st_r).max() <= 1e-6
    # graph and eager runs, and two runs, are bitwise equal
    for res2, st2 in runs[1:]:
        assert np.array_equal(st, st2) and res2["J_final"] == res["J_final"]
        assert np.array_equal(res2["trace"], res["trace"], equal_nan=True)


# ---------------------------------------------------------------- 6. it is robust
def cam_dist(p, a, b):
    """norm of the camera columns' difference (intrinsics and baselines: the state before the frame poses)"""
    n = p.n_cams * synth.MAX_INTR + 7 * (p.n_cams - 1)
    return float(np.linalg.norm(a[:n] - b[:n]))


ROBUST_KW = dict(policy="lm", max_iterations=30, lambda0=10.0, eps_x=1e-3, eps_j=1.0)


def test_cauchy_resists_the_outliers(capi, oracle_mod):
    p, o, cache, clean = rig(oracle_mod, "c2_small")
    # on the restatement first: the chosen seed shows it with a factor >= 3
    st_clean, _ = R.Robust(oracle_mod.Oracle(clean)).optimize(clean.state_init, **ROBUST_KW)
    st_plain, _ = R.Robust(o, cache=cache).optimize(clean.state_init, **ROBUST_KW)
    st_cauchy, _ = opt_reference(oracle_mod, ("c2_small", "lm", "cauchy", "none", 30))
    d_plain, d_cauchy = cam_dist(p, st_plain, st_clean), cam_dist(p, st_cauchy, st_clean)
    print("restatement:", d_plain, d_cauchy)
    assert d_plain >= 3.0 * d_cauchy
    # the same inequality on the device
    out = {}
    for key, prob, est in (("clean", clean, "none"), ("plain", p, "none"), ("cauchy", p, "cauchy")):
        g = solver(capi, prob, est, "none")
        g.set_state(clean.state_init)
        g.optimize(**ROBUST_KW)
        out[key] = g.get_state()
        g.close()
    g_plain, g_cauchy = cam_dist(p, out["plain"], out["clean"]), cam_dist(p, out["cauchy"], out["clean"])
    print("device:", g_plain, g_cauchy)
    assert g_cauchy < g_plain and g_plain >= 3.0 * g_cauchy


# ---------------------------------------------------------------- 7. covariance scaling
@pytest.mark.parametrize("name", ["c1_12", "c4_small"])
def test_covariance_scales_with_sigma(capi, oracle_mod, name):
    clean = rig(oracle_mod, name)[3]
    a = capi.Solver(clean)
    g = solver(capi, clean, "none", "iso")
    outs = []
    for s in (a, g):
        s.set_state(clean.state_truth)
        s.build()
        s.set_constant_conditioner(0.0)
        ok, out = s.covariance(cross=True)
        assert ok
        outs.append(out)
    ref, got = outs
    sc, sf = np.sqrt(np.diag(ref["Pcc"])), np.sqrt(np.einsum("fii->fi", ref["Pff"]))
    s2 = SIGMA ** 2
    e = dict(Pcc=(np.abs(got["Pcc"] - s2 * ref["Pcc"]) / (s2 * np.outer(sc, sc))).max(),
             Pff=(np.abs(got["Pff"] - s2 * ref["Pff"]) / (s2 * sf[:, :, None] * sf[:, None, :])).max(),
             Pfc=(np.abs(got["Pfc"] - s2 * ref["Pfc"]) / (s2 * sf[:, :, None] * sc[None, None, :])).max())
    print(name, e)
    assert max(e.values()) <= 1e-8, e
    a.close()
    g.close()


# ---------------------------------------------------------------- 8. errors
def test_bad_settings_are_rejected(capi, oracle_mod):
    p = rig(oracle_mod, "c1_5")[0]
    g = capi.Solver(p)
    g.set_state(p.state_init)
    J0 = g.eval_cost()
    for bad in ([1.0, 2.0, 1.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 1.0], [1.0, 0.0, float("nan")], [1.0, 1.0, 1.0]):
        with pytest.raises(capi.KbError, match="not positive definite"):
            g.set_corner_invR([bad])
    per = per_corner_invR(p.n_corners)
    per[7] = [1.0, 1.5, 1.0]
    with pytest.raises(capi.KbError, match="corner 7 is not positive definite"):
        g.set_corner_invR(per)
    with pytest.raises(capi.KbError, match="n must be 0, 1 or the number of corners"):
        g.set_corner_invR(per[:5])
    for param in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(capi.KbError, match="positive and finite"):
            g.set_mestimator("huber", param)
    m = capi.MEstimator(9, 1.0)
    assert capi.lib().kb_set_mestimator(g.h, m) < 0 and b"unknown estimator" in capi.lib().kb_last_error()
    # nothing was set: still the unweighted handle
    assert g.eval_cost() == J0 and g.build_kernel_name() == capi.Solver(p).build_kernel_name()
    g.close()


def test_refused_paths_leave_the_handle_usable(capi, oracle_mod):
    p = rig(oracle_mod, "c4_7")[0]
    ref = variant(oracle_mod, "c4_7", "huber", "none")
    want = ref.cost(p.state_init)
    g = solver(capi, p, "huber", "none")
    g.set_state(p.state_init)
    g.build()
    refused = {
        "kb_run_gn_iterations": lambda: g.run_gn(2),
        "kb_gn_prepare": lambda: g.gn_prepare(2),
        "kb_gn_launch": lambda: g.gn_launch(2),
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
    # the other call order: a sharded handle refuses the settings
    s = capi.Solver(p)
    s.comm_init(capi.comm_unique_id(), 1, 0)
    with pytest.raises(capi.KbError, match="unsharded handles only"):
        s.set_mestimator("huber", 2.0)
    with pytest.raises(capi.KbError, match="unsharded handles only"):
        s.set_corner_invR([1.0, 0.0, 1.0])
    s.close()
    # clearing both settings restores the fused GN entry points
    g.set_mestimator("none")
    g.set_corner_invR(None)
    f = capi.Solver(p)
    for h in (g, f):
        h.set_state(p.state_init)
        h.run_gn(3)
    assert np.array_equal(g.get_state(), f.get_state())
    assert g.gn_prepare(2) in (True, False)
    g.gn_launch(2)
    g.close()
    f.close()
