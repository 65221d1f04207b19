"""Preconditions of tests/test_gpu_spline_robust.py, from the restatement (tests/spline_robust_ref.py) and the oracle
alone -- no device.

  * with unit weights the restatement is the oracle: every block of SplineOracle.system and .cost (rel 1e-13; measured
    <= 4e-15), and optimize() gives the oracle's iteration counts and trace;
  * at the states of every one-step check (state_init, the restatement's converged Huber state, its state after two
    passes) each family has a term with w < 1, at the converged state at least half its terms with w = 1, and no term
    within 1e-9 (relative) of the Huber threshold k^2, so that no branch of the weight can flip on rounding (measured:
    99.8 .. 100 % of the terms in the tail at state_init; 7 % of the corners and 3 .. 6 % of the IMU terms at the
    converged state; imu_sparse has exactly one gyro and one accel term of 31 there; 8 .. 86 % of the corners after
    two passes);
  * every run the device test compares passes robust_ref.assert_not_marginal, has no failed iteration, and moves its own
    final state by <= spline_cases.LM_REPRO_MAX when the restatement's rows are summed in a permuted order (measured:
    <= 2.3e-8 on n7, n12, views, c51, knots; n4 moves by 5e-6 (GN) and 4.9e-7 (LM) and takes one-step checks only);
  * the dx floors (H against H summed in three permuted orders) of every one-step solve the device test compares are
    <= spline_cases.FLOOR_MAX, and the gradient cancels exactly for the variant and state that
    spline_robust_ref.cancels names (which solves are compared and why: spline_robust_ref.STEP_CASES);
  * the robust fit does what it is for: on n7 the Huber solution lies closer to the clean problem's GN solution than the
    unweighted fit of the same contaminated data (measured: max|dstate| 0.31 against 32.9);
  * the new setters refuse a null handle by name (the argument checks that need no device).
"""
import numpy as np
import pytest

from . import robust_ref as RR
from . import spline_cases as SC
from . import spline_robust_ref as SR

UNIT_CASES = ["n4", "n7", "n12", "views", "c51", "imu_sparse"]
STEP_CASES = list(SR.STEP_CASES)  # the device test's one-step cases
RUN_CASES = ["n7", "n12", "views", "c51", "knots"]


@pytest.mark.parametrize("name", UNIT_CASES)
def test_unit_weights_are_the_oracle(name, oracle_mod):
    p = SC.problem(name)
    o = oracle_mod.SplineOracle(p)
    r = SR.SplineRobust(o)
    for st in (p.state_init, p.state_truth):
        s, so = r.system(st), o.system(st, nthreads=4)
        for k in ("Hcc", "Hsc", "Hband", "gc", "gs"):
            assert SC.rel(s[k], so[k]) < 1e-13, (k, SC.rel(s[k], so[k]))
        assert abs(s["cost"] - so["cost"]) <= 1e-13 * so["cost"]
        assert abs(r.cost(st) - o.cost(st)) <= 1e-13 * so["cost"]


@pytest.mark.parametrize("name,policy", [("n7", "gn"), ("n7", "lm"), ("views", "lm")])
def test_unit_weight_optimize_is_the_oracles(name, policy, oracle_mod):
    p = SC.problem(name)
    o = oracle_mod.SplineOracle(p)
    st, res = SR.SplineRobust(o).optimize(p.state_init, policy=policy, **SC.OPT)
    st_o, res_o = o.optimize(p.state_init, policy=policy, nthreads=4, **SC.OPT)
    assert res["iterations"] == res_o["iterations"] and res["failed_iterations"] == res_o["failed_iterations"]
    assert res["trace"].shape == res_o["trace"].shape
    assert np.array_equal(res["trace"][:, 3], res_o["trace"][:, 3])
    # the final J to the runs' bar; the J of the passes before it only to 10 x FLOOR_MAX: the restatement solves densely,
    # the oracle by its band solver, their steps differ by up to FLOOR_MAX (relative), and away from the minimum J is
    # first order in the step
    assert abs(res["J_final"] - res_o["J_final"]) <= 1e-9 * res_o["J_final"]
    assert SC.rel(res["trace"][:, 0], res_o["trace"][:, 0]) < 10 * SC.FLOOR_MAX
    assert np.abs(st - st_o).max() < 1e-6


@pytest.mark.parametrize("name", STEP_CASES)
def test_weights_are_active_and_off_the_threshold(name):
    R = SR.ref(name)
    r = R.robust(SR.HUBER_ALL, SR.INVR)
    for which, st in enumerate(R.states()):
        for f, (s, w) in r.family_sw(st).items():
            if s.size == 0:  # imu_none
                assert f != "reprojection"
                continue
            k2 = SR.HUBER_ALL[f][1] ** 2
            tail = float(np.mean(w < 1.0))
            print(f"[{name}] state {which} {f}: {100 * tail:.1f} % of {s.size} terms in the tail")
            assert np.any(w < 1.0), (which, f)
            assert np.abs(s - k2).min() / k2 >= 1e-9, (which, f)
            if which == 1:
                assert np.mean(w == 1.0) >= 0.5, (which, f, tail)


@pytest.mark.parametrize("name,policy,kinds", [(n, pol, "huber") for n in RUN_CASES for pol in ("gn", "lm")] +
                         [("views", "gn", "cauchy")])
def test_runs_are_decided_and_reproducible(name, policy, kinds):
    R = SR.ref(name)
    opt = SR.LM_OPT if policy == "lm" else SC.OPT
    st, res = R.run(policy, kinds)
    worst = RR.assert_not_marginal(res, opt["eps_x"], opt["eps_j"])
    assert res["failed_iterations"] == 0 and not res["linear_solver_failure"]
    assert res["iterations"] < opt["max_iterations"]
    st_p, res_p = R.run(policy, kinds, SR.PERM_SEED)
    move = np.abs(st - st_p).max()
    print(f"[{name}] {policy} {kinds}: {res['iterations']} it; permuted-order run moves the state by {move:.1e}; "
          f"margins {worst}")
    assert res_p["iterations"] == res["iterations"] and res_p["failed_iterations"] == 0
    assert move <= SC.LM_REPRO_MAX


@pytest.mark.parametrize("name", STEP_CASES)
def test_one_step_floors(name):
    """every solve the device test compares (spline_robust_ref.step_lambdas) has a floor <= FLOOR_MAX (measured: a
    factor 10 or more inside it); the floors of the solves it does not compare are printed for the record.  And the
    gradient cancels (< 1e-3 of its summands' scale, gc and gs; measured 3e-8 .. 3e-5 after the GN runs, 5e-4 after
    imu_none's LM run) exactly where spline_robust_ref.cancels says, and is >= 1e-3 of it everywhere else (measured
    >= 5e-3), so the one exception to the 1e-10 bar on the gradient blocks is decided here."""
    R = SR.ref(name)
    for which, st in enumerate(R.states()):
        for tag, kinds, invR in SR.variants(R.p.n_corners):
            r = R.robust(kinds, invR)
            compared = SR.step_lambdas(name, which, tag)
            for lam, (ok, _, floor) in R.floors(r, st, (10.0, 0.0) if R.case.gn else (10.0,)).items():
                print(f"[{name}] state {which} {tag} lambda {lam:g}: floor {floor:.1e}"
                      f"{'' if lam in compared else '  (not compared)'}")
                assert ok
                if lam in compared:
                    assert floor <= SC.FLOOR_MAX, (tag, which, lam, floor)
            s = r.system(st)
            for k in ("gc", "gs"):
                ratio = np.abs(s[k]).max() / s["gscale"][k]
                print(f"[{name}] state {which} {tag}: max|{k}| is {ratio:.1e} of its summands' scale")
                assert (ratio < 1e-3) == SR.cancels(tag, which), (tag, which, k, ratio)


def test_huber_fit_is_closer_to_the_clean_solution(oracle_mod):
    R = SR.ref("n7")
    o_clean = oracle_mod.SplineOracle(R.clean)
    st_clean, res_clean = o_clean.optimize(R.clean.state_init, policy="gn", nthreads=4, **SC.OPT)
    st_h, _ = R.run("gn")
    st_u, _ = R.robust(None, None).optimize(R.p.state_init, policy="gn", **SC.OPT)
    dh, du = np.abs(st_h - st_clean).max(), np.abs(st_u - st_clean).max()
    print(f"max|state - clean GN solution|: Huber {dh:.3g}, unweighted {du:.3g}")
    assert dh < du


def test_setters_refuse_a_null_handle_by_name():
    from kalibr_amd import capi
    L = capi.lib()
    m = capi.MEstimator(1, 2.0)
    import ctypes as C
    one = np.array([1.0, 0.0, 1.0])
    w = np.zeros(1)
    for name, call in (("kb_sp_set_mestimator", lambda: L.kb_sp_set_mestimator(None, 0, C.byref(m))),
                       ("kb_sp_set_corner_invR", lambda: L.kb_sp_set_corner_invR(None, capi._d(one), 1)),
                       ("kb_sp_get_mestimator_weights", lambda: L.kb_sp_get_mestimator_weights(None, 0, capi._d(w), None))):
        assert call() < 0
        assert name in L.kb_last_error().decode()
    assert set(("kb_sp_set_mestimator", "kb_sp_get_mestimator_weights")) <= set(capi.EXPORTS)
    assert "kb_sp_set_corner_invR" in capi.EXPORTS_MIXED_CASE
    assert capi.SP_TERMS == {"reprojection": 0, "gyro": 1, "accel": 2}
