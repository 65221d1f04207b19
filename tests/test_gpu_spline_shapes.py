"""The spline path (kb_sp_*) against the oracle over the shape sweep of tests/spline_cases.py: node counts 2 .. 65 of
the cyclic reduction, all three paddings of the last node, every k_sp_camsolve<CM> width, absent / short views, IMU
rates, non-uniform knots -- and the captured GN pass (kb_sp_run_gn_iterations: H_cc's column sums inside k_sp_elim1,
lambda^2 written by the build), step by step along the oracle's GN trajectory.

Bars (FP64 throughout, as tests/test_gpu_spline.py): cost rel 1e-12; normal-equation blocks and rhs rel 1e-10 of the
block's scale; GN / LM runs: identical iteration counts, J rel 1e-9, state within 1e-6.  The dx bar is
max(1e-8, 100 x floor) with floor = max|dx_band - dx_dense| / max|dx_dense| from the oracle's own two solvers at that
state and lambda (tests/test_spline_cases.py holds every floor to <= 1e-7, so no bar exceeds 1e-5; the factor 100
allows the device's cyclic reduction an elimination order of its own).  One captured pass moves the state by dx, so
its state bar is the dx bar times max(max|dx|, 1).

Every case runs everywhere: which checks a case takes is a column of the table, checked against the oracle alone in
tests/test_spline_cases.py -- nothing here is skipped or filtered at run time.
"""
import numpy as np
import pytest

from kalibr_amd import capi

from . import spline_cases as SC
from .spline_cases import rel

pytestmark = pytest.mark.gpu


# ---- part a: the separate entries (kb_sp_build / kb_sp_solve / kb_sp_apply_update, kb_sp_optimize) ----
def check_cost(g, r, tol=1e-12):
    for st in (r.p.state_init, r.p.state_truth):
        g.set_state(st)
        J, Jo = g.eval_cost(), r.o.cost(st)
        assert abs(J - Jo) <= tol * Jo, (J, Jo)


def check_system(g, r, tol_cost=1e-12):
    g.set_state(r.p.state_init)
    g.build()
    s, so = g.system(), r.sys0
    assert abs(s["cost"] - so["cost"]) <= tol_cost * so["cost"]
    for k in ("Hcc", "Hsc", "gc", "gs", "Hband"):
        assert rel(s[k], so[k]) < 1e-10, k
    assert rel(g.rhs(), np.concatenate([so["gc"], so["gs"]])) < 1e-10


def check_solves(g, r, tag):
    """dx at lambda = 10 and, where the case allows it, lambda = 0, on the system built at state_init"""
    g.set_state(r.p.state_init)
    g.build()
    todo = [(10.0, r.ok10, r.dx10, r.floor10)]
    if r.case.gn:
        todo.append((0.0, r.oks[0], r.dxs[0], r.floors[0]))
    for lam, ok_o, dx_o, floor in todo:
        g.set_constant_conditioner(lam)
        ok, dx = g.solve()
        assert ok and ok_o
        e = rel(dx, dx_o)
        print(f"[{tag}] solve lambda={lam:g}: rel(dx) {e:.2e}  floor {floor:.2e}  bar {SC.dx_bar(floor):.1e}")
        assert floor <= SC.FLOOR_MAX and e < SC.dx_bar(floor), (lam, e, floor)
    return dx  # of the last solve, which the handle still holds


def check_update(g, r, dx):
    s0 = r.p.state_init
    dX = g.apply_update()
    st_o, dX_o = r.o.apply_update(s0, dx)
    assert abs(dX - dX_o) <= 1e-15 * dX_o
    assert np.abs(g.get_state() - st_o).max() < 1e-12
    g.revert()
    assert np.array_equal(g.get_state(), s0)
    g.apply_update(dx)  # host-given dx takes the same update rules
    assert np.abs(g.get_state() - st_o).max() < 1e-12


def check_optimize(g, r, policy, tag):
    g.set_state(r.p.state_init)
    res = g.optimize(policy=policy, **SC.OPT)
    st_o, res_o = r.optimize(policy)
    dJ = abs(res["J_final"] - res_o["J_final"]) / res_o["J_final"]
    dS = np.abs(g.get_state() - st_o).max()
    print(f"[{tag}] optimize {policy}: {res['iterations']} it ({res_o['iterations']}), {res['failed_iterations']} "
          f"failed ({res_o['failed_iterations']}); J rel {dJ:.2e}  state {dS:.2e}")
    assert res["iterations"] == res_o["iterations"] and res["failed_iterations"] == res_o["failed_iterations"]
    assert dJ <= 1e-9
    assert dS < 1e-6


# ---- part b: the captured GN pass ----
def check_pass_step(g, r, k, tag, tol_cost=1e-12):
    """one captured pass from the oracle's s_k lands on its s_{k+1} = s_k (+) dx_k, and the pass's cost is the cost
    of the state it left"""
    g.set_state(r.states[k])
    g.run_gn(1)
    st = g.get_state()
    bar = SC.dx_bar(r.floors[k]) * max(np.abs(r.dxs[k]).max(), 1.0)
    e = np.abs(st - r.states[k + 1]).max()
    J, Jo = g.eval_cost(), r.o.cost(st)
    print(f"[{tag}] pass from s{k}: max|state - s{k + 1}| {e:.2e}  bar {bar:.1e}  (max|dx| "
          f"{np.abs(r.dxs[k]).max():.2e}, floor {r.floors[k]:.2e});  cost rel {abs(J - Jo) / Jo:.1e}")
    assert r.oks[k] and r.floors[k] <= SC.FLOOR_MAX
    assert e <= bar, (k, e, bar)
    assert abs(J - Jo) <= tol_cost * Jo, (J, Jo)
    return st


def check_pass(g, r, tag, steps=SC.Ref.N_STEPS):
    """the graph captured at s_0 replayed at s_1, s_2; then it_o passes from state_init against the oracle's converged
    GN run (it_o iterations) and two more against that run continued by two steps.  (it_o + 2 passes cannot be held
    to 1e-6 of the state after it_o: the oracle's own next two steps move it by 4e-6 .. 3e-2 on these cases, the
    run having stopped at dx <= 1e-3 or dJ <= 1e-3 -- so each state is compared at its own pass count.)"""
    for k in range(steps):
        check_pass_step(g, r, k, tag)
    st_o, res_o = r.optimize("gn")
    st_t, J_t = r.gn_tail(2)
    g.set_state(r.p.state_init)
    for n_pass, st_ref, J_ref in ((res_o["iterations"], st_o, res_o["J_final"]), (2, st_t, J_t)):
        g.run_gn(n_pass)
        dS = np.abs(g.get_state() - st_ref).max()
        dJ = abs(g.eval_cost() - J_ref) / J_ref
        print(f"[{tag}] +{n_pass} passes: state {dS:.2e}  J rel {dJ:.2e}")
        assert dS < 1e-6
        assert dJ <= 1e-9
    print(f"[{tag}] (the oracle's own two further steps moved its state by {np.abs(st_t - st_o).max():.1e})")


def check_pass_motion(g, name, tag):
    """a BSplineMotionError set on the handle: the pass is captured again (H_cc's sums in k_sp_reduce_cc, the motion
    term's build cost after them) and matches the oracle with the same term (cost bar 1e-10, as the motion tests of
    test_gpu_spline.py); removed, the plain pass is back"""
    g.set_motion_error(SC.W_MOTION, 2)
    check_pass_step(g, SC.ref(name, motion=True), 0, tag + " +motion", tol_cost=1e-10)
    g.set_motion_error(None)
    check_pass_step(g, SC.ref(name), 0, tag + " -motion")


@pytest.mark.parametrize("name", SC.NAMES)
def test_case(name):
    r = SC.ref(name)
    c = r.case
    g = capi.SplineSolver(r.p)
    try:
        assert (g.C, g.K) == (c.C, r.p.n_coeffs)
        check_cost(g, r)
        check_system(g, r)
        dx = check_solves(g, r, name)
        check_update(g, r, dx)
        if c.gn:
            check_optimize(g, r, "gn", name)
        if c.lm:
            check_optimize(g, r, "lm", name)
        if c.gn:
            check_pass(g, r, name)
        if c.motion:
            check_pass_motion(g, name, name)
    finally:
        g.close()


# ---- part c: the opt-in variants (read from the environment when the handle is made) ----
def _variant(monkeypatch, env, name, with_pass):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tag = name + " " + ",".join(f"{k}={v}" for k, v in env.items())
    r = SC.ref(name)
    assert r.case.gn
    g = capi.SplineSolver(r.p)
    try:
        check_cost(g, r)
        check_system(g, r)
        check_solves(g, r, tag)
        check_optimize(g, r, "gn", tag)
        if with_pass:
            check_pass(g, r, tag)
    finally:
        g.close()


@pytest.mark.parametrize("name", ["n2b", "n4", "n33"])
def test_schur_sums_in_their_own_launch(monkeypatch, name):
    """KSP_ZSF=0: k_sp_zschur instead of the extra blocks of the top level"""
    _variant(monkeypatch, {"KSP_ZSF": "0"}, name, True)


@pytest.mark.parametrize("name", ["n4", "n33"])
def test_cc_sums_separate_against_fused(monkeypatch, name):
    """KSP_CC_SEPARATE (read when the pass is captured): H_cc's column sums by k_sp_reduce_cc instead of k_sp_elim1's
    extra blocks.  Both meet the oracle within the pass bar; the two kernels add the partial rows in different orders
    (16 waves x 8 accumulators against 64 phases and a 4-ary tree), so the states agree to rounding, not bitwise --
    the bar between them is twice the pass bar."""
    r = SC.ref(name)
    out = []
    for sep in (False, True):
        if sep:
            monkeypatch.setenv("KSP_CC_SEPARATE", "1")
        g = capi.SplineSolver(r.p)
        try:
            out.append(check_pass_step(g, r, 0, name + (" cc separate" if sep else " cc fused")))
        finally:
            g.close()
    d = np.abs(out[0] - out[1]).max()
    print(f"[{name}] fused against separate: max|state difference| {d:.2e}  bitwise {np.array_equal(out[0], out[1])}")
    assert d <= 2.0 * SC.dx_bar(r.floors[0]) * max(np.abs(r.dxs[0]).max(), 1.0)
