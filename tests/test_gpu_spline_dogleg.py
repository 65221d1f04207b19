"""Dog-leg trust-region policy on the spline path (kb_sp_optimize policy 2, kb_sp_dogleg_step, kb_sp_rhs_jtj_rhs,
kb_sp_get_dogleg_trace) against the restatement of the policy over the spline oracle
(tests/spline_dogleg_ref.py; its preconditions, the pinned step / accept strings among them, are in
tests/test_spline_dogleg_ref.py).

Bars: rhs_jtj_rhs, sd_scale and |dx_sd| rel 1e-10 against the oracle's blocks (the camera path's SD bar) and rel 1e-12
against the same form computed in numpy from the device's own kb_sp_get_system blocks (the new kernel alone, without
the build); beta and delta of the step primitive rel 1e-8, its dx within spline_cases.dx_bar of the case's lambda = 0
floor; runs: equal step and accept strings and counts, J_final rel 1e-9, state within 1e-6, per-pass delta, |dx_sd|,
|dx_gn| and beta within bar x max(|ref|, 1), bar the largest dx_bar over the systems the run solved (100 x the oracle's
own band-against-dense difference there, at least 1e-8) -- the bar test_gpu_spline_shapes.py derives for a pass's
state, dx_bar x max(max|dx|, 1), applied to lengths in that state space.
"""
import numpy as np
import pytest

from kalibr_amd import capi

from . import spline_cases as SC
from . import spline_dogleg_ref as D

pytestmark = pytest.mark.gpu

SD, GN, DL = D.SD, D.GN, D.DL


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _solver(p, state=None):
    g = capi.SplineSolver(p)
    g.set_state(p.state_init if state is None else state)
    return g


def _steps(dt):
    return "".join(D.STEP[int(t)] if t >= 0 else "x" for t in dt[:, 1])


def _accepts(tr):
    return "".join(str(int(a)) for a in tr[:, 3])


# ---------------------------------------------------------------- 1. quadratic form
def _check_form(g, sys_o, tag):
    """rhs_jtj_rhs, sd_scale and |dx_sd| of the built system against the oracle's blocks (sys_o, or None) and against
    the device's own blocks"""
    ghg = g.rhs_jtj_rhs()
    ok, _, info = g.dogleg_step(1e-12)  # far inside |dx_sd|: the SD branch, no solve
    assert ok and info["step_type"] == SD and info["dx_gn_norm"] == 0.0
    for what, s, tol in (("oracle", sys_o, 1e-10), ("own blocks", g.system(), 1e-12)):
        if s is None:
            continue
        want = D.g_h_g(s)
        _, sd_scale, _, sdn = D.steepest_descent(s)
        e = (_rel(ghg, want), _rel(info["sd_scale"], sd_scale), _rel(info["dx_sd_norm"], sdn))
        print(f"[{tag}] against {what}: rel g^T H g {e[0]:.2e}  sd_scale {e[1]:.2e}  |dx_sd| {e[2]:.2e}  (bar {tol:.0e})")
        assert max(e) <= tol, (what, e)
    return ghg


@pytest.mark.parametrize("name", ["n2b", "n2c", "n4", "n3", "n33", "c23", "c64", "views", "imu_none"])
def test_quadratic_form(name):
    r = SC.ref(name)
    g = _solver(r.p)
    try:
        g.build()
        _check_form(g, r.sys0, name)
    finally:
        g.close()


def test_quadratic_form_with_motion_error_and_huber():
    """n4 (K mod 3 = 1) once more with a BSplineMotionError (its Q blocks are part of D0 / U0), then with Huber on the
    reprojection family (the weights are whatever the build put into the blocks: the device's own blocks only)"""
    g = _solver(SC.problem("n4"))
    try:
        g.set_motion_error(SC.W_MOTION, 2)
        g.build()
        a = _check_form(g, SC.ref("n4", motion=True).sys0, "n4 +motion")
        g.set_motion_error(None)
        g.set_mestimator("reprojection", "huber", 1.0)
        g.build()
        assert (g.mestimator_weights("reprojection")[0] < 1.0).any()
        b = _check_form(g, None, "n4 +huber")
        assert a != b
    finally:
        g.close()


# ---------------------------------------------------------------- 2. step primitive
@pytest.mark.parametrize("name", ["n7", "c64", "views"])
def test_step_primitive(name):
    r = SC.ref(name)
    p, s = r.p, dict(r.sys0)
    J = s["cost"]
    _, sd_scale, dx_sd, sdn = D.steepest_descent(s)
    dx_gn = r.dxs[0]
    gnn = float(np.linalg.norm(dx_gn))
    assert r.oks[0] and r.floors[0] <= SC.FLOOR_MAX and sdn < gnn
    bar = SC.dx_bar(r.floors[0])
    g = _solver(p)
    try:
        g.build()
        g.set_constant_conditioner(0.0)
        ok0, dx0 = g.solve()
        assert ok0
        types = []
        for delta in (0.0, 0.5 * sdn, 0.5 * (sdn + gnn), 2.0 * gnn):
            ref = D.select(delta, J, sd_scale, dx_sd, sdn, dx_gn, gnn)
            ok, dx, info = g.dogleg_step(delta)
            e = np.abs(dx - ref["dx"]).max() / np.abs(ref["dx"]).max()
            print(f"[{name}] delta {delta:.3e}: type {info['step_type']} ({ref['type']})  rel dx {e:.2e} (bar {bar:.1e})  "
                  f"{info}")
            assert ok and info["step_type"] == ref["type"]
            types.append(ref["type"])
            assert _rel(info["delta"], ref["delta"]) <= 1e-8
            assert _rel(info["sd_scale"], sd_scale) <= 1e-10 and _rel(info["dx_sd_norm"], sdn) <= 1e-10
            assert e <= bar
            if ref["type"] == SD:
                assert info["dx_gn_norm"] == 0.0  # not solved
                assert _rel(info["L0_over_J"], ref["L0"] / J) <= 1e-9
            else:
                assert _rel(info["dx_gn_norm"], gnn) <= bar
            if ref["type"] == DL:
                assert _rel(info["beta"], ref["beta"]) <= 1e-8
            if ref["type"] == GN:
                assert info["L0_over_J"] == 1.0
            # a query: the state is untouched
            assert np.array_equal(g.get_state(), p.state_init)
        assert set(types) == {SD, GN, DL}
        ok1, dx1 = g.solve()
        assert ok1 and np.array_equal(dx0, dx1)
    finally:
        g.close()


# ---------------------------------------------------------------- 3. runs
def _run(g, p, delta_init):
    g.set_state(p.state_init)
    return g.optimize(policy="dogleg", delta_init=delta_init, **D.OPT)


@pytest.mark.parametrize("name,delta_init", D.RUNS)
def test_run(name, delta_init):
    ref = D.reference(name, delta_init)
    p = SC.problem(name)
    g = capi.SplineSolver(p)
    try:
        res = _run(g, p, delta_init)
        st = g.get_state()
    finally:
        g.close()
    tr, dt = res["trace"], res["dogleg_trace"]
    dJ, dS = _rel(res["J_final"], ref["J_final"]), np.abs(st - ref["state"]).max()
    print(f"[{name} {delta_init}] {_steps(dt)} {_accepts(tr)} ({ref['steps']} {ref['accepted']})  J rel {dJ:.2e}  "
          f"state {dS:.2e}  bar {ref['bar']:.1e} (floor {ref['floor']:.2e})")
    assert _steps(dt) == ref["steps"] and _accepts(tr) == ref["accepted"]
    assert res["iterations"] == ref["iterations"] and res["failed_iterations"] == ref["failed_iterations"]
    assert res["linear_solver_failure"] == 0 and len(tr) == len(dt) == len(ref["passes"]) == res["passes"]
    # The per-pass bar, as test_gpu_spline_shapes.py derives a pass's: a pass leaves the device's state within
    # dx_bar x max(max|dx|, 1) of the oracle's, and delta, |dx_sd| and |dx_gn| of the next pass are lengths in that
    # state space (beta a ratio of them), so each is held to |got - ref| <= bar x max(|ref|, 1) with bar the largest
    # dx_bar over the systems the run solved.  (Near convergence g is a difference of large terms: the relative error
    # of |dx_sd| there exceeds the bar while its absolute error is far below the state's own.)
    worst, worst_rel = dict(delta=0.0, sdn=0.0, gnn=0.0, beta=0.0), dict(delta=0.0, sdn=0.0, gnn=0.0, beta=0.0)
    for k, q in enumerate(ref["passes"]):
        assert tr[k, 1] == dt[k, 0]  # kb_sp_get_trace's lambda column carries delta
        cmp = [("delta", dt[k, 0], q["delta"]), ("sdn", dt[k, 4], q["sdn"]), ("gnn", dt[k, 5], q["gnn"])]
        if q["type"] == DL:
            cmp.append(("beta", dt[k, 2], q["beta"]))
        for what, got, want in cmp:
            worst[what] = max(worst[what], abs(got - want) / max(abs(want), 1.0))
            if want != 0.0:
                worst_rel[what] = max(worst_rel[what], _rel(got, want))
        print(f"[{name} {delta_init}] pass {k}: " + "  ".join(f"{w} {got:.6e} ({_rel(got, want):.1e})"
                                                              for w, got, want in cmp if want != 0.0))
    print(f"[{name} {delta_init}] worst per-pass error over max(|ref|, 1): "
          + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()) + "   relative: "
          + "  ".join(f"{k} {v:.2e}" for k, v in worst_rel.items()))
    assert max(worst.values()) <= ref["bar"], worst
    assert dJ <= 1e-9
    assert dS <= 1e-6
    # a pass after a rejected step runs on the held system: |dx_sd| stays bitwise, and so does |dx_gn| unless this is
    # the pass that first needs the GN step; delta halves exactly where the restatement's does
    reused = 0
    for k, q in enumerate(ref["passes"]):
        if q["built"]:
            continue
        reused += 1
        qp = ref["passes"][k - 1]
        assert dt[k, 4] == dt[k - 1, 4]
        assert q["solved"] or dt[k, 5] == dt[k - 1, 5]
        assert (dt[k, 0] == dt[k - 1, 0] / 2.0) == (q["delta"] == qp["delta"] / 2.0)
        assert (dt[k, 0] == dt[k - 1, 0]) == (q["delta"] == qp["delta"])
    if (name, delta_init) == ("n4", 0.0):
        # passes 2 .. 24 are rejected; 3 .. 24 run on the system and the GN step of pass 2.  (The radius stays where it
        # is over them: get_dJ() compares the rejected cost with the cost before the last accepted step, so rho > 0.75.)
        assert reused == 22 and dt[2, 5] > 0.0 and np.all(dt[3:, 5] == dt[2, 5])


# ---------------------------------------------------------------- 4. failed solve
def test_failed_solve():
    p = D.unobserved_tail(SC.problem("imu_none"))
    g = _solver(p)
    try:
        g.build()
        g.set_constant_conditioner(0.0)
        ok, _ = g.solve()
        assert not ok
        res = g.optimize(policy="dogleg", delta_init=0.0, eps_x=1e-3, eps_j=1.0, max_iterations=4)
        assert _steps(res["dogleg_trace"]) == "xxxx" and _accepts(res["trace"]) == "0000"
        assert res["iterations"] == 0 and res["failed_iterations"] == 4 and res["linear_solver_failure"] == 1
        assert np.array_equal(g.get_state(), p.state_init)
        g.build()
        ok, _, info = g.dogleg_step(0.0)
        assert not ok and info["step_type"] == -1
    finally:
        g.close()


# ---------------------------------------------------------------- 5. determinism and coexistence
def test_two_runs_are_bitwise_equal():
    p = SC.problem("n2c")
    out = []
    for _ in range(2):
        g = capi.SplineSolver(p)
        try:
            res = _run(g, p, 0.01)
            out.append((res, g.get_state()))
        finally:
            g.close()
    (a, sa), (b, sb) = out
    assert np.array_equal(a["trace"], b["trace"]) and np.array_equal(a["dogleg_trace"], b["dogleg_trace"])
    assert np.array_equal(sa, sb)


def test_other_policies_after_dogleg_on_the_same_handle():
    """LM, GN and the captured GN pass on a handle that ran dog-leg first are bitwise a fresh handle's, and so is the
    dog-leg run after them"""
    p = SC.problem("n7")
    g, f = capi.SplineSolver(p), capi.SplineSolver(p)
    try:
        first = _run(g, p, 0.01)
        for h in (g, f):
            h.set_state(p.state_init)
        for policy in ("lm", "gn"):
            out = []
            for h in (g, f):
                h.set_state(p.state_init)
                res = h.optimize(policy=policy, **SC.OPT)
                assert "dogleg_trace" not in res
                out.append((res["trace"], h.get_state(), res["iterations"], res["failed_iterations"]))
            assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
            assert out[0][2:] == out[1][2:]
        out = []
        for h in (g, f):
            h.set_state(p.state_init)
            h.run_gn(3)
            out.append(h.get_state())
        assert np.array_equal(out[0], out[1])
        again = _run(f, p, 0.01)
        assert np.array_equal(first["dogleg_trace"], again["dogleg_trace"]) and np.array_equal(first["trace"], again["trace"])
    finally:
        g.close()
        f.close()


# ---------------------------------------------------------------- 6. errors
def test_errors():
    p = SC.problem("n2c")
    g = _solver(p)
    try:
        with pytest.raises(capi.KbError, match="kb_sp_rhs_jtj_rhs: build first"):
            g.rhs_jtj_rhs()
        with pytest.raises(capi.KbError, match="kb_sp_dogleg_step: build first"):
            g.dogleg_step(1.0)
        g.build()
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(capi.KbError, match="kb_sp_dogleg_step: delta"):
                g.dogleg_step(bad)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(capi.KbError, match="kb_sp_set_dogleg_options: delta_init"):
                g.optimize(policy="dogleg", delta_init=bad, max_iterations=2)
        assert np.array_equal(g.get_state(), p.state_init)
        # the system a run leaves is not a built one
        g.optimize(policy="dogleg", max_iterations=2)
        with pytest.raises(capi.KbError, match="build first"):
            g.rhs_jtj_rhs()
    finally:
        g.close()
    L, v, ok, inf = capi.lib(), capi.C.c_double(), capi.C.c_int(), capi.DoglegInfo()
    for name, call in (("kb_sp_rhs_jtj_rhs", lambda: L.kb_sp_rhs_jtj_rhs(None, capi.C.byref(v))),
                       ("kb_sp_set_dogleg_options", lambda: L.kb_sp_set_dogleg_options(None, None)),
                       ("kb_sp_dogleg_step", lambda: L.kb_sp_dogleg_step(None, 1.0, None, capi.C.byref(inf),
                                                                         capi.C.byref(ok))),
                       ("kb_sp_get_dogleg_trace", lambda: L.kb_sp_get_dogleg_trace(None, None, 0))):
        assert call() < 0 and L.kb_last_error().decode().startswith(name + ": null")
