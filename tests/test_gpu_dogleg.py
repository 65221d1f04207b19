"""Dog-leg trust-region policy on the device (kb_optimize policy 2, kb_dogleg_step, kb_get_dogleg_trace) against the
restatement of the policy over the CPU oracle's primitives (tests/dogleg_ref.py; the oracle itself has no dog-leg).

Bounds: sd_scale and |dx_sd| rel 1e-10 (the project's bound for blocks and rhs); |dx_gn|, beta and dx rel 1e-8 of
max|dx| (the bound for the solve); J_final rel 1e-9, state abs 1e-6, delta and beta per pass rel 1e-8.  Every optimizer
case first asserts on the restatement's own run that no decision is marginal (dogleg_ref.assert_not_marginal), so an
equal step / accept sequence is a meaningful requirement.
"""
import dataclasses

import numpy as np
import pytest

from kalibr_amd import synth

from . import dogleg_ref as R

pytestmark = pytest.mark.gpu

SD, GN, DL = R.SD, R.GN, R.DL

PROBLEMS = {
    "c1_12": lambda: synth.make_config(1, n_frames=12),  # C = 8
    "c4_8": lambda: synth.make_config(4, n_frames=8, p_view=0.7),  # C = 106: the two-slot route and k_solve<0>
    "c6_small": lambda: synth.make_config(6, n_frames=40, p_view=0.8),  # C = 42, four camera models
    "c2_ragged": lambda: synth.make_config(2, n_frames=60, p_view=0.5, seed_offset=7),
    # frame counts that are no multiple of the 4 frames per block (the clamped tail)
    "c1_5": lambda: synth.make_config(1, n_frames=5),
    "c4_7": lambda: synth.make_config(4, n_frames=7, p_view=0.7),
}
_cache = {}


@pytest.fixture(scope="module")
def capi():
    from kalibr_amd import capi as K
    return K


def problem(name):
    if name not in _cache:
        _cache[name] = PROBLEMS[name]()
    return _cache[name]


_ref_cache = {}


def reference(oracle_mod, name, delta_init, eps_x, eps_j, max_it):
    """the restatement's run of a case, computed once and shared (read-only)"""
    key = (name, delta_init, eps_x, eps_j, max_it)
    if key not in _ref_cache:
        p = problem(name)
        r = R.run(oracle_mod.Oracle(p), p.state_init, delta_init, eps_x, eps_j, max_it)
        r["worst"] = R.assert_not_marginal(r)
        _ref_cache[key] = r
    return _ref_cache[key]


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# ---------------------------------------------------------------- 1. the step primitive
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_step_primitive(capi, oracle_mod, name):
    p = problem(name)
    o = oracle_mod.Oracle(p)
    A = o.arrow(p.state_init)
    J = o.cost(p.state_init)
    _, sd_scale, dx_sd, sdn = R.steepest_descent(A)
    ok_o, dx_gn = o.solve(A, 0.0)
    assert ok_o
    gnn = float(np.linalg.norm(dx_gn))
    assert sdn < gnn
    g = capi.Solver(p)
    g.set_state(p.state_init)
    g.build()
    deltas = [0.0, 0.5 * sdn, float(np.sqrt(sdn * gnn)), 2.0 * gnn]
    want_types = [DL, SD, DL, GN]
    for delta, wt in zip(deltas, want_types):
        ref = R.select(delta, J, sd_scale, dx_sd, sdn, dx_gn, gnn)
        assert ref["type"] == wt
        ok, dx, info = g.dogleg_step(delta)
        print(name, delta, info)
        assert ok and info["step_type"] == wt
        assert _rel(info["sd_scale"], sd_scale) <= 1e-10 and _rel(info["dx_sd_norm"], sdn) <= 1e-10
        assert _rel(info["delta"], ref["delta"]) <= 1e-8
        scale = np.abs(ref["dx"]).max()
        assert np.abs(dx - ref["dx"]).max() <= 1e-8 * scale
        if wt == SD:
            assert info["dx_gn_norm"] == 0.0  # not solved
            assert _rel(info["L0_over_J"], ref["L0"] / J) <= 1e-9
        else:
            assert _rel(info["dx_gn_norm"], gnn) <= 1e-8
        if wt == DL:
            assert _rel(info["beta"], ref["beta"]) <= 1e-8
            assert _rel(info["L0_over_J"], ref["beta"] * (2 - ref["beta"])) <= 1e-8
            if delta == 0.0:
                assert abs(info["beta"] - 0.5) <= 1e-9
        if wt == GN:
            assert info["L0_over_J"] == 1.0
        if wt in (SD, DL):
            assert _rel(float(np.linalg.norm(dx)), info["delta"]) <= 1e-10
        # a query: the state is untouched and a following solve still returns the GN step
        assert np.array_equal(g.get_state(), p.state_init)
    ok, dx = g.solve()
    assert ok and np.abs(dx - dx_gn).max() <= 1e-8 * np.abs(dx_gn).max()
    g.close()


def test_step_needs_a_built_system(capi):
    p = problem("c1_12")
    g = capi.Solver(p)
    g.set_state(p.state_init)
    with pytest.raises(capi.KbError, match="kb_build"):
        g.dogleg_step(1.0)
    g.build()
    g.optimize(policy="gn", max_iterations=1)
    with pytest.raises(capi.KbError, match="kb_build"):
        g.dogleg_step(1.0)
    g.close()


# ---------------------------------------------------------------- 2 - 4. the device-resident loop
def check_run(capi, oracle_mod, name, delta_init, eps_x, eps_j, max_it, steps, accepted=None):
    ref = reference(oracle_mod, name, delta_init, eps_x, eps_j, max_it)
    assert ref["steps"] == steps, ref["steps"]  # the restatement's sequence is pinned
    if accepted is not None:
        assert ref["accepted"] == accepted
    p = problem(name)
    g = capi.Solver(p)
    g.set_state(p.state_init)
    res = g.optimize(policy="dogleg", delta_init=delta_init, eps_x=eps_x, eps_j=eps_j, max_iterations=max_it)
    tr, dt = res["trace"], res["dogleg_trace"]
    got_steps = "".join(R.STEP[int(t)] if t >= 0 else "x" for t in dt[:, 1])
    got_acc = "".join(str(int(a)) for a in tr[:, 3])
    print(name, delta_init, got_steps, got_acc, res["J_final"], ref["J_final"], ref["worst"])
    assert got_steps == steps and got_acc == ref["accepted"]
    assert res["iterations"] == ref["iterations"] and res["failed_iterations"] == ref["failed_iterations"]
    assert res["linear_solver_failure"] == 0 and len(tr) == len(dt) == len(ref["passes"])
    assert _rel(res["J_final"], ref["J_final"]) <= 1e-9
    assert np.abs(g.get_state() - ref["state"]).max() <= 1e-6
    for k, q in enumerate(ref["passes"]):
        assert _rel(dt[k, 0], q["delta"]) <= 1e-8, (k, dt[k, 0], q["delta"])
        assert tr[k, 1] == dt[k, 0]  # kb_get_trace's lambda column carries delta
        if q["type"] == DL:
            assert _rel(dt[k, 2], q["beta"]) <= 1e-8, (k, dt[k, 2], q["beta"])
        assert _rel(tr[k, 0], q["J"]) <= 1e-9
    g.close()
    return res, ref


@pytest.mark.parametrize("name", ["c1_12", "c4_8", "c6_small"])
def test_default_policy_parity(capi, oracle_mod, name):
    """delta_init = 0, the reference behaviour: D G G G; c6_small's last pass is rejected (the revert)"""
    res, ref = check_run(capi, oracle_mod, name, 0.0, 1e-3, 1.0, 25, "DGGG")
    if name == "c6_small":
        assert ref["accepted"] == "1110" and res["failed_iterations"] == 1


@pytest.mark.parametrize("name,max_it,steps", [("c1_12", 25, "SSSSDDDDDGGG"), ("c4_8", 13, "SSSDDDDDDDGGG"),
                                               ("c2_ragged", 12, "SSSDDDDDDDGG")])
def test_all_three_branches(capi, oracle_mod, name, max_it, steps):
    check_run(capi, oracle_mod, name, 1e-3, 1e-9, 1e-3, max_it, steps)


def test_reuse_after_rejection(capi, oracle_mod):
    """the four rejected passes neither rebuild nor re-solve: |dx_gn| and |dx_sd| stay bitwise constant over them
    while delta halves"""
    res, _ = check_run(capi, oracle_mod, "c6_small", 1e-3, 1e-9, 1e-3, 16, "SSSDDDDDDDGGGGGG", "1111111111110000")
    assert res["failed_iterations"] == 4
    dt = res["dogleg_trace"]
    # pass 11 is the last accepted one; passes 12 .. 15 are rejected, 13 .. 15 run on the system of pass 12
    for k in (13, 14, 15):
        assert dt[k, 4] == dt[12, 4] and dt[k, 5] == dt[12, 5] and dt[k, 5] > 0.0
        assert dt[k, 0] == dt[k - 1, 0] / 2.0


# ---------------------------------------------------------------- 6. failed solve
def _truncate_view(p, v, keep):
    """problem with view v cut to its first `keep` corners (as tests/test_gpu_edge_cases.py)"""
    o = p.view_offset
    idx = np.concatenate([np.arange(o[u], o[u + 1] if u != v else o[u] + keep) for u in range(p.n_views)])
    counts = np.array([(o[u + 1] - o[u]) if u != v else keep for u in range(p.n_views)])
    return dataclasses.replace(p, corner_id=p.corner_id[idx].astype(np.int32), y=p.y[idx].copy(),
                               view_offset=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))


def test_failed_solve(capi, oracle_mod):
    """a frame without a seen corner: the GN solve the first pass needs fails, is retried on every pass (each a failed
    iteration) and no step is applied"""
    p = _truncate_view(synth.make_config(1, n_frames=6), 3, 0)
    ref = R.run(oracle_mod.Oracle(p), p.state_init, 0.0, 1e-3, 1.0, 5)
    assert ref["steps"] == "xxxxx" and ref["failed_iterations"] == 5 and ref["iterations"] == 0
    g = capi.Solver(p)
    g.set_state(p.state_init)
    res = g.optimize(policy="dogleg", delta_init=0.0, max_iterations=5)  # returns 0 (no KbError)
    assert res["linear_solver_failure"] == 1 and res["failed_iterations"] == 5 and res["iterations"] == 0
    assert np.array_equal(g.get_state(), p.state_init)
    assert list(res["dogleg_trace"][:, 1]) == [-1.0] * 5
    g.build()
    ok, _, _ = g.dogleg_step(0.0)
    assert not ok
    g.close()


# ---------------------------------------------------------------- 7. mechanics
def test_graph_and_determinism(capi):
    p = problem("c6_small")
    runs = []
    for use_graph in (True, False, True):
        g = capi.Solver(p)
        g.set_state(p.state_init)
        res = g.optimize(policy="dogleg", delta_init=1e-3, eps_x=1e-9, eps_j=1e-3, max_iterations=16,
                         use_graph=use_graph)
        assert res["graphed"] == int(use_graph)
        runs.append((res, g.get_state()))
        g.close()
    for res, st in runs[1:]:
        assert np.array_equal(res["trace"], runs[0][0]["trace"])
        assert np.array_equal(res["dogleg_trace"], runs[0][0]["dogleg_trace"])
        assert np.array_equal(st, runs[0][1])


def test_lm_after_dogleg_on_the_same_handle(capi):
    p = problem("c1_12")
    g = capi.Solver(p)
    g.set_state(p.state_init)
    g.optimize(policy="dogleg", delta_init=1e-3, eps_x=1e-9, eps_j=1e-3, max_iterations=25)
    g.set_state(p.state_init)
    a = g.optimize(policy="lm", max_iterations=20)
    sa = g.get_state()
    f = capi.Solver(p)
    f.set_state(p.state_init)
    b = f.optimize(policy="lm", max_iterations=20)
    assert np.array_equal(a["trace"], b["trace"]) and np.array_equal(sa, f.get_state())
    # and the dog-leg again after LM, on the same handle, repeats itself
    g.set_state(p.state_init)
    c = g.optimize(policy="dogleg", delta_init=1e-3, eps_x=1e-9, eps_j=1e-3, max_iterations=25)
    f.set_state(p.state_init)
    d = f.optimize(policy="dogleg", delta_init=1e-3, eps_x=1e-9, eps_j=1e-3, max_iterations=25)
    assert np.array_equal(c["dogleg_trace"], d["dogleg_trace"]) and np.array_equal(g.get_state(), f.get_state())
    g.close()
    f.close()


def test_policy_errors(capi):
    p = problem("c1_12")
    subs = [p.frame_slice(0, 5), p.frame_slice(5, 12)]
    solvers = [capi.Solver(s) for s in subs]
    capi.comm_init_local(solvers)
    solvers[0].set_state(subs[0].state_init)
    with pytest.raises(capi.KbError, match="unsharded"):
        solvers[0].optimize(policy="dogleg", max_iterations=3)
    for s in solvers:
        s.close()
    g = capi.Solver(p)
    g.set_state(p.state_init)
    with pytest.raises(capi.KbError, match="unknown policy"):
        g.optimize(policy=3, max_iterations=3)
    with pytest.raises(capi.KbError, match="delta_init"):
        g.optimize(policy="dogleg", delta_init=-1.0, max_iterations=3)
    g.close()
