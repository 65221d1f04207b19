"""The preconditions of the spline shape sweep (tests/spline_cases.py), from the oracle alone: every case sits on the
edge it was made for, and at every (state, lambda) the GPU module solves, the oracle's two solvers (band Cholesky and
dense) succeed and agree to FLOOR_MAX -- so a dx bar derived from that floor never exceeds 1e-5, and a case the
reference itself cannot solve is a failure here, never a skip there."""
import numpy as np
import pytest

from kalibr_amd import synth
from oracle import oracle as O

from . import spline_cases as SC


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_reaches_its_edge(name):
    c, p = SC.BY_NAME[name], SC.problem(name)
    K = p.n_coeffs
    assert ((K + 2) // 3, K % 3, p.cam_cols) == (c.n, c.kmod3, c.C)
    assert K >= 4 and p.n_views > 0 and p.n_corners > 0
    # what the device's upload requires: views sorted by frame, one per (frame, camera), offsets monotone
    assert np.all(np.diff(p.view_frame) >= 0) and np.all(np.diff(p.view_offset) > 0)
    assert len(set(zip(p.view_frame.tolist(), p.view_cam.tolist()))) == p.n_views
    assert p.view_offset[0] == 0 and p.view_offset[-1] == p.n_corners == p.y.shape[0]
    t_min, t_max = p.knots[p.order - 1], p.knots[p.knots.size - p.order]
    assert t_min <= p.frame_time[0] and p.frame_time[-1] <= t_max
    assert p.n_imu == 0 or (t_min <= p.imu_time[0] and p.imu_time[-1] <= t_max)


def test_table_covers_the_edges():
    assert {c.kmod3 for c in SC.CASES} == {0, 1, 2}
    assert {2, 3, 4, 16, 17, 32, 33, 35, 64, 65} <= {c.n for c in SC.CASES}
    # both padded-slot counts of the last node (K % 3 = 1: two identity rows, K % 3 = 2: one) at the smallest n too
    assert {c.kmod3 for c in SC.CASES if c.n == 2} == {0, 1, 2}
    Cs = {c.C for c in SC.CASES}
    for lo, hi in ((16, 32), (32, 40), (40, 48), (48, 64)):  # one k_sp_camsolve<CM> each
        assert any(lo < C <= hi for C in Cs), (lo, hi)
    assert 48 in Cs and 64 in Cs
    assert any(set(c.models) != {SC.RT} for c in SC.CASES)  # the all-models build and cost kernels
    assert {m for c in SC.CASES for m in c.models} == set(synth.NINTR)  # all seven camera models
    # a frame or an IMU sample exactly at t_max (the t == tmax branch of the device side's basis_weights)
    p = SC.problem("c64")
    assert p.frame_time[-1] == p.knots[p.knots.size - p.order] == p.imu_time[-1]
    # the GN-pass checks with and without a motion error run at a power of two and next to one
    assert {c.n for c in SC.CASES if c.motion} == {4, 33}
    assert all(c.gn for c in SC.CASES if c.motion)


@pytest.mark.parametrize("name", SC.NAMES)
def test_oracle_floor_and_runs(name):
    """floor(s, lambda) = max|dx_band - dx_dense| / max|dx_dense| <= FLOOR_MAX, both solves ok, at lambda = 10 at
    state_init and (GN cases) at lambda = 0 along the oracle's GN states s_0, s_1, s_2; the GN / LM runs the GPU
    module compares against have no failed iteration, and the LM run is reproducible under another summation order"""
    c, r = SC.BY_NAME[name], SC.ref(name)
    print(f"{name}: floor(lambda=10) {r.floor10:.2e}; floor(lambda=0) at s0, s1, s2: "
          + ", ".join(f"{f:.2e}" for f in r.floors))
    assert r.ok10 and r.floor10 <= SC.FLOOR_MAX
    assert np.isfinite(r.sys0["cost"]) and r.sys0["cost"] > 0.0
    if c.gn:
        assert len(r.floors) == SC.Ref.N_STEPS and all(r.oks)
        assert max(r.floors) <= SC.FLOOR_MAX, r.floors
        st, res = r.optimize("gn")
        assert res["failed_iterations"] == 0 and not res["linear_solver_failure"]
        assert 0 < res["iterations"] <= SC.OPT["max_iterations"]
        # the pass-by-pass trajectory is the run's: the same first three costs
        for k in range(min(3, res["iterations"])):
            Jk = r.o.cost(r.states[k + 1])
            assert abs(Jk - res["trace"][k, 0]) <= 1e-9 * Jk
    if c.lm:
        st, res = r.optimize("lm")
        assert res["failed_iterations"] == 0 and not res["linear_solver_failure"]
        st1, res1 = r.o.optimize(r.p.state_init, policy="lm", nthreads=1, **SC.OPT)
        print(f"{name}: LM {res['iterations']} it; 1 thread against 4: max|state difference| "
              f"{np.abs(st1 - st).max():.1e}")
        assert res1["iterations"] == res["iterations"] and res1["failed_iterations"] == 0
        assert np.abs(st1 - st).max() <= SC.LM_REPRO_MAX


@pytest.mark.parametrize("name", [c.name for c in SC.CASES if c.motion])
def test_oracle_floor_with_motion_error(name):
    r = SC.ref(name, motion=True)
    assert r.ok10 and r.floor10 <= SC.FLOOR_MAX
    assert r.oks == [True] and r.floors[0] <= SC.FLOOR_MAX


# ---- the surgery ----
def _base():
    return synth.make_spline_problem([SC.RT, SC.RT], 31, 12, knots_per_second=10.0)


def _same_but(p, q, changed):
    import dataclasses
    for f in dataclasses.fields(p):
        if f.name in changed or f.name in ("meta", "name"):
            continue
        a, b = getattr(p, f.name), getattr(q, f.name)
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, f.name


VIEW_FIELDS = {"view_frame", "view_cam", "view_offset", "corner_id", "y"}


def test_drop_round_trip():
    p = _base()
    assert p.n_views == 62 and np.all(np.diff(p.view_offset) >= 66)  # every view present, each with > 65 corners
    q = SC.drop(p, lambda f, c: True)
    _same_but(p, q, set())
    q = SC._views(p)
    _same_but(p, q, VIEW_FIELDS)
    views = {(int(f), int(c)): int(b - a) for f, c, a, b in
             zip(q.view_frame, q.view_cam, q.view_offset[:-1], q.view_offset[1:])}
    gone = {(0, 0), (0, 1), (7, 0), (7, 1), (30, 0)} | {(f, 1) for f in range(31) if f % 3 == 1}
    assert set(views) == {(f, c) for f in range(31) for c in range(2)} - gone
    assert views[(3, 0)] == 1 and views[(5, 1)] == 65
    full = {(int(f), int(c)): int(b - a) for f, c, a, b in
            zip(p.view_frame, p.view_cam, p.view_offset[:-1], p.view_offset[1:])}
    assert all(n == full[k] for k, n in views.items() if k not in ((3, 0), (5, 1)))
    assert q.n_corners == sum(views.values()) == q.y.shape[0] == q.corner_id.size
    assert np.all(np.diff(q.view_offset) > 0) and np.all(np.diff(q.view_frame) >= 0)
    # the kept corners are the original ones, in order
    v = list(zip(q.view_frame.tolist(), q.view_cam.tolist())).index((5, 1))
    v0 = list(zip(p.view_frame.tolist(), p.view_cam.tolist())).index((5, 1))
    assert np.array_equal(q.y[q.view_offset[v]: q.view_offset[v + 1]], p.y[p.view_offset[v0]: p.view_offset[v0] + 65])
    # a view whose corners all go disappears
    q1 = SC.drop(p, lambda f, c: True, lambda f, c, j: (f, c) != (2, 1))
    assert q1.n_views == p.n_views - 1 and (2, 1) not in set(zip(q1.view_frame.tolist(), q1.view_cam.tolist()))
    for s in (q, q1):
        assert np.isfinite(O.SplineOracle(s).cost(s.state_init))


def test_without_imu_round_trip():
    p = _base()
    q = SC.without_imu(p)
    _same_but(p, q, {"imu_time", "imu_gyro", "imu_acc"})
    assert q.n_imu == 0 and q.imu_gyro.shape == (0, 3) and q.imu_acc.shape == (0, 3)
    J, J0 = O.SplineOracle(q).cost(q.state_init), O.SplineOracle(p).cost(p.state_init)
    assert np.isfinite(J) and 0.0 < J < J0


def test_jitter_knots_round_trip():
    p = _base()
    q = SC.jitter_knots(p, 5)
    _same_but(p, q, {"knots"})
    o, kn, k0 = p.order, q.knots, p.knots
    h = k0[o] - k0[o - 1]
    assert kn.size == k0.size and np.all(np.diff(kn) > 0.39 * h)
    assert np.array_equal(kn[:o], k0[:o]) and np.array_equal(kn[-o:], k0[-o:])  # t_min, t_max and outside them
    moved = np.abs(kn[o:-o] - k0[o:-o])
    assert np.all(moved <= 0.3 * h * (1 + 1e-12)) and np.all(moved > 0.0) and moved.max() > 0.15 * h
    assert not np.array_equal(SC.jitter_knots(p, 6).knots, kn)
    assert np.isfinite(O.SplineOracle(q).cost(q.state_init))
