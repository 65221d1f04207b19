"""Preconditions of tests/test_gpu_spline_dogleg.py, from the oracle alone (CPU): the restatement's run of every
(case, delta_init) it uses is pinned here (step string, accept string) and shown to hold no marginal decision
(dogleg_ref.assert_not_marginal), so that an equal step / accept sequence is a meaningful requirement of the device;
the spline system's g^T H g from its blocks is checked against the dense term rows; and the failed-solve problem is
shown to fail in the oracle's own solver.

The pinned strings are what the restatement gave when the runs were chosen (eps_x = 1e-3, eps_j = 1.0, 25 iterations at
most); a change to synth or to the oracle that moves a run is caught here, not on the GPU.
"""
import numpy as np
import pytest

from kalibr_amd import synth
from oracle import oracle as O

from . import spline_cases as SC
from . import spline_dogleg_ref as D

# (steps, accepts) of D.RUNS, in order
PINNED = {
    ("n3", 0.01): ("SDDDDDDGGGG", "1" * 11),
    ("n33", 0.01): ("SSDDDDDDGGG", "1" * 11),
    ("c23", 0.01): ("SSDDDDDDGGGG", "1" * 12),
    ("c64", 0.01): ("SDDDDDDDGGG", "1" * 11),
    ("views", 0.01): ("SDDDDDDGGGG", "1" * 11),
    ("n17", 0.01): ("SDDDDDDDGGG", "1" * 11),
    ("n7", 0.0): ("DGGGG", "1" * 5),
    ("n2c", 0.0): ("DGGGGGG", "1" * 7),
    ("n4", 0.0): ("DG" + "G" * 23, "11" + "0" * 23),
    ("imu_dense", 0.01): ("SDDDDDDDGGGGGGGGGGGGGGGGG", "111111111" + "0" * 16),
    ("c44", 0.05): ("DDDDDDGG", "11111110"),
}
# the oracle's own band-against-dense difference at the systems a run solves: at state_init test_spline_cases.py holds
# it to SC.FLOOR_MAX = 1e-7; along a dog-leg run it reaches 8e-7 (n2c, n33), so the per-pass bars (100 x floor) stay
# below 1e-4 under this cap
RUN_FLOOR_MAX = 1e-6


@pytest.mark.parametrize("name,delta_init", D.RUNS)
def test_run_is_pinned_and_not_marginal(name, delta_init):
    assert delta_init == 0.0 or delta_init > D.OPT["eps_x"]
    r = D.reference(name, delta_init)  # asserts assert_not_marginal on its own run
    print(name, delta_init, r["steps"], r["accepted"], r["worst"], f"floor {r['floor']:.2e} bar {r['bar']:.1e}")
    assert (r["steps"], r["accepted"]) == PINNED[(name, delta_init)]
    assert r["linear_solver_failure"] == 0 and "x" not in r["steps"]
    assert r["iterations"] == len(r["steps"]) and r["failed_iterations"] == r["accepted"].count("0")
    assert r["floor"] <= RUN_FLOOR_MAX
    same, d_state, d_J = r["repro"]
    print(f"  band against dense solver: state {d_state:.1e}  J {d_J:.1e}")
    assert same and d_state <= D.REPRO_STATE_MAX and d_J <= D.REPRO_J_MAX
    # a pass after a rejected step keeps the system, every other pass builds; a system is solved at most once
    solves = 0
    for k, p in enumerate(r["passes"]):
        assert p["built"] == (k == 0 or r["passes"][k - 1]["accepted"] == 1)
        solves = int(p["solved"]) + (0 if p["built"] else solves)
        assert solves <= 1


@pytest.mark.parametrize("name,delta_init", D.NOT_REPRODUCIBLE)
def test_a_run_left_out_cannot_referee_its_bars(name, delta_init):
    """the listed run that is not taken: the oracle's band and dense solvers end further apart than the bars on the
    device's J_final and state"""
    same, d_state, d_J = D.reproducibility(name, delta_init)
    print(name, delta_init, same, f"state {d_state:.1e}  J {d_J:.1e}")
    assert (name, delta_init) not in D.RUNS
    assert d_state > D.REPRO_STATE_MAX and d_J > D.REPRO_J_MAX


def test_runs_cover_the_policy_and_the_shapes():
    assert set(PINNED) == set(D.RUNS) and len(D.RUNS) == len(PINNED)
    steps = "".join(v[0] for v in PINNED.values())
    assert {"S", "D", "G"} <= set(steps)
    # a rejected step followed by a pass that does not rebuild
    assert any("0" in acc[:-1] for _, acc in PINNED.values())
    cases = [SC.BY_NAME[n] for n, _ in D.RUNS]
    assert {c.kmod3 for c in cases} == {0, 1, 2}
    assert any(c.n == 2 for c in cases) and {23, 64} <= {c.C for c in cases}


def test_g_h_g_against_dense_rows():
    """g^T H g from (Hcc, Hsc, Hband) equals |J g|^2 over the dense reprojection and IMU rows"""
    p = synth.make_spline_config(n_frames=16)
    o = O.SplineOracle(p)
    st = p.state_init
    rows = [o.reproj_dense(st, v, k)[1] for v in range(p.n_views)
            for k in range(p.view_offset[v + 1] - p.view_offset[v])]
    rows += [o.imu_dense(st, m)[1] for m in range(p.n_imu)]
    J = np.vstack(rows)
    s = D.Adapter(o).system(st)
    g = s["rhs"]
    want = float(np.sum((J @ g) ** 2))
    got = D.g_h_g(s)
    print(got, want, abs(got - want) / want)
    assert abs(got - want) <= 1e-10 * want
    _, sd_scale, dx_sd, sdn = D.steepest_descent(s)
    assert abs(sd_scale - (g @ g) / want) <= 1e-10 * sd_scale and abs(sdn - sd_scale * np.linalg.norm(g)) <= 1e-12 * sdn


def test_unobserved_tail_fails_the_oracles_solve():
    """imu_none without the views of its last 10 frames: the last coefficients carry no term, the oracle's solve at
    lambda = 0 reports failure, and the restatement's run is failed iterations only"""
    p = D.unobserved_tail(SC.problem("imu_none"))
    o = O.SplineOracle(p)
    s = o.system(p.state_init)
    assert not np.any(s["Hband"][-1]) and not np.any(s["gs"][-6:]) and not np.any(s["Hsc"][-6:])
    ok, _ = o.solve(s, 0.0)
    assert not ok
    r = D.run(D.Adapter(o), p.state_init, 0.0, max_iterations=4)
    assert r["steps"] == "xxxx" and r["iterations"] == 0 and r["failed_iterations"] == 4
    assert r["linear_solver_failure"] == 1 and np.array_equal(r["state"], p.state_init)
