"""The preconditions of the one-model rig sweep (tests/model_set_cases.py), from synth and the oracle alone: every rig
synthesises with the camera-block width its row records, the oracle's blocks are finite at both states and its Schur
and dense solves at lambda = 10 agree, the rigs admitted to the three-pass Gauss-Newton comparison are exactly those on
which the oracle's own passes succeed and do not depend on its summation order, and the crafted states have the
geometry they are there for -- so a rig the reference cannot referee is a failure here, never a skip on the GPU."""
import numpy as np
import pytest

from kalibr_amd import synth
from oracle import oracle as O

from . import model_set_cases as MC


def test_table_covers_the_instantiations():
    assert len(MC.SMALL) == 18 and len(MC.PIPED) == 12 and len(MC.X4) == 6 and len(MC.LARGE) == 6
    assert {MC.RIGS[n].model for n in MC.SMALL} == set(MC.MODELS) == set(synth.NINTR) - {synth.PINHOLE_RADTAN}
    by_n = lambda sel: tuple(sorted(MC.RIGS[n].C for n in MC.SMALL if sel(MC.RIGS[n].n)))  # noqa: E731
    assert by_n(lambda n: n == 1) == MC.C_X1
    assert by_n(lambda n: n == 4) == MC.C_X4
    assert by_n(lambda n: n >= 7) == MC.C_X8
    # k_build on one camera, k_buildp from four; non-expanded partials up to C = 64, expanded above
    assert all(MC.RIGS[n].kernel == ("k_build" if MC.RIGS[n].n == 1 else "k_buildp") for n in MC.RIGS)
    assert all(MC.RIGS[n].C <= 64 for n in MC.X4) and all(64 < MC.RIGS[n].C <= 111 for n in MC.PIPED if n not in MC.X4)
    # the large rigs: one of each intrinsic count 5, 6, 9 at either block width, two frames per block, a short last one
    assert sorted(synth.NINTR[MC.RIGS[n].model] for n in MC.LARGE) == [5, 5, 6, 6, 9, 9]
    for n in MC.LARGE:
        r = MC.RIGS[n]
        bpc = 2 if r.n == 4 else 1
        gf = (r.n_frames + 256 * bpc - 1) // (256 * bpc)
        assert gf == r.gframes == 2 and r.n_frames % gf == 1
    # the Gauss-Newton list: every rig is either admitted or left out with a reason, and the 10 x4 / x8 rigs of the
    # five models on which undamped GN is defined are admitted
    assert set(MC.GN_ADMITTED) | set(MC.GN_LEFT_OUT) == set(MC.RIGS)
    assert not set(MC.GN_ADMITTED) & set(MC.GN_LEFT_OUT) and len(set(MC.GN_ADMITTED)) == len(MC.GN_ADMITTED)
    assert {n for n in MC.PIPED if MC.RIGS[n].model != MC.OR} <= set(MC.GN_ADMITTED)
    assert all(MC.RIGS[n].model != MC.OR for n in MC.GN_ADMITTED)


def _dense_H(A, lam):
    C, F = A["Hcc"].shape[0], A["Hff"].shape[0]
    H = np.zeros((C + 6 * F, C + 6 * F))
    H[:C, :C] = A["Hcc"]
    for f in range(F):
        o = C + 6 * f
        H[o:o + 6, o:o + 6] = A["Hff"][f]
        H[o:o + 6, :C] = A["Hfc"][f]
        H[:C, o:o + 6] = A["Hfc"][f].T
    return H + lam * lam * np.eye(C + 6 * F)


@pytest.mark.parametrize("name", list(MC.RIGS))
def test_rig_synthesises_and_the_oracle_solves_it(name):
    r, p = MC.RIGS[name], MC.problem(name)
    assert (p.n_cams, p.n_frames, p.cam_cols) == (r.n, r.n_frames, r.C)
    assert set(p.cam_model.tolist()) == {r.model}
    assert p.n_views > 0 and np.all(np.diff(p.view_offset) > 0) and np.all(np.diff(p.view_frame) >= 0)
    if r.n > 1:  # p_view < 1: absent views
        assert p.n_views < r.n * r.n_frames
    R = MC.ref(name)
    for which in ("init", "truth"):
        A = R.arrow(which)
        assert all(np.isfinite(A[k]).all() for k in ("Hff", "Hfc", "gf", "Hcc", "gc", "rhs")), which
        assert np.isfinite(A["cost"]) and A["cost"] > 0.0
        ok, dx = R.solve(which)
        if p.total_cols > 800:  # the oracle's dense solve is an unblocked Cholesky: LAPACK's on the same matrix
            ok_d, dx_d = True, np.linalg.solve(_dense_H(A, 10.0), A["rhs"])
        else:
            ok_d, dx_d = R.solve(which, dense=True)
        floor = MC.rel(dx, dx_d)
        print(f"{name} {which}: oracle Schur against dense at lambda = 10: {floor:.1e}")
        assert ok and ok_d and floor <= MC.FLOOR_MAX


@pytest.mark.parametrize("name", list(MC.RIGS))
def test_gauss_newton_admission(name):
    """admitted <=> the oracle's three undamped passes succeed and its 1-thread and 8-thread runs agree to
    GN_SPREAD_MAX in every state entry"""
    R = MC.ref(name)
    (s8, r8), (s1, r1) = R.gn(8), R.gn(1)
    runs_ok = all(r["iterations"] == 3 and r["failed_iterations"] == 0 and not r["linear_solver_failure"]
                  for r in (r1, r8)) and np.isfinite(s1).all() and np.isfinite(s8).all()
    spread = float(np.abs(s1 - s8).max()) if runs_ok else float("inf")
    print(f"{name}: oracle's three GN passes ok {runs_ok}, 1 thread against 8: {spread:.1e}")
    assert (runs_ok and spread <= MC.GN_SPREAD_MAX) == (name in MC.GN_ADMITTED)
    if MC.RIGS[name].model == MC.OR:
        assert not runs_ok  # undamped GN is not defined on omni-radtan rigs: failed iterations, not a spread


# ---- the crafted states ----
@pytest.mark.parametrize("name", list(MC.EDGE_RIGS))
def test_edge_state_geometry(name):
    p, st = MC.edge_problem(name), MC.edge_state(name)
    want_r2 = (5e-6, 2.5e-5, 5e-18, 2e-12)
    for cam, f0 in MC.EDGE_RIGS[name]:
        assert int(p.cam_model[cam]) in (MC.EQ, MC.FV)
        for k, (ex, ey) in enumerate(MC.EDGE_POINTS):
            P = MC.first_corner(p, f0 + k, cam)
            x, y, z = MC.normalised(p, st, f0 + k, cam, P)
            z0 = MC.normalised(p, p.state_init, f0 + k, cam, P)[2]
            assert abs(x - ex) <= 1e-12 * abs(ex) + 1e-15 and abs(y - ey) <= 1e-12 * abs(ey) + 1e-15
            assert abs(z - z0) <= 1e-12 * z0 and z > 0.3
            r2 = x * x + y * y
            assert abs(r2 - want_r2[k]) <= 1e-6 * want_r2[k]
            # a factor 2 from either threshold (5e-6 sits on the factor itself)
            assert not (0.5e-5 * (1 + 1e-6) < r2 < 2e-5) and not (0.5e-8 < np.sqrt(r2) < 2e-8)
    # only the translations of the crafted frames moved
    moved = np.nonzero(st != p.state_init)[0]
    allowed = {MC._frame_offset(p, f0 + k) + 4 + i for _, f0 in MC.EDGE_RIGS[name] for k in range(4) for i in range(3)}
    assert set(moved.tolist()) <= allowed and moved.size >= 3 * 4 * len(MC.EDGE_RIGS[name]) - 2
    A = O.Oracle(p).arrow(st)
    assert all(np.isfinite(A[k]).all() for k in ("Hff", "Hfc", "gf", "Hcc", "gc", "rhs")) and np.isfinite(A["cost"])


@pytest.mark.parametrize("name", [n for n in MC.EDGE_RIGS if n != "equi x4"])
def test_edge_state_reaches_fovs_small_radius_branch_in_the_oracle(name):
    """inside the limit the w column of the crafted term is the same constant (w - sin w) / (w^2 cos^2(w / 2)) in both
    rows, times fu and fv (the reference's quirk); outside it the rows are u ds and v ds"""
    p, st = MC.edge_problem(name), MC.edge_state(name)
    o = O.Oracle(p)
    cam, f0 = [(c, f) for c, f in MC.EDGE_RIGS[name] if int(p.cam_model[c]) == MC.FV][0]
    fu, fv, w = st[cam * synth.MAX_INTR], st[cam * synth.MAX_INTR + 1], st[cam * synth.MAX_INTR + 4]
    col = MC.w_column(p, cam)
    const = (w - np.sin(w)) / (w * w * np.cos(0.5 * w) ** 2)
    for k, inside in ((0, True), (1, False)):
        v = int(np.nonzero((p.view_frame == f0 + k) & (p.view_cam == cam))[0][0])
        _, _, J = o.term_dense(st, v, 0)
        ju, jv = -J[0, col] / fu, -J[1, col] / fv  # the term is e = y - projection
        if inside:
            assert abs(ju - const) <= 1e-14 * const and abs(jv - const) <= 1e-14 * const
        else:
            ex, ey = MC.EDGE_POINTS[k]
            assert abs(ju / jv - ex / ey) <= 1e-9 and abs(ju) < 0.1 * const


@pytest.mark.parametrize("name", list(MC.SMALL_W))
def test_small_w_states(name):
    p = MC.edge_problem(name)
    states = MC.small_w_states(name)
    assert sorted(w * w for _, ws in states for w in ws.values()) == pytest.approx([1e-6, 9e-6], rel=1e-12)
    for st, ws in states:
        assert all(w * w < 1e-5 for w in ws.values())
        A = O.Oracle(p).arrow(st)
        assert all(np.isfinite(A[k]).all() for k in ("Hff", "Hfc", "gf", "Hcc", "gc", "rhs"))
        for cam in ws:
            c = MC.w_column(p, cam)
            assert not A["Hcc"][c].any() and not A["Hcc"][:, c].any() and not A["Hfc"][:, :, c].any()
            assert A["gc"][c] == 0.0
        # the other cameras' w columns are live
        for cam in range(p.n_cams):
            if int(p.cam_model[cam]) == MC.FV and cam not in ws:
                assert A["Hcc"][MC.w_column(p, cam), MC.w_column(p, cam)] > 0.0


def test_pose_steps_straddle_the_series_threshold():
    p = MC.edge_problem("fov x4")
    dx = MC.pose_steps(p)
    C = p.cam_cols
    th = [float(np.linalg.norm(dx[C + 6 * k: C + 6 * k + 3])) for k in range(8)]
    assert th[0] == th[4] == 0.0
    for k in range(8):
        assert abs(th[k] - MC.ROT_NORMS[k % 4]) <= 1e-12 * MC.ROT_NORMS[k % 4]
    lim = 2.0 ** -13
    assert MC.ROT_NORMS[1] < 0.1 * lim and 0.8 * lim < MC.ROT_NORMS[2] < lim < MC.ROT_NORMS[3] < 1.3 * lim
    for j in range(3):
        b = C - 18 + 6 * j
        assert abs(np.linalg.norm(dx[b: b + 3]) - MC.ROT_NORMS[j]) <= 1e-12 * max(MC.ROT_NORMS[j], 1e-300)
    st, dX = O.Oracle(p).apply_update(p.state_init, dx)
    assert np.isfinite(st).all() and dX > 0.0
    # a zero rotation step leaves the quaternion as it is, bit for bit
    o = MC._frame_offset(p, 0)
    assert np.array_equal(st[o: o + 4], p.state_init[o: o + 4])
