"""kb_sp_covariance / kb_sp_curve_covariance against the dense reference of tests/spline_cov_ref.py.

Every (case, state, lambda) of spline_cov_ref.TABLE is compared: Sigma_theta,theta, Sigma_s,theta and every band block,
correlation-normalised (|dev - ref|_ij / sqrt(ref_ii ref_jj)), under spline_cases.dx_bar(floor) with the entry's own
floor (tests/test_spline_cov_ref.py holds every floor to FLOOR_MAX without a device).  n in {2, 3, 4, 7, 12, 16, 17, 32,
33, 35, 64, 65} covers the top-only walk, both parities of the l / r pairing and strides with more and fewer than 16
nodes; K mod 3 in {0, 1, 2} the padded slots; c23 .. c64 every k_sp_cov_cam<CM>.
"""
import numpy as np
import pytest

from kalibr_amd import capi, synth

from . import spline_cases as SC
from . import spline_cov_ref as CR

pytestmark = pytest.mark.gpu


def _built(g, state, lam):
    g.set_state(state)
    g.build()
    g.set_constant_conditioner(lam)


def _check_blocks(dev, S, C, K, floor, tag):
    errs = CR.block_errors(dev, S, C, K)
    bar = SC.dx_bar(floor)
    print(f"[{tag}] " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"  floor {floor:.2e}  bar {bar:.1e}")
    assert floor <= SC.FLOOR_MAX
    for k, v in errs.items():
        assert v < bar, (tag, k, v, bar)


def _check_symmetric(out, K):
    assert np.array_equal(out["Ptt"], out["Ptt"].T)
    d0 = out["Pband"][:, 0]
    assert np.array_equal(d0, np.transpose(d0, (0, 2, 1)))


@pytest.mark.parametrize("name", SC.NAMES)
def test_parity(name):
    """every table entry of the case: the blocks against Sigma_ref, ok as kb_sp_solve's, exact symmetry of Sigma_tt and
    of the (k, k) blocks; at (init, 10) a second call returns the same bits"""
    r = SC.ref(name)
    g = capi.SplineSolver(r.p)
    try:
        for n, which, lam in CR.ENTRIES:
            if n != name:
                continue
            pd, S, floor = CR.entry(name, which, lam)
            assert pd
            _built(g, CR.state_of(r, which), lam)
            ok_s, _ = g.solve()
            ok, out = g.covariance(cross=True)
            assert ok and ok_s
            _check_blocks(out, S, g.C, g.K, floor, f"{name} {which} lambda={lam:g}")
            _check_symmetric(out, g.K)
            # blocks past the last coefficient are zeros
            for d in range(1, 4):
                assert np.all(out["Pband"][g.K - d:, d] == 0.0)
            if (which, lam) == ("init", 10.0):
                ok2, out2 = g.covariance(cross=True)
                assert ok2 and all(np.array_equal(out[k], out2[k]) for k in out)
                ok3, out3 = g.covariance(cross=False, band=False)
                assert ok3 and out3["Pst"] is None and out3["Pband"] is None and np.array_equal(out3["Ptt"], out["Ptt"])
    finally:
        g.close()


def test_not_ok_leaves_outputs_untouched():
    """imu_none at lambda = 0: no term touches the IMU columns, their pivots are exactly 0, kb_sp_solve says 0 and so
    does the query, which leaves prefilled buffers as they were"""
    r = SC.ref("imu_none")
    g = capi.SplineSolver(r.p)
    try:
        _built(g, r.p.state_init, 0.0)
        ok_s, _ = g.solve()
        buf = dict(Ptt=np.full((g.C, g.C), 7.0), Pst=np.full((6 * g.K, g.C), 7.0), Pband=np.full((g.K, 4, 6, 6), 7.0))
        ok, out = g.covariance(cross=True, out=buf)
        assert ok is False and ok_s is False
        assert all(np.all(buf[k] == 7.0) for k in buf)
        okc, P = g.curve_covariance(r.p.frame_time[:3])
        assert okc is False and np.all(P == 0.0)
        # the same handle under lambda = 10 answers
        g.set_constant_conditioner(10.0)
        ok, out = g.covariance(cross=True, out=buf)
        assert ok and np.all(np.isfinite(buf["Ptt"]))
    finally:
        g.close()


@pytest.mark.parametrize("name", ["n4", "n33"])
def test_query_leaves_solver_as_a_solve_does(name):
    """dx and the state are bitwise those of a plain kb_sp_solve; apply_update after the query applies that dx; three
    captured GN passes after a query end at the bits of three passes without it"""
    r = SC.ref(name)
    g, h = capi.SplineSolver(r.p), capi.SplineSolver(r.p)
    try:
        for sv in (g, h):
            _built(sv, r.p.state_init, 10.0)
        ok, dx = h.solve()
        okc, _ = g.covariance(cross=True)
        assert ok and okc
        assert np.array_equal(g.get_state(), r.p.state_init)
        dX_g, dX_h = g.apply_update(), h.apply_update()  # the device-resident dx of either call
        assert dX_g == dX_h
        assert np.array_equal(g.get_state(), h.get_state())
        _built(g, r.p.state_init, 10.0)  # a solve after a query returns the plain solve's dx
        assert g.covariance()[0]
        okg, dxg = g.solve()
        assert okg and np.array_equal(dxg, dx)
        for sv in (g, h):
            sv.set_state(r.p.state_init)
        g.run_gn(1)  # (captures the pass)
        h.run_gn(1)
        g.build()
        g.set_constant_conditioner(10.0)
        assert g.covariance()[0]
        g.curve_covariance(r.p.frame_time[:2])
        g.run_gn(2)
        h.run_gn(2)
        assert np.array_equal(g.get_state(), h.get_state())
    finally:
        g.close()
        h.close()


@pytest.mark.parametrize("name", ["n7", "n33", "knots"])
def test_curve_covariance(name):
    """at frame times, at a knot, at t_min and t_max against the numpy reference over the dense Sigma_ref, under the
    entry's bar; a time outside the interval is refused"""
    r = SC.ref(name)
    p = r.p
    pd, S, floor = CR.entry(name, "init", 10.0)
    t_min, t_max = p.knots[p.order - 1], p.knots[-p.order]
    times = np.concatenate([p.frame_time, [p.knots[p.order + 1], t_min, t_max]])
    g = capi.SplineSolver(p)
    try:
        _built(g, p.state_init, 10.0)
        ok, P = g.curve_covariance(times)
        P_ref, scale = CR.curve_ref(S, g.C, p.knots, p.order, times)
        e = float((np.abs(P - P_ref) / scale).max())
        print(f"[{name}] curve covariance at {times.size} times: {e:.2e}  floor {floor:.2e}  bar {SC.dx_bar(floor):.1e}")
        assert ok and pd and floor <= SC.FLOOR_MAX
        assert e < SC.dx_bar(floor)
        ok2, P2 = g.curve_covariance(times)
        assert ok2 and np.array_equal(P, P2)
        st = g.get_state()
        for bad in (t_min - 1e-3, t_max + 1e-3):
            with pytest.raises(capi.KbError, match="outside the spline interval"):
                g.curve_covariance([times[0], bad])
        assert np.array_equal(g.get_state(), st)
    finally:
        g.close()


@pytest.mark.parametrize("name", ["n4", "n33"])
def test_motion_error_and_priors_are_part_of_the_system(name):
    """with W_MOTION set, and with position priors as well: the inverse of the oracle's system built with those terms"""
    from oracle import oracle as O
    p = SC.problem(name)
    pri = synth.make_position_priors(p, 0, rate=50.0, seed=3)
    g = capi.SplineSolver(p)
    try:
        for tag, kw in (("motion", dict(motion_W=SC.W_MOTION, motion_order=2)),
                        ("motion+priors", dict(motion_W=SC.W_MOTION, motion_order=2, position_priors=pri))):
            o = O.SplineOracle(p, **kw)
            g.set_motion_error(SC.W_MOTION, 2)
            if "position_priors" in kw:
                g.set_position_priors(*pri)
            H = CR.dense(o.system(p.state_init, nthreads=4), 10.0)
            S, floor = CR.reference(H)
            _built(g, p.state_init, 10.0)
            ok, out = g.covariance(cross=True)
            assert ok
            _check_blocks(out, S, g.C, g.K, floor, f"{name} {tag}")
    finally:
        g.close()


def test_weighted_handle_inverts_the_weighted_system():
    """a uniform invR = I / sigma^2 and Huber on the reprojection family: the inverse of the weighted system of
    tests/spline_robust_ref.py at lambda = 10 (the query inverts what kb_sp_build made)"""
    from . import spline_robust_ref as RB
    rr = RB.ref("n7")
    kinds = {"reprojection": RB.HUBER_ALL["reprojection"]}
    rob = rr.robust(kinds, RB.INVR)
    H = CR.dense(rob.system(rr.p.state_init), 10.0)
    S, floor = CR.reference(H)
    g = capi.SplineSolver(rr.p)
    try:
        RB.apply_settings(g, kinds, RB.INVR)
        _built(g, rr.p.state_init, 10.0)
        ok, out = g.covariance(cross=True)
        assert ok
        _check_blocks(out, S, g.C, g.K, floor, "n7 huber+invR")
        # and not the unweighted one
        H0 = CR.dense(rr.o.system(rr.p.state_init, nthreads=4), 10.0)
        assert CR.corr_diff(CR.inv_equilibrated(H0)[:g.C, :g.C], S[:g.C, :g.C]) > 1e-3
    finally:
        g.close()


def test_refused_before_build():
    p = SC.problem("n4")
    g = capi.SplineSolver(p)
    try:
        g.set_state(p.state_init)
        with pytest.raises(capi.KbError, match="build first"):
            g.covariance()
        with pytest.raises(capi.KbError, match="build first"):
            g.curve_covariance(p.frame_time[:2])
    finally:
        g.close()


@pytest.mark.parametrize("name", ["n4", "n33"])
def test_schur_sums_in_their_own_launch(monkeypatch, name):
    """KSP_ZSF=0 (k_sp_zschur instead of the top level's extra blocks) is accepted and agrees bitwise with the default.

    The two solves sum the Schur complement in different orders (by default node 0's Z_R^T Z_R is added last, with
    KSP_ZSF=0 it is the first summand of k_sp_zschur's block 0), so their dx differ in the last bits; the query sums S
    once more in k_sp_zschur's order on a default handle before it inverts it, and every factor it reads besides S is
    the same in both modes."""
    p = SC.problem(name)
    g = capi.SplineSolver(p)
    monkeypatch.setenv("KSP_ZSF", "0")
    h = capi.SplineSolver(p)
    try:
        outs = []
        for sv in (g, h):
            _built(sv, p.state_init, 10.0)
            ok, out = sv.covariance(cross=True)
            assert ok
            outs.append(out)
        for k in outs[0]:
            print(f"[{name}] KSP_ZSF=0 against the default, {k}: max |diff| {np.abs(outs[0][k] - outs[1][k]).max():.2e}")
        for k in outs[0]:
            assert np.array_equal(outs[0][k], outs[1][k]), k
    finally:
        g.close()
        h.close()
