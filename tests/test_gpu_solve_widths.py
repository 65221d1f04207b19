"""kb_solve, kb_covariance and the loops over them at every camera-block width C at which the reduced-system path
changes its code (tests/solve_width_cases.py: the ends of every k_solve<CM> / k_cov_cam<CM> bucket, nb = 5, 6, 7 of the
blocked factorisation, the three k_schur<ms>, every step of cov_invert_columns' rounds), one handle per row.

Per row, at state_init and state_truth, for each admitted lambda: the per-call dx against the oracle's Schur solve and
against numpy.linalg.solve of the dense H (the oracle's LDL^T restates the kernel's algebra and could share a mistake;
LAPACK does not), camera part (k_solve) and frame part (k_backsub) apart; the residual; the covariance blocks against
numpy.linalg.inv of the dense H in test_gpu_covariance.py's metric; repeatability to the bit.  Rows 17, 65 and 111 again
on their first 13 frames; rows 17, 32, 64, 65, 80 and 111 under a diagonal conditioner; six LM iterations on every row
and three GN passes where undamped GN is defined; the non-positive-definite flag at C = 27 and C = 80.

Bars (test_gpu_parity.py, test_gpu_covariance.py): dx 1e-8 of max|dx|, residual 1e-9 of |rhs|, covariance 1e-8,
J_final 1e-9 relative, state 1e-6.  test_solve_width_cases.py holds the references to a tenth of these among
themselves.  Every handle asserts its C and build kernel.

Measured on an MI355X (worst over states and lambdas; dx against the oracle / against LAPACK):

    C     k_solve dx        k_backsub dx      resid    cov      LM it / failed  LM J     LM state  GN state (optimize / run_gn)
    16    2.1e-11 / 2.3e-11 1.1e-13 / 1.5e-13 6.4e-13  3.5e-11  5 / 0           1.7e-16  1.0e-12   4.5e-13 / 4.5e-13
    17    3.6e-12 / 1.6e-11 8.0e-13 / 6.8e-13 6.6e-13  1.3e-11  6 / 0           6.0e-15  5.7e-12   2.3e-13 / 2.3e-13
    24    2.3e-12 / 6.2e-12 7.1e-13 / 1.4e-12 1.6e-13  3.8e-12  6 / 0           4.0e-16  3.5e-12   -
    27    3.2e-11 / 3.5e-11 8.9e-14 / 8.2e-14 1.1e-12  3.6e-11  6 / 0           3.7e-15  2.8e-12   2.3e-13 / 2.3e-13
    31    2.2e-11 / 2.1e-11 9.8e-14 / 8.0e-14 3.1e-12  8.5e-11  6 / 0           1.1e-15  9.6e-12   4.4e-12 / 4.4e-12
    32    4.7e-11 / 4.0e-11 1.1e-13 / 9.7e-14 2.3e-12  1.7e-10  6 / 3           2.7e-14  1.8e-12   2.9e-11 / 2.9e-11
    33    1.6e-11 / 1.6e-11 2.4e-13 / 3.1e-13 2.0e-12  3.1e-11  6 / 0           6.3e-15  5.2e-12   3.4e-13 / 3.4e-13
    48    2.0e-11 / 3.5e-11 1.7e-13 / 2.2e-13 3.3e-12  6.8e-11  6 / 1           7.8e-13  2.5e-11   9.1e-13 / 9.1e-13
    49    1.3e-10 / 1.3e-10 2.0e-13 / 2.4e-13 2.8e-12  2.6e-10  6 / 0           2.7e-14  3.1e-11   5.5e-12 / 5.5e-12
    63    4.9e-11 / 5.4e-11 7.4e-14 / 8.0e-14 1.3e-11  1.4e-10  6 / 0           1.5e-15  6.1e-12   1.2e-12 / 1.2e-12
    64    8.5e-11 / 8.6e-11 1.0e-13 / 1.0e-13 1.7e-12  9.7e-11  6 / 0           3.0e-15  2.1e-11   1.5e-12 / 1.5e-12
    65    6.2e-11 / 6.1e-11 1.7e-13 / 1.9e-13 4.6e-12  1.0e-10  6 / 0           8.2e-16  1.5e-11   5.7e-13 / 5.7e-13
    79    4.5e-11 / 5.1e-11 9.4e-14 / 1.0e-13 4.2e-12  1.1e-10  6 / 2           3.4e-13  1.5e-11   2.3e-12 / 2.3e-12
    80    2.0e-10 / 2.0e-10 1.7e-13 / 2.1e-13 2.2e-12  2.4e-10  6 / 2           4.4e-13  1.2e-11   1.1e-11 / 1.1e-11
    81    1.2e-11 / 1.8e-10 1.7e-12 / 2.0e-12 2.3e-12  8.0e-11  6 / 0           5.6e-15  8.3e-12   -
    95    2.8e-11 / 7.0e-11 1.1e-13 / 1.7e-13 3.1e-12  1.1e-10  6 / 2           9.3e-12  2.0e-10   1.2e-11 / 1.2e-11
    96    8.1e-11 / 7.1e-11 3.5e-14 / 3.7e-14 7.2e-12  3.5e-10  6 / 2           2.8e-14  1.2e-11   3.4e-11 / 3.4e-11
    97    1.2e-10 / 1.2e-10 1.1e-13 / 1.1e-13 1.2e-11  3.8e-10  6 / 0           7.0e-15  4.9e-11   3.3e-11 / 3.3e-11
    111   4.6e-10 / 5.0e-10 1.2e-12 / 1.2e-12 9.3e-12  1.3e-09  6 / 0           2.6e-13  3.9e-10   -

    diagonal conditioner, C = 17: k_solve dx 2.0e-13 / 1.1e-12 k_backsub dx 7.3e-14 / 6.8e-14 resid 4.3e-15 cov 3.8e-12
    diagonal conditioner, C = 32: k_solve dx 9.0e-13 / 7.5e-12 k_backsub dx 1.3e-14 / 1.6e-14 resid 4.9e-15 cov 7.8e-12
    diagonal conditioner, C = 64: k_solve dx 2.2e-12 / 2.0e-12 k_backsub dx 2.7e-14 / 2.0e-14 resid 5.2e-15 cov 3.3e-12
    diagonal conditioner, C = 65: k_solve dx 3.8e-12 / 6.9e-12 k_backsub dx 1.6e-14 / 1.1e-14 resid 4.8e-15 cov 3.7e-12
    diagonal conditioner, C = 80: k_solve dx 2.0e-12 / 4.4e-12 k_backsub dx 1.4e-14 / 1.0e-14 resid 3.4e-15 cov 1.5e-11
    diagonal conditioner, C = 111: k_solve dx 2.5e-11 / 2.6e-11 k_backsub dx 5.1e-14 / 7.0e-14 resid 8.7e-15 cov 8.7e-11
    13 frames, C = 17: k_solve dx 4.0e-12 / 1.0e-11 k_backsub dx 5.4e-13 / 4.3e-13 resid 7.3e-13 cov 7.9e-12
    13 frames, C = 65: k_solve dx 3.1e-11 / 3.7e-11 k_backsub dx 1.8e-13 / 1.6e-13 resid 4.2e-12 cov 7.1e-11
    13 frames, C = 111: k_solve dx 4.1e-10 / 4.2e-10 k_backsub dx 2.1e-12 / 2.1e-12 resid 7.1e-12 cov 7.2e-10

The frame without corners (lambda = 10): dx 3.1e-13 (C = 27), 8.8e-12 (C = 80), covariance 1.6e-12, 6.9e-12,
|Sigma_ff - I / 100| = 0.  The module: 66 tests, 2.9 s.
"""
import numpy as np
import pytest

from . import solve_width_cases as W

pytestmark = pytest.mark.gpu

SENT = -7.25
_handles = {}


@pytest.fixture(scope="module")
def capi():
    from kalibr_amd import capi as K
    return K


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for g in _handles.values():
        g.close()
    _handles.clear()


def _handle(capi, key, p, C):
    """one handle per problem, created once; it asserts the path the row is there for"""
    if key not in _handles:
        g = capi.Solver(p)
        assert g.C == C == p.cam_cols, key
        assert g.build_kernel_name() == W.build_kernel(p.n_cams), key
        _handles[key] = g
    return _handles[key]


def _row(capi, C):
    return _handle(capi, ("row", C), W.problem(C), C), W.ref(C)


def _dx_figures(R, sname, lam, dx):
    """the device's dx against both references, camera part and frame part apart (each of max|dx| of its reference),
    and its residual in the dense system"""
    C = R.C
    ok_o, dx_o = R.oracle_dx(sname, lam)
    dx_l = R.dense_dx(sname, lam)
    rhs = R.arrow(sname)["rhs"]
    fig = {}
    for name, ref in (("oracle", dx_o), ("lapack", dx_l)):
        s = np.abs(ref).max()
        fig[f"cam/{name}"] = float(np.abs(dx[:C] - ref[:C]).max() / s)
        fig[f"frames/{name}"] = float(np.abs(dx[C:] - ref[C:]).max() / s)
    fig["resid"] = float(np.linalg.norm(R.H(sname, lam) @ dx - rhs) / np.linalg.norm(rhs))
    return ok_o, fig


def _assert_dx(fig, tag):
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert fig["cam/oracle"] <= W.DEV_DX and fig["cam/lapack"] <= W.DEV_DX, (tag, "k_solve", fig)
    assert fig["frames/oracle"] <= W.DEV_DX and fig["frames/lapack"] <= W.DEV_DX, (tag, "k_backsub", fig)
    assert fig["resid"] <= W.DEV_RESID, (tag, fig)


def _symmetric(out):
    assert np.array_equal(out["Pcc"], out["Pcc"].T)
    assert np.array_equal(out["Pff"], out["Pff"].transpose(0, 2, 1))


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("Pcc", "Pff", "Pfc"))


def _solve_and_covariance(g, R, lams, tag):
    """the per-call checks of one handle at both states: solve, covariance, repeatability"""
    for sname in W.STATES:
        g.set_state(getattr(R.p, sname))
        g.build()
        for lam in lams:
            t = f"{tag} {sname} lambda {lam:g}:"
            g.set_constant_conditioner(lam)
            ok, dx = g.solve()
            ok_o, fig = _dx_figures(R, sname, lam, dx)
            assert ok == ok_o and ok, t
            _assert_dx(fig, t)
            ok2, dx2 = g.solve()
            assert ok2 and np.array_equal(dx, dx2), t               # fixed summation order: bitwise repeatable
            okc, out = g.covariance(cross=True)
            assert okc == ok, t
            e = W.cov_errs(out, R.P(sname, lam), R.C)
            print(t, "covariance", " ".join(f"{k} {v:.2e}" for k, v in e.items()))
            assert max(e.values()) <= W.DEV_COV, (t, e)
            _symmetric(out)
            okc2, out2 = g.covariance(cross=True)
            assert okc2 and _same_bits(out, out2), t
            ok3, dx3 = g.solve()                                     # the query leaves the system as it was
            assert ok3 and np.array_equal(dx, dx3), t


@pytest.mark.parametrize("C", list(W.ROWS))
def test_solve_and_covariance(capi, C):
    g, R = _row(capi, C)
    assert W.lambdas(C) == ((1.0, 10.0) if C in W.SINGULAR_ROWS else (0.0, 1.0, 10.0))
    _solve_and_covariance(g, R, W.lambdas(C), f"C = {C}")


@pytest.mark.parametrize("C", W.SLICE_ROWS)
def test_thirteen_frames(capi, C):
    """an odd F: a short last block of k_cov_frames with one frame in its last wave, a short last block of k_backsub"""
    R = W.slice_ref(C)
    g = _handle(capi, ("slice", C), R.p, C)
    assert R.p.n_frames == W.SLICE_FRAMES and (g.ncols - g.C) // 6 == W.SLICE_FRAMES
    _solve_and_covariance(g, R, W.lambdas(C), f"C = {C}, {W.SLICE_FRAMES} frames")


@pytest.mark.parametrize("C", W.DIAG_ROWS)
def test_diagonal_conditioner(capi, C):
    g, R = _row(capi, C)
    sname, lam = "state_init", W.DIAG_LAMBDA
    g.set_state(R.p.state_init)
    g.build()
    g.set_constant_conditioner(10.0)
    ok10, dx10 = g.solve()
    ok10c, cov10 = g.covariance(cross=True)
    assert ok10 and ok10c
    g.set_conditioner(W.diagonal(g.ncols))
    ok, dx = g.solve()
    okc, out = g.covariance(cross=True)
    g.set_constant_conditioner(10.0)
    t = f"C = {C} diagonal conditioner:"
    assert ok and okc
    _, fig = _dx_figures(R, sname, lam, dx)
    _assert_dx(fig, t)
    e = W.cov_errs(out, R.P(sname, lam), C)
    print(t, "covariance", " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= W.DEV_COV, (t, e)
    _symmetric(out)
    assert np.abs(dx - dx10).max() > 1e-3 * np.abs(dx10).max()        # another system
    ok_b, dx_b = g.solve()                                             # the constant conditioner again: the same bits
    ok_bc, cov_b = g.covariance(cross=True)
    assert ok_b and ok_bc and np.array_equal(dx_b, dx10) and _same_bits(cov_b, cov10)


def _assert_loop(tag, r_g, st_g, r_o, st_o):
    dj = abs(r_g["J_final"] - r_o["J_final"]) / r_o["J_final"]
    ds = float(np.abs(st_g - st_o).max())
    print(f"{tag}: iterations {r_g['iterations']}/{r_o['iterations']} failed {r_g['failed_iterations']}/"
          f"{r_o['failed_iterations']} J_final rel {dj:.2e} max|state - oracle| {ds:.2e}")
    assert r_g["iterations"] == r_o["iterations"], tag
    assert r_g["failed_iterations"] == r_o["failed_iterations"], tag
    assert np.array_equal(r_g["trace"][:, 3], r_o["trace"][:, 3]), tag   # the same accept / revert decisions
    assert dj <= W.DEV_J and ds < W.DEV_STATE, tag


@pytest.mark.parametrize("C", list(W.ROWS))
def test_lm_loop(capi, C):
    g, R = _row(capi, C)
    st_o, r_o = R.loop("lm")
    g.set_state(R.p.state_init)
    r_g = g.optimize(**W.LM)
    _assert_loop(f"C = {C} LM", r_g, g.get_state(), r_o, st_o)


@pytest.mark.parametrize("C", W.GN_ROWS)
def test_gn_loops(capi, C):
    """optimize(policy="gn") and run_gn(3): for C > 64 the fused pass with expanded partials on the pipelined build"""
    g, R = _row(capi, C)
    st_o, r_o = R.loop("gn")
    assert r_o["iterations"] == 3 and r_o["failed_iterations"] == 0
    g.set_state(R.p.state_init)
    r_g = g.optimize(**W.GN)
    _assert_loop(f"C = {C} GN", r_g, g.get_state(), r_o, st_o)
    g.set_state(R.p.state_init)
    g.run_gn(3)
    ds = float(np.abs(g.get_state() - st_o).max())
    print(f"C = {C} run_gn(3): max|state - oracle| {ds:.2e}")
    assert ds < W.DEV_STATE


@pytest.mark.parametrize("C", W.NONPD_ROWS)
def test_not_positive_definite(capi, C):
    """a frame without corners: at lambda = 0 both entry points report ok = 0 and write nothing; damped, both succeed
    and that frame's step is 0, its Sigma_ff = I / lambda^2 and its Sigma_fc = 0"""
    R, f = W.nonpd_ref(C), W.nonpd_frame(C)
    p = R.p
    g = _handle(capi, ("nonpd", C), p, C)
    F = p.n_frames
    g.set_state(p.state_init)
    g.build()
    g.set_constant_conditioner(0.0)
    dx = np.full(g.ncols, SENT)
    ok = capi.C.c_int(1)
    capi._check(capi.lib().kb_solve(g.h, capi._d(dx), capi.C.byref(ok)))
    assert ok.value == 0 and np.all(dx == SENT)
    sent = dict(Pcc=np.full((C, C), SENT), Pff=np.full((F, 6, 6), SENT), Pfc=np.full((F, 6, C), SENT))
    okc, out = g.covariance(cross=True, out=sent)
    assert not okc and all(out[k] is sent[k] and np.all(sent[k] == SENT) for k in sent)
    g.set_constant_conditioner(10.0)
    ok, dx = g.solve()
    ok_o, fig = _dx_figures(R, "state_init", 10.0, dx)
    assert ok and ok_o
    _assert_dx(fig, f"C = {C}, frame {f} without corners, lambda 10:")
    assert not dx[C + 6 * f:C + 6 * f + 6].any()
    okc, out = g.covariance(cross=True)
    assert okc
    e = W.cov_errs(out, R.P("state_init", 10.0), C)
    d_ff = float(np.abs(out["Pff"][f] - np.eye(6) / 100.0).max())
    print(f"C = {C} covariance", e, f"|Sigma_ff - I/100| {d_ff:.1e}")
    assert max(e.values()) <= W.DEV_COV
    assert d_ff <= 1e-12 and not out["Pfc"][f].any()
    _symmetric(out)


def test_every_bucket_ran(capi):
    """the handles above cover both end rows of every bucket, on the path the table records"""
    for C, r in W.ROWS.items():
        g, _ = _row(capi, C)
        assert (g.C, W.solve_cm(g.C), W.schur_ms(g.C), W.nb(g.C)) == (C, r.cm, r.ms, r.nb)
        assert g.build_kernel_name() == ("k_buildp" if len(r.models) >= 4 else "k_build")
    for cm in (16, 24, 32, 48, 64, 0):
        assert sum(r.cm == cm for r in W.ROWS.values()) >= (1 if cm == 16 else 2)   # CM = 16: C = 16 and, elsewhere, 5
