"""CPU preconditions of the spline covariance checks (tests/spline_cov_ref.py): every table entry is positive definite
and its reference reproduces itself to FLOOR_MAX; the table covers what it must; the selected-inverse recursion the
device walks, restated in numpy, equals the dense inverse; the curve-covariance reference is symmetric
positive semi-definite.  No device."""
import numpy as np
import pytest

from . import spline_cases as SC
from . import spline_cov_ref as CR


def test_table_coverage():
    assert set(CR.TABLE[("init", 10.0)]) == set(SC.NAMES) and len(SC.NAMES) == 28
    for key, need in CR.COVERAGE.items():
        names = CR.TABLE[key]
        assert len(set(names)) == len(names) >= need, key
    assert set(CR.TABLE[("s1", 10.0)]) <= set(SC.GN_NAMES) and len(SC.GN_NAMES) == 25
    # the sweeps the device checks rely on
    init10 = {SC.BY_NAME[n] for n in CR.TABLE[("init", 10.0)]}
    assert {c.n for c in init10} >= {2, 3, 4, 7, 12, 16, 17, 32, 33, 35, 64, 65}
    assert {c.kmod3 for c in init10} == {0, 1, 2}
    assert {c.C for c in init10} >= {23, 31, 37, 42, 44, 48, 51, 53, 64}


@pytest.mark.parametrize("name", SC.NAMES)
def test_entry_preconditions(name):
    """H + lambda^2 I positive definite and floor <= FLOOR_MAX at every entry of the case"""
    for n, which, lam in CR.ENTRIES:
        if n != name:
            continue
        pd, ref, floor = CR.entry(n, which, lam)
        print(f"[{n}] {which} lambda={lam:g}: pd {pd}  floor {floor:.2e}  bar {SC.dx_bar(floor):.1e}")
        assert pd
        assert floor <= SC.FLOOR_MAX, (n, which, lam, floor)
        assert np.array_equal(ref, ref.T)


def test_imu_none_is_singular_at_lambda_0():
    """no term touches the IMU columns without samples: their rows of H are exactly zero"""
    r = SC.ref("imu_none")
    H = CR.dense(r.sys0, 0.0)
    C = r.sys0["Hcc"].shape[0]
    assert np.all(H[C - 9:C] == 0.0)
    assert not CR.is_pd(H)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 7, 12, 16, 17, 33])
def test_recursion_equals_dense_inverse(n):
    b, C = 6, 5
    H = CR.random_arrow(n, b, C, seed=100 + n)
    S = np.linalg.inv(H)
    out = CR.selected_inverse(H, n, b, C)
    sc = np.abs(S).max()
    assert np.abs(out["Ptt"] - S[:C, :C]).max() <= 1e-13 * sc
    for i in range(n):
        a = C + i * b
        assert np.abs(out["St"][i] - S[a:a + b, :C]).max() <= 1e-13 * sc
        assert np.abs(out["D"][i] - S[a:a + b, a:a + b]).max() <= 1e-13 * sc
        if i + 1 < n:
            assert np.abs(out["X"][i] - S[a:a + b, a + b:a + 2 * b]).max() <= 1e-13 * sc


@pytest.mark.parametrize("name", ["n7", "knots"])
def test_curve_reference_is_psd(name):
    r = SC.ref(name)
    pd, S, floor = CR.entry(name, "init", 10.0)
    assert pd
    p = r.p
    C = r.sys0["Hcc"].shape[0]
    t_min, t_max = p.knots[p.order - 1], p.knots[-p.order]
    times = np.concatenate([p.frame_time[:5], [p.knots[p.order + 1], t_min, t_max]])
    P, scale = CR.curve_ref(S, C, p.knots, p.order, times)
    for q in range(len(times)):
        assert np.abs(P[q] - P[q].T).max() <= 1e-15 * np.abs(P[q]).max()
        assert np.linalg.eigvalsh(0.5 * (P[q] + P[q].T)).min() >= -1e-12 * np.abs(P[q]).max()
    assert np.all(scale > 0.0)
