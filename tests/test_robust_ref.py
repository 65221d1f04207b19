"""The numpy restatement of robust terms (tests/robust_ref.py) checked on the CPU: with unit weights it reproduces the
oracle's Optimizer2 run; the five weight functions hold at hand-computed points; the C-ABI exports the new entries."""
import math
import os
import re

import numpy as np
import pytest

from kalibr_amd import synth

from . import robust_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RIGS = {
    "c1_small": lambda: synth.make_config(1, n_frames=12),
    "c2_small": lambda: synth.make_config(2, n_frames=60),
}


@pytest.mark.parametrize("name", list(RIGS))
@pytest.mark.parametrize("policy", ["lm", "gn"])
def test_unit_weights_reproduce_the_oracle(oracle_mod, name, policy):
    p = RIGS[name]()
    o = oracle_mod.Oracle(p)
    kw = dict(policy=policy, lambda0=10.0, max_iterations=8 if policy == "gn" else 200, eps_x=1e-3, eps_j=1.0)
    st_o, r_o = o.optimize(p.state_init, **kw)
    st_r, r_r = R.Robust(o).optimize(p.state_init, **kw)
    print(name, policy, r_o["iterations"], r_o["J_final"], r_r["J_final"])
    assert r_r["iterations"] == r_o["iterations"] and r_r["failed_iterations"] == r_o["failed_iterations"]
    assert np.array_equal(r_r["trace"][:, 3], r_o["trace"][:, 3])
    assert abs(r_r["J_final"] - r_o["J_final"]) <= 1e-12 * r_o["J_final"]
    assert abs(r_r["J_start"] - r_o["J_start"]) <= 1e-12 * r_o["J_start"]


def test_unit_weight_system_is_the_oracles_arrow(oracle_mod):
    p = RIGS["c1_small"]()
    o = oracle_mod.Oracle(p)
    A = o.arrow(p.state_init)
    S = R.Robust(o).system(p.state_init)
    for k in ("Hff", "Hfc", "Hcc", "gf", "gc"):
        assert np.abs(S[k] - A[k]).max() <= 1e-12 * np.abs(A[k]).max(), k
    assert abs(S["cost"] - A["cost"]) <= 1e-12 * A["cost"]


def test_weight_functions_at_hand_computed_points():
    w = R.weight
    # Huber(2): 1 below k^2 = 4, k / sqrt(s) from s = k^2 on (the comparison is s < k^2)
    assert w(R.HUBER, 2.0, 0.0) == 1.0 and w(R.HUBER, 2.0, 3.999) == 1.0
    assert w(R.HUBER, 2.0, 4.0) == 1.0  # 2 / sqrt(4): the second branch, continuous
    assert w(R.HUBER, 2.0, 16.0) == 0.5 and w(R.HUBER, 2.0, 400.0) == 0.1
    # Cauchy(4): 1 / (1 + s / 4)
    assert w(R.CAUCHY, 4.0, 0.0) == 1.0 and w(R.CAUCHY, 4.0, 4.0) == 0.5 and w(R.CAUCHY, 4.0, 12.0) == 0.25
    # Geman-McClure(9): 9 / (9 + s)^2 (1/9 at s = 0, not 1: the reference's form)
    assert w(R.GEMAN_MCCLURE, 9.0, 0.0) == 9.0 / 81.0 and w(R.GEMAN_MCCLURE, 9.0, 1.0) == 0.09
    assert w(R.GEMAN_MCCLURE, 9.0, 21.0) == 0.01
    # Blake-Zisserman(2, 0.999, 0.1): eps = 9 exp(-chi2inv(0.999, 2)) = 9 (1 - 0.999)^2 = 9e-6
    eps = R.blake_zisserman_epsilon(2, 0.999, 0.1)
    assert abs(eps - 9e-6) <= 1e-18
    assert w(R.BLAKE_ZISSERMAN, eps, 0.0) == 1.0 / (1.0 + eps)
    s_cut = -2.0 * math.log(1.0 - 0.999)  # the weight at the cut is wCut
    assert abs(w(R.BLAKE_ZISSERMAN, eps, s_cut) - 0.1) <= 1e-12
    assert w(R.BLAKE_ZISSERMAN, eps, 1000.0) == 0.0  # exp underflow: weight 0, no NaN
    assert w(R.NONE, 0.0, 7.0) == 1.0


def test_python_binding_epsilon_matches():
    from kalibr_amd import capi
    assert capi.blake_zisserman_epsilon(2, 0.999, 0.1) == R.blake_zisserman_epsilon(2, 0.999, 0.1)
    with pytest.raises(ValueError):
        capi.blake_zisserman_epsilon(3, 0.999, 0.1)


def test_contamination_is_seeded_and_gross():
    p = RIGS["c1_small"]()
    q, idx = R.contaminate(p, 5)
    q2, idx2 = R.contaminate(p, 5)
    assert np.array_equal(q.y, q2.y) and np.array_equal(idx, idx2)
    d = np.linalg.norm(q.y - p.y, axis=1)
    assert idx.size == round(0.03 * p.n_corners) and np.all(d[idx] >= 20.0 - 1e-9) and np.all(d[idx] <= 60.0 + 1e-9)
    assert np.count_nonzero(d) == idx.size


def test_c_abi_declares_and_exports_the_new_entries():
    names = ["kb_set_mestimator", "kb_set_corner_invR", "kb_get_mestimator_weights"]
    hdr = open(os.path.join(ROOT, "include", "kalibr_hip.h")).read()
    src = open(os.path.join(ROOT, "kalibr_amd", "csrc", "kb_capi.hip")).read()
    for n in names:
        assert re.search(r"\bint %s\(kb_handle\* h" % n, hdr), n
        assert re.search(r"^int %s\(kb_handle\* h" % n, src, re.M), n
    for k in ("KB_MEST_NONE = 0", "KB_MEST_HUBER = 1", "KB_MEST_CAUCHY = 2", "KB_MEST_GEMAN_MCCLURE = 3",
              "KB_MEST_BLAKE_ZISSERMAN = 4"):
        assert k in hdr
    from kalibr_amd import build, capi
    if os.path.exists(build.OUT):  # the built library exports them (no device needed to load it)
        L = capi.lib()
        for n in names:
            assert hasattr(L, n), n


def test_header_library_and_binding_lists_agree_for_names_of_any_case():
    """tests/test_capi_boundary.py matches lower-case names only, so it does not see kb_set_corner_invR.  The same
    three-way agreement with a pattern that takes upper-case letters: every kb_* function the header declares is in
    EXPORTS or EXPORTS_MIXED_CASE and nothing else is, the library exports it, and the binding gave it its int
    return type."""
    import ctypes
    from kalibr_amd import capi
    txt = open(os.path.join(ROOT, "include", "kalibr_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"\b(kb_[A-Za-z_0-9]+)\s*\(", txt)))
    assert "kb_set_corner_invR" in declared
    assert declared == sorted(capi.EXPORTS + capi.EXPORTS_MIXED_CASE)
    assert all(n != n.lower() for n in capi.EXPORTS_MIXED_CASE) and all(n == n.lower() for n in capi.EXPORTS)
    L = capi.lib()
    for n in capi.EXPORTS_MIXED_CASE:
        assert hasattr(L, n), n
        assert getattr(L, n).restype is ctypes.c_int and getattr(L, n).argtypes, n
