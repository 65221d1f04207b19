"""The build kernels of the six one-model camera sets that no other module launches (omni-radtan, EUCM, omni,
double-sphere, pinhole-equidistant, pinhole-FOV: kb_build_tu.hip at KB_TU_ID 1 .. 6) and the limit branches of the
device maths (kb_math.h), against the CPU oracle.  The rigs, the crafted states and the oracle's side are
tests/model_set_cases.py's; tests/test_model_set_cases.py holds their preconditions.

Every handle asserts build_kernel_name() and the camera-block width of the case table.

  1. per-call parity, 18 rigs (x1: k_build<1>, x4: k_buildp<5>, x8: k_buildp<7>), at state_init and state_truth:
     eval_cost, build() + normal_blocks(), rhs(), solve() at lambda = 10
  2. the 12 x4 / x8 rigs through k_build<4 | 7> (KB_BUILD_PIPE=0 at kb_create)
  3. three undamped Gauss-Newton passes (the GNF = true instantiations), optimize(policy="gn") and run_gn(3), on the
     rigs of model_set_cases.GN_ADMITTED.  Undamped Gauss-Newton is not defined on a rig of omni-radtan cameras
     (tests/test_gpu_buildp_tail.py; one accepted step and three failed ones in the oracle itself), and on the
     double-sphere x1 rig the oracle's own three passes move by 8.8e-6 with its summation order: those rigs get checks
     1, 2, 4 and 5's per-call part only
  4. the weighted instantiations on the six x4 rigs, contaminated: Huber (both branches occur) and a per-corner invR,
     through k_build<.., WT> ("general") and the weighted k_buildp ("pipe"), against tests/robust_ref.py
  5. two frames per block with and without the per-view table on the six large rigs (FOV, EUCM, omni-radtan: 5, 6, 9
     intrinsics) at two blocks per CU (x4 f515) and one (x8 | x7 f257): the per-call blocks and, where admitted, the
     three passes
  6. branch edges: FOV's r^2 < 1e-5 and w^2 < 1e-5 limits, the equidistant r <= 1e-8 scale -- in the one-model FOV and
     equidistant instantiations and in configs 6 (the all-models one, which tells the two apart at run time), through
     k_buildp and k_build -- and update_pose's theta < 2^-13 series.  r = 0 exactly is left out: the equidistant
     Jacobian is 0 / 0 there in the reference, the oracle and the device alike.

Bars (tests/test_gpu_parity.py, tests/test_gpu_buildp_tail.py): cost 1e-12 relative; blocks and rhs 1e-10 of the block
maximum; dx 1e-8 of max|dx|; after three passes J_final 1e-9 relative and every state entry within 1e-6; (w, s) 1e-12
(tests/test_gpu_robust.py); apply_update 1e-14 with the same dX and a bitwise revert (test_update_revert).

Worst figures measured on an MI355X (every test prints its own):
  1. blocks 3.3e-15 at state_init; at state_truth, where the gradient nearly cancels, gf 6.4e-12, gc and rhs 2.5e-11;
     build cost 7.8e-15, eval_cost 1.5e-14, dx 3.9e-12
  2. blocks and rhs 9.7e-15, cost 1.9e-15
  3. J_final 4.8e-14; state 1.5e-12, double-sphere x4 / x8 9.5e-10 / 1.1e-9 (the oracle's own spread there: 5e-9)
  4. blocks and rhs 7.2e-15, cost 6.6e-16, s 3.8e-13, w 7.0e-14; the same through k_build and k_buildp
  5. blocks 5.1e-15, rhs 1.7e-14, cost 1.2e-15; J_final 3.9e-15, state 2.0e-12; the same figures with and without
     the table
  6. blocks and rhs 1.1e-14, cost 5.0e-15, w's rows and columns exactly zero; apply_update bitwise the oracle's
"""
import numpy as np
import pytest

from . import model_set_cases as MC
from . import robust_ref as R
from . import test_gpu_robust as T

pytestmark = pytest.mark.gpu

BLOCKS = ("Hff", "Hfc", "gf", "Hcc", "gc")
_cache = {}


@pytest.fixture(scope="module")
def capi():
    from kalibr_amd import capi as K
    return K


def _handle(capi, p, kernel, C, monkeypatch=None, **env):
    """a handle created under the switches kb_create reads (KB_BUILD_PIPE, KB_BUILDP_VIEWTAB), which are unset again
    before anything else runs"""
    for k in ("KB_BUILD_PIPE", "KB_BUILDP_VIEWTAB"):
        if monkeypatch is not None:
            if k in env:
                monkeypatch.setenv(k, env[k])
            else:
                monkeypatch.delenv(k, raising=False)
    g = capi.Solver(p)
    if monkeypatch is not None:
        for k in env:
            monkeypatch.delenv(k, raising=False)
    assert g.build_kernel_name() == kernel
    assert g.C == C == p.cam_cols
    return g


def _block_figs(g, A):
    """build() at the handle's state against the oracle's blocks A"""
    g.build()
    B = g.normal_blocks()
    figs = {k: MC.rel(B[k], A[k]) for k in BLOCKS}
    figs["rhs"] = MC.rel(g.rhs(), A["rhs"])
    figs["cost"] = abs(B["cost"] - A["cost"]) / A["cost"]
    return figs, B


def _check_blocks(what, figs):
    print(what, "vs oracle:", " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    for k in BLOCKS + ("rhs",):
        assert figs[k] < 1e-10, (what, k)
    assert figs["cost"] <= 1e-12, what


def _check_gn(what, g, p, st_o, r_o):
    assert r_o["iterations"] == 3 and r_o["failed_iterations"] == 0 and np.isfinite(st_o).all()
    g.set_state(p.state_init)
    r_g = g.optimize(**MC.GN)
    st_g = g.get_state()
    g.set_state(p.state_init)
    g.run_gn(3)
    st_r = g.get_state()
    print(f"{what}: J_final rel {abs(r_g['J_final'] - r_o['J_final']) / r_o['J_final']:.2e} max|state - oracle| "
          f"optimize {np.abs(st_g - st_o).max():.3e} run_gn(3) {np.abs(st_r - st_o).max():.3e}")
    assert r_g["iterations"] == 3 and r_g["failed_iterations"] == 0
    assert abs(r_g["J_final"] - r_o["J_final"]) <= 1e-9 * r_o["J_final"]
    assert np.abs(st_g - st_o).max() < 1e-6
    assert np.abs(st_r - st_o).max() < 1e-6


# ---------------------------------------------------------------- 1. per-call parity
@pytest.mark.parametrize("name", MC.SMALL)
def test_per_call_parity(capi, oracle_mod, name):
    r, ref = MC.RIGS[name], MC.ref(name)
    g = _handle(capi, ref.p, r.kernel, r.C)
    for which in ("init", "truth"):
        st, A = ref.state(which), ref.arrow(which)
        g.set_state(st)
        Jo = ref.o.cost(st)
        figs, _ = _block_figs(g, A)
        figs["eval_cost"] = abs(g.eval_cost() - Jo) / Jo
        g.set_constant_conditioner(10.0)
        ok, dx = g.solve()
        ok_o, dx_o = ref.solve(which)
        assert ok and ok_o
        figs["dx"] = MC.rel(dx, dx_o)
        _check_blocks(f"{name} {r.kernel} state_{which}", figs)
        assert figs["eval_cost"] <= 1e-12
        assert figs["dx"] < 1e-8
    g.close()


# ---------------------------------------------------------------- 2. k_build on the rigs that pipeline
@pytest.mark.parametrize("name", MC.PIPED)
def test_k_build_on_the_pipelined_rigs(capi, oracle_mod, monkeypatch, name):
    r, ref = MC.RIGS[name], MC.ref(name)
    g = _handle(capi, ref.p, "k_build", r.C, monkeypatch, KB_BUILD_PIPE="0")
    g.set_state(ref.p.state_init)
    figs, _ = _block_figs(g, ref.arrow("init"))
    g.close()
    _check_blocks(f"{name} k_build (KB_BUILD_PIPE=0)", figs)


# ---------------------------------------------------------------- 3. three Gauss-Newton passes
@pytest.mark.parametrize("name", [n for n in MC.GN_ADMITTED if n not in MC.LARGE])
def test_three_gauss_newton_passes(capi, oracle_mod, name):
    r, ref = MC.RIGS[name], MC.ref(name)
    st_o, r_o = ref.gn()
    g = _handle(capi, ref.p, r.kernel, r.C)
    _check_gn(name, g, ref.p, st_o, r_o)
    g.close()


# ---------------------------------------------------------------- 4. the weighted instantiations
def _robust_case(name):
    """(contaminated problem, the restatement's system at state_init): Huber k = 2 and a per-corner invR"""
    if ("w", name) not in _cache:
        from oracle import oracle as O
        p, _ = R.contaminate(MC.problem(name), T.SEED)
        kind, param = T.ESTIMATORS["huber"]
        S = R.Robust(O.Oracle(p), kind, param, T.invR_of("per_corner", p.n_corners)).system(p.state_init, True)
        S.pop("H")
        _cache["w", name] = (p, S)
    return _cache["w", name]


@pytest.mark.parametrize("mode,kernel", [("general", "k_build"), ("pipe", "k_buildp")])
@pytest.mark.parametrize("name", MC.X4)
def test_weighted_instantiations(capi, oracle_mod, name, mode, kernel):
    p, S = _robust_case(name)
    kind, k = T.ESTIMATORS["huber"]
    assert np.any(S["s"] < k * k) and np.any(S["s"] >= k * k) and S["w"].min() < 0.1  # both Huber branches
    g = _handle(capi, p, "k_buildp", MC.RIGS[name].C)
    g.set_robust_build(mode)
    g.set_mestimator(kind, k)
    g.set_corner_invR(T.invR_of("per_corner", p.n_corners))
    assert g.build_kernel_name() == kernel
    g.set_state(p.state_init)
    J = g.eval_cost()
    w, s = g.mestimator_weights()
    figs, _ = _block_figs(g, S)
    assert g.build_kernel_name() == kernel
    g.close()
    figs["eval_cost"] = abs(J - S["cost"]) / S["cost"]
    figs["s"] = float((np.abs(s - S["s"]) / np.maximum(1.0, np.abs(S["s"]))).max())
    figs["w"] = float((np.abs(w - S["w"]) / np.maximum(1.0, np.abs(S["w"]))).max())
    _check_blocks(f"{name} weighted {kernel}", figs)
    assert figs["eval_cost"] <= 1e-12
    assert figs["s"] <= 1e-12 and figs["w"] <= 1e-12


# ---------------------------------------------------------------- 5. frames per block and the per-view table
@pytest.mark.parametrize("table", [True, False], ids=["table", "no table"])
@pytest.mark.parametrize("name", MC.LARGE)
def test_two_frames_per_block(capi, oracle_mod, monkeypatch, name, table):
    r, ref = MC.RIGS[name], MC.ref(name)
    p = ref.p
    g = _handle(capi, p, "k_buildp", r.C, monkeypatch, **({} if table else {"KB_BUILDP_VIEWTAB": "0"}))
    assert g.build_viewtab() is table
    g.set_state(p.state_init)
    figs, _ = _block_figs(g, ref.arrow("init"))
    _check_blocks(f"{name} table {'on' if table else 'off'}", figs)
    if name in MC.GN_ADMITTED:
        st_o, r_o = ref.gn()
        _check_gn(f"{name} table {'on' if table else 'off'}", g, p, st_o, r_o)
    g.close()


# ---------------------------------------------------------------- 6. branch edges of the device maths
def _edge_oracle(name):
    if ("e", name) not in _cache:
        from oracle import oracle as O
        _cache["e", name] = O.Oracle(MC.edge_problem(name))
    return _cache["e", name]


def _check_state(capi, monkeypatch, what, p, o, st, pipe):
    """cost and blocks at st through k_buildp or k_build; returns the device's blocks"""
    env = {} if pipe else {"KB_BUILD_PIPE": "0"}
    g = _handle(capi, p, "k_buildp" if pipe else "k_build", p.cam_cols, monkeypatch, **env)
    g.set_state(st)
    A = o.arrow(st)
    Jo = o.cost(st)
    figs, B = _block_figs(g, A)
    figs["eval_cost"] = abs(g.eval_cost() - Jo) / Jo
    g.close()
    _check_blocks(what, figs)
    assert figs["eval_cost"] <= 1e-12
    return A, B


@pytest.mark.parametrize("pipe", [True, False], ids=["k_buildp", "k_build"])
@pytest.mark.parametrize("name", list(MC.EDGE_RIGS))
def test_small_radius_branches(capi, oracle_mod, monkeypatch, name, pipe):
    """corners at r^2 = 5e-6 | 2.5e-5 (FOV's limit 1e-5 between them) and r = 2.2e-9 | 1.4e-6 (the equidistant limit
    1e-8 between them) on the optical axis' side; r = 0 exactly is left out (0 / 0 in the equidistant Jacobian)"""
    p, st = MC.edge_problem(name), MC.edge_state(name)
    _check_state(capi, monkeypatch, f"{name} edge state {'k_buildp' if pipe else 'k_build'}", p, _edge_oracle(name), st,
                 pipe)


@pytest.mark.parametrize("pipe", [True, False], ids=["k_buildp", "k_build"])
@pytest.mark.parametrize("name", list(MC.SMALL_W))
def test_small_w_branch(capi, oracle_mod, monkeypatch, name, pipe):
    """FOV's w^2 < 1e-5 limit (w^2 = 1e-6, 9e-6): the identity, and w's rows and columns exactly zero on both sides"""
    p = MC.edge_problem(name)
    for st, ws in MC.small_w_states(name):
        A, B = _check_state(capi, monkeypatch, f"{name} w = {sorted(ws.values())} {'k_buildp' if pipe else 'k_build'}",
                            p, _edge_oracle(name), st, pipe)
        for cam in ws:
            c = MC.w_column(p, cam)
            for X in (A, B):
                assert not X["Hcc"][c].any() and not X["Hcc"][:, c].any() and not X["Hfc"][:, :, c].any()
                assert X["gc"][c] == 0.0


def test_update_pose_series_branch(capi, oracle_mod):
    """rotation steps of norm 0, 1e-5, 1.0e-4 and 1.5e-4: theta < 2^-13 takes 1/2 + theta^2 / 48 for sin(theta/2) /
    theta.  Beside test_update_revert's bar of 1e-14 the quaternions are held to 16 ulp of 1: at these angles the two
    forms agree to theta^4 / 3840 < 1e-19, an entry of the new quaternion is a sum of four products of magnitude <= 1
    (four roundings on either side) and the half-angle sine and cosine are good to 4 ulp in either library, while a
    wrong series coefficient moves an entry by theta^3 / 48 = 2e-14 at theta = 1e-4."""
    p = MC.edge_problem("fov x4")
    dx = MC.pose_steps(p)
    o = _edge_oracle("fov x4")
    g = _handle(capi, p, "k_buildp", p.cam_cols)
    g.set_state(p.state_init)
    dX = g.apply_update(dx)
    st_g = g.get_state()
    st_o, dX_o = o.apply_update(p.state_init, dx)
    q = []
    for k in range(p.n_cams - 1 + p.n_frames):
        b = p.n_cams * 10 + 7 * k
        q.extend(range(b, b + 4))
    print(f"apply_update: dX {dX!r} / {dX_o!r}; max|state - oracle| {np.abs(st_g - st_o).max():.2e}, quaternions "
          f"{np.abs(st_g[q] - st_o[q]).max():.2e}")
    assert dX == dX_o
    assert np.abs(st_g - st_o).max() < 1e-14
    assert np.abs(st_g[q] - st_o[q]).max() <= 16 * 2.0 ** -53
    g.revert()
    assert np.array_equal(g.get_state(), p.state_init)
    g.close()
