"""The heads and tails of the GN pass kernels (k_buildp prologue and partial-row store, k_solve<0> staging) at the
smallest shapes at which they can go wrong, on the GN fused route with expanded partials (C > 64), against the CPU
oracle's 3 undamped Gauss-Newton iterations.

Bar (test_gpu_parity.py / test_gpu_fullsize.py): the same iteration count, J_final within 1e-9 relative, every state
entry within 1e-6 of the oracle.

  f2    8 cameras (C = 106), 2 frames: two blocks of one frame each (the prologue with G = 1), k_colsumx's 16 waves
        clamped onto 2 partial rows
  f17   8 cameras, 17 frames: one block more than the 16 column-sum waves
  f257  8 cameras, 257 frames, p_view 0.7: 2 frames per block, 129 blocks, the last one holds a single frame (the
        prologue's j < G clamp, the row store of a short block), ragged corner counts
  c78   6 cameras (C = 78, 5 tile rows), 24 frames: the smallest rig on this route; its image is well under one
        staging round of k_solve<0>, so the store predicate does the work
  c96   4 pinhole-radtan + 2 EUCM + 2 FOV (C = 96 = 6 * 16): row C (b) opens a tile row of its own.  The rig with
        C = 112 (6 omni-radtan + 2 pinhole-radtan) is not used: its camera block is rank-deficient without damping
        (as configs[2]'s, test_gpu_fullsize.py), and the oracle's Gauss-Newton diverges on it from every seed tried
        and from the true state, so there is no trajectory to compare; C = 96 is the largest multiple of 16 the
        other camera models reach with 8 cameras.
"""
import numpy as np
import pytest

from kalibr_amd import synth

pytestmark = pytest.mark.gpu

PR, EUCM, FOV = synth.PINHOLE_RADTAN, synth.EUCM, synth.PINHOLE_FOV
PROBLEMS = {
    "f2": lambda: synth.make_config(4, n_frames=2),
    "f17": lambda: synth.make_config(4, n_frames=17),
    "f257": lambda: synth.make_config(4, n_frames=257, p_view=0.7),
    "c78": lambda: synth.make_problem([PR] * 6, 24, seed=20261015 + 46),
    "c96": lambda: synth.make_problem([PR] * 4 + [EUCM] * 2 + [FOV] * 2, 24, seed=20261015 + 112),
}
GN = dict(policy="gn", max_iterations=3)
_cache = {}


@pytest.fixture(scope="module")
def capi():
    from kalibr_amd import capi as K
    return K


def _case(oracle_mod, name):
    """problem and the oracle's result, computed once per case and not modified"""
    if name not in _cache:
        p = PROBLEMS[name]()
        st_o, r_o = oracle_mod.Oracle(p).optimize(p.state_init, nthreads=8, **GN)
        _cache[name] = (p, st_o, r_o)
    return _cache[name]


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_gn_fused_parity(capi, oracle_mod, name):
    p, st_o, r_o = _case(oracle_mod, name)
    # the oracle converges on the case: 3 accepted steps, finite, cost decreasing
    assert r_o["iterations"] == 3 and r_o["failed_iterations"] == 0
    assert np.isfinite(st_o).all() and np.all(np.diff(r_o["trace"][:, 0]) < 0)
    g = capi.Solver(p)
    assert g.C == p.cam_cols and g.C > 64
    g.set_state(p.state_init)
    r_g = g.optimize(**GN)
    st_g = g.get_state()
    print(f"{name}: C={g.C} frames={p.n_frames} iterations {r_g['iterations']}/{r_o['iterations']} "
          f"J_final {r_g['J_final']:.15g}/{r_o['J_final']:.15g} max|state - oracle| {np.abs(st_g - st_o).max():.3e}")
    assert r_g["iterations"] == r_o["iterations"]
    assert r_g["failed_iterations"] == r_o["failed_iterations"]
    assert abs(r_g["J_final"] - r_o["J_final"]) <= 1e-9 * r_o["J_final"]
    assert np.abs(st_g - st_o).max() < 1e-6
    # the bench loop (kb_run_gn_iterations: the same passes without the convergence tests) takes the same 3 steps
    g.set_state(p.state_init)
    g.run_gn(3)
    st_r = g.get_state()
    g.close()
    print(f"{name}: run_gn(3) max|state - oracle| {np.abs(st_r - st_o).max():.3e}")
    assert np.abs(st_r - st_o).max() < 1e-6


def test_short_last_block_is_deterministic(capi):
    """f257: two fresh solvers agree bitwise after 5 passes (fixed reduction order, no stale load)"""
    p = PROBLEMS["f257"]()
    st = []
    for _ in range(2):
        g = capi.Solver(p)
        g.set_state(p.state_init)
        g.run_gn(5)
        st.append(g.get_state())
        g.close()
    assert np.isfinite(st[0]).all()
    assert np.array_equal(st[0], st[1])


@pytest.mark.parametrize("kw", [dict(), GN], ids=["lm", "gn"])
def test_short_last_block_graph_equals_eager(capi, kw):
    """f257: the captured passes and the eager per-pass loop give the same bits (the default LM run, whose builds
    take the prologue without a pending step, and the GN fused run)"""
    p = PROBLEMS["f257"]()
    a = capi.Solver(p)
    a.set_state(p.state_init)
    ra = a.optimize(use_graph=True, **kw)
    b = capi.Solver(p)
    b.set_state(p.state_init)
    rb = b.optimize(use_graph=False, sync_every=1, **kw)
    assert ra["iterations"] == rb["iterations"]
    assert np.array_equal(a.get_state(), b.get_state())
    a.close()
    b.close()
