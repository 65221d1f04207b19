"""k_buildp's block epilogue against the CPU oracle: the partial-row store of the frame waves (schur_tiles_store_x:
per-tile packed index, step and count, the EX reads at clamped indices) and the view waves' expansion it subtracts
from, at every position the camera block's last row and the tile grid can take to each other.

Every problem gets two checks.  The per-call build() runs the non-expanded store; the fused Gauss-Newton pass
(optimize(policy="gn") and run_gn) runs the expanded one wherever C > 64.  A wrong index step, count or clamp puts
entries of S = H_cc - sum H_fc^T A_f (or of b) into other entries or drops them: whole digits of the step, far outside
the bars below.

  camera count   rigs of 4, 5, 6, 7, 8 pinhole-radtan cameras at 9 frames: C = 50, 64, 78, 92, 106.  The expanded path
                 is off for the first two and on for the last three; C = 64 puts row C (the b row) at the head of a
                 new tile, the others put it at positions 2, 14, 12 and 10 of the last tile.
  frames/block   the 6- and 8-camera rigs at 257 frames and the 8-camera rig at 513 frames, p_view 0.7: two and three
                 frames per block, both view-buffer parities, an odd count, a short last block, views without corners.
  intrinsics     configs[2]'s mixed omni-radtan + EUCM rig (the wide two-model instantiation, C = 48) at 12 frames, a
                 6-camera rig mixing those two models with pinhole-radtan (the all-model instantiation, 9, 6 and 8
                 intrinsics, C = 76), and a 6-camera pinhole-radtan + EUCM rig (8 and 6 intrinsics, C = 74), so that
                 the expanded path sees cameras with unequal intrinsic counts.

Undamped Gauss-Newton is not defined on a rig with omni-radtan cameras: the oracle's own passes fail from the initial
state, from the true state and from its LM solution alike (one accepted step of ~1e3..1e10 in the state, then three
failed ones; tests/test_gpu_sharded_local.py notes the same), so rounding decides the trajectory and there are no
"oracle's three passes" to compare with.  The two rigs with omni-radtan cameras therefore get the per-call check only;
the pinhole-radtan + EUCM rig, on which the oracle's three passes succeed, carries the unequal intrinsic counts
through the fused, expanded path.

Bars, as in test_gpu_parity.py and test_gpu_syrk_operands.py: normal-equation blocks and rhs 1e-10 of the block
maximum, cost 1e-12 relative; after three undamped Gauss-Newton passes J_final 1e-9 relative and every state entry
within 1e-6 of the oracle's three passes.  Each test asserts that the handle runs k_buildp.
"""
import numpy as np
import pytest

from kalibr_amd import synth

pytestmark = pytest.mark.gpu

GN = dict(policy="gn", max_iterations=3)
PR, OR, EU = synth.PINHOLE_RADTAN, synth.OMNI_RADTAN, synth.EUCM
_cache = {}


def _rig(n, n_frames, p_view=1.0):
    return lambda: synth.make_problem([PR] * n, n_frames, seed=20261019 + n, p_view=p_view,
                                      name=f"{n}-cam pinhole-radtan rig, {n_frames} frames")


# name -> (problem, C, expanded partials in the fused pass)
PROBLEMS = {
    "n4 f9": (_rig(4, 9), 50, False),
    "n5 f9": (_rig(5, 9), 64, False),
    "n6 f9": (_rig(6, 9), 78, True),
    "n7 f9": (_rig(7, 9), 92, True),
    "n8 f9": (_rig(8, 9), 106, True),
    "n6 f257": (_rig(6, 257, 0.7), 78, True),
    "n8 f257": (_rig(8, 257, 0.7), 106, True),
    "n8 f513": (_rig(8, 513, 0.7), 106, True),
    "c3 f12": (lambda: synth.make_config(3, n_frames=12, p_view=0.8), 48, False),
    "mixed6 f12": (lambda: synth.make_problem([OR, EU, PR, OR, EU, PR], 12, seed=20261019, p_view=0.8,
                                              name="6-cam omni-radtan + EUCM + pinhole-radtan rig, 12 frames"), 76, True),
    "eucm6 f12": (lambda: synth.make_problem([PR, EU, PR, PR, EU, PR], 12, seed=20261019, p_view=0.8,
                                             name="6-cam pinhole-radtan + EUCM rig, 12 frames"), 74, True),
}
GN_UNDEFINED = ("c3 f12", "mixed6 f12")  # omni-radtan cameras: see the module docstring
SPARSE = ("n6 f257", "n8 f257", "n8 f513")


@pytest.fixture(scope="module")
def capi():
    from kalibr_amd import capi as K
    return K


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def _problem(name):
    if ("p", name) not in _cache:
        _cache["p", name] = PROBLEMS[name][0]()
    return _cache["p", name]


def _case(oracle_mod, name):
    """problem, the oracle's blocks at the initial state and its 3 GN passes: computed once, not modified"""
    if name not in _cache:
        p = _problem(name)
        o = oracle_mod.Oracle(p)
        A = o.arrow(p.state_init)
        st_o, r_o = o.optimize(p.state_init, nthreads=8, **GN)
        _cache[name] = (p, A, st_o, r_o)
    return _cache[name]


def _solver(capi, p, name):
    g = capi.Solver(p)
    assert g.build_kernel_name() == "k_buildp", name
    assert g.C == PROBLEMS[name][1] == p.cam_cols
    return g


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_per_call_build(capi, oracle_mod, name):
    p, A, _, _ = _case(oracle_mod, name)
    g = _solver(capi, p, name)
    g.set_state(p.state_init)
    g.build()
    B = g.normal_blocks()
    figs = {k: _rel(B[k], A[k]) for k in ("Hff", "Hfc", "gf", "Hcc", "gc")}
    figs["rhs"] = _rel(g.rhs(), A["rhs"])
    figs["cost"] = abs(B["cost"] - A["cost"]) / A["cost"]
    g.close()
    print(name, "per-call build vs oracle:", " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    for k in ("Hff", "Hfc", "gf", "Hcc", "gc", "rhs"):
        assert figs[k] < 1e-10, k
    assert figs["cost"] <= 1e-12


@pytest.mark.parametrize("name", [n for n in PROBLEMS if n not in GN_UNDEFINED])
def test_fused_gn_three_passes(capi, oracle_mod, name):
    p, _, st_o, r_o = _case(oracle_mod, name)
    assert r_o["iterations"] == 3 and r_o["failed_iterations"] == 0 and np.isfinite(st_o).all()
    assert (p.cam_cols > 64) == PROBLEMS[name][2]  # the expanded partials are on exactly where C > 64
    g = _solver(capi, p, name)
    g.set_state(p.state_init)
    r_g = g.optimize(**GN)
    st_g = g.get_state()
    g.set_state(p.state_init)
    g.run_gn(3)
    st_r = g.get_state()
    g.close()
    print(f"{name}: J_final {r_g['J_final']:.15g}/{r_o['J_final']:.15g} max|state - oracle| optimize "
          f"{np.abs(st_g - st_o).max():.3e} run_gn(3) {np.abs(st_r - st_o).max():.3e}")
    assert r_g["iterations"] == 3 and r_g["failed_iterations"] == 0
    assert abs(r_g["J_final"] - r_o["J_final"]) <= 1e-9 * r_o["J_final"]
    assert np.abs(st_g - st_o).max() < 1e-6
    assert np.abs(st_r - st_o).max() < 1e-6


@pytest.mark.parametrize("name", SPARSE)
def test_sparse_problems_have_empty_views_and_short_last_blocks(name):
    """what the p_view 0.7 problems are there for: at least one (frame, camera) view without corners, and an odd
    frame count (the last of the two-frame blocks is short)"""
    p = _problem(name)
    seen = set(zip(p.view_frame.tolist(), p.view_cam.tolist()))
    cnt = np.diff(p.view_offset)
    assert len(seen) < p.n_frames * p.n_cams or (cnt == 0).any()
    assert p.n_frames % 2 == 1
