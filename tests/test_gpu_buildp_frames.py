"""k_buildp over many frames per block against the CPU oracle: what a view wave or a frame wave keeps in registers
from one frame of its block to the next (lane-dependent addresses, the expansion tail's LDS indices and store
offsets, the accumulator form of the MFMAs) must hold for every frame of the block, for both parities of the view
buffers and for cameras whose intrinsic counts differ.  A value wrongly carried over shows in the frames after the
first of a block: with one to three frames per block (tests/test_gpu_buildp_tail.py) each parity is seen at most
twice, here it recurs.

  n6 f1027, n8 f1027   6- and 8-camera pinhole-radtan rigs at 1027 frames, p_view 0.7, seed 20261020 + n: five frames
                       per block, so each view-buffer parity recurs within a block; a short last block of 2 frames;
                       views without corners; C = 78 and 106, both on the expanded path.
  eucm6 f515           a 6-camera pinhole-radtan + EUCM rig ([PR, EU, PR, PR, EU, PR], 8 and 6 intrinsics, C = 74) at
                       515 frames, p_view 0.8: three frames per block and a short last block of 2, so the per-camera
                       column offsets are seen over several frames by cameras with unequal intrinsic counts.

The oracle's three undamped Gauss-Newton passes succeed on all three (3 iterations, 0 failed, a finite state; the
test asserts it), so every case gets both checks of tests/test_gpu_buildp_tail.py: the per-call build() and the fused
pass (optimize(policy="gn") and run_gn(3)).

Bars, as there: normal-equation blocks and rhs 1e-10 of the block maximum, cost 1e-12 relative; after three undamped
Gauss-Newton passes J_final 1e-9 relative and every state entry within 1e-6 of the oracle's three passes.  Each test
asserts that the handle runs k_buildp.
"""
import numpy as np
import pytest

from kalibr_amd import synth

pytestmark = pytest.mark.gpu

GN = dict(policy="gn", max_iterations=3)
PR, EU = synth.PINHOLE_RADTAN, synth.EUCM
_cache = {}


def _rig(n, n_frames, p_view):
    return lambda: synth.make_problem([PR] * n, n_frames, seed=20261020 + n, p_view=p_view,
                                      name=f"{n}-cam pinhole-radtan rig, {n_frames} frames")


# name -> (problem, C, frames per block, frames of the last block)
PROBLEMS = {
    "n6 f1027": (_rig(6, 1027, 0.7), 78, 5, 2),
    "n8 f1027": (_rig(8, 1027, 0.7), 106, 5, 2),
    "eucm6 f515": (lambda: synth.make_problem([PR, EU, PR, PR, EU, PR], 515, seed=20261020, p_view=0.8,
                                              name="6-cam pinhole-radtan + EUCM rig, 515 frames"), 74, 3, 2),
}


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
    assert p.cam_cols > 64  # the expanded partials of the fused pass
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


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_fused_gn_three_passes(capi, oracle_mod, name):
    p, _, st_o, r_o = _case(oracle_mod, name)
    assert r_o["iterations"] == 3 and r_o["failed_iterations"] == 0 and np.isfinite(st_o).all()
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


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_problems_have_the_frames_per_block_they_are_there_for(name):
    """the block geometry the cases are chosen for (k_buildp runs up to 256 blocks of equally many frames: three or
    more frames per block, a short last block) and at least one (frame, camera) view without corners"""
    p = _problem(name)
    _, _, per_block, last = PROBLEMS[name]
    assert (p.n_frames + 255) // 256 == per_block >= 3
    assert p.n_frames % per_block == last
    seen = set(zip(p.view_frame.tolist(), p.view_cam.tolist()))
    assert len(seen) < p.n_frames * p.n_cams or (np.diff(p.view_offset) == 0).any()
