"""k_buildp's 4x4x4 SYRK operand fetch against the CPU oracle, at every number of row-quad pairs a pass can issue.
The checks hold for whichever fetch the library is built with: the default six reads per pair on the 17-double row
stride, or KB_SYRK_DPP's two reads from the tile of kalibr_amd/csrc/kb_syrk_tile.h with the other four operands formed
by DPP lane rotations.

8-camera pinhole-radtan problems (configs[3]'s rig) whose views are trimmed here to 1, 8, 9, 56, 57, 64, 65, 72, 73
and 120 corners -- every count np = 1..8 of row-quad pairs a pass can issue, one- and two-pass views, the all-valid
pass -- and to none (the upload takes an empty view; the kernel forms its chain without a pass).  Two sizes: 9 frames
(one frame per block) and 257 frames at p_view 0.7 as in test_gpu_pass_heads.py (two frames per block: both
view-buffer parities, the prefetch across frames).  Once more on configs[2]'s mixed rig (omni-radtan + EUCM), the
kernel's wide two-model instantiation.

Bars, as in test_gpu_parity.py: normal-equation blocks and rhs 1e-10 of the block maximum, cost 1e-12 relative, and
after three undamped Gauss-Newton passes J_final 1e-9 relative and every state entry within 1e-6 of the oracle.  A
wrong operand (a lane offset, a rotation direction, the select side of the paired (0,2), (1,3) instruction) replaces
whole 4 x 4 blocks of a view's Hessian by other blocks, far outside these.
"""
import numpy as np
import pytest

from kalibr_amd import synth

pytestmark = pytest.mark.gpu

COUNTS = [1, 8, 9, 56, 57, 64, 65, 72, 73, 120, 0]
GN = dict(policy="gn", max_iterations=3)
_cache = {}


def _trim(p, stride):
    """views 0, stride, 2 stride, ... (the first with enough corners from there on) cut to COUNTS corners"""
    cnt = np.diff(p.view_offset).astype(int)
    keep, used, v = cnt.copy(), [], 0
    for n in COUNTS:
        while cnt[v] < n or v in used:
            v += 1
        keep[v] = n
        used.append(v)
        v += stride
    sel = np.concatenate([np.arange(p.view_offset[i], p.view_offset[i] + keep[i]) for i in range(cnt.size)])
    q = synth.Problem(
        cam_model=p.cam_model, target=p.target, view_frame=p.view_frame, view_cam=p.view_cam,
        view_offset=np.concatenate([[0], np.cumsum(keep)]).astype(np.int32),
        corner_id=p.corner_id[sel].astype(np.int32), y=p.y[sel].copy(), state_truth=p.state_truth,
        state_init=p.state_init, resolution=p.resolution, name=p.name + " (trimmed views)", meta=dict(p.meta))
    got = np.diff(q.view_offset)[used].tolist()
    assert got == COUNTS and len(set(used)) == len(COUNTS)
    # the trimmed views sit on different cameras and frames; every frame keeps full views
    assert len({int(q.view_cam[i]) for i in used}) >= 6
    return q


PROBLEMS = {
    "f9": lambda: _trim(synth.make_config(4, n_frames=9), 7),
    "f257": lambda: _trim(synth.make_config(4, n_frames=257, p_view=0.7), 131),
}


@pytest.fixture(scope="module")
def capi():
    from kalibr_amd import capi as K
    return K


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def _case(oracle_mod, name):
    """problem, the oracle's blocks at the initial state and its 3 GN passes: computed once, not modified"""
    if name not in _cache:
        p = PROBLEMS[name]()
        o = oracle_mod.Oracle(p)
        A = o.arrow(p.state_init)
        st_o, r_o = o.optimize(p.state_init, nthreads=8, **GN)
        _cache[name] = (p, A, st_o, r_o)
    return _cache[name]


def _check_build(g, p, A, tag):
    g.set_state(p.state_init)
    g.build()
    B = g.normal_blocks()
    figs = {k: _rel(B[k], A[k]) for k in ("Hff", "Hfc", "gf", "Hcc", "gc")}
    figs["rhs"] = _rel(g.rhs(), A["rhs"])
    figs["cost"] = abs(B["cost"] - A["cost"]) / A["cost"]
    print(tag, "per-call build vs oracle:", " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    for k in ("Hff", "Hfc", "gf", "Hcc", "gc", "rhs"):
        assert figs[k] < 1e-10, k
    assert figs["cost"] <= 1e-12


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_per_call_build(capi, oracle_mod, name):
    p, A, _, _ = _case(oracle_mod, name)
    g = capi.Solver(p)
    assert g.C == 106
    _check_build(g, p, A, name)
    g.close()


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_fused_gn_three_passes(capi, oracle_mod, name):
    p, _, st_o, r_o = _case(oracle_mod, name)
    assert r_o["iterations"] == 3 and r_o["failed_iterations"] == 0 and np.isfinite(st_o).all()
    g = capi.Solver(p)
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


def test_mixed_model_wide_kernel(capi, oracle_mod):
    """configs[2]'s rig, 12 frames: two projection models in one block, 9 intrinsics per omni-radtan camera"""
    p = synth.make_config(3, n_frames=12, p_view=0.8)
    A = oracle_mod.Oracle(p).arrow(p.state_init)
    g = capi.Solver(p)
    _check_build(g, p, A, "c3 f12")
    g.close()
