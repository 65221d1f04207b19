"""k_buildp's view waves at partial corner passes, and its per-block frame-view vector, against the CPU oracle.

A view lane past its view's last corner stores zero Jacobian rows, and the SYRK issues only the pairs of row quads
(8 rows) that hold a valid row: whatever form the row stores take, the rows of a partial pass that are read must be
the view's or zero, whatever the pass or the frame before left in the tile.  The cases truncate every view's corner
list so that the counts run through 1, 7, 8, 9, 56, 57, 63, 64, 65, 71, 72, 73 and 120: every remainder of 8 rows
that matters, on the first and on the second pass, next to full passes.  The view waves take each frame's corner
range from a per-lane vector loaded in the prologue (lane l: frame l of the block, reloaded every 64 frames:
kb_kernels.hip buildp_fview_lanes); the last case runs blocks of 65 frames.

Bars (tests/test_gpu_buildp_viewtab.py, test_per_call_build and test_fused_gn_three_passes): normal-equation blocks
and rhs 1e-10 of the block maximum, cost 1e-12 relative; after three undamped Gauss-Newton passes J_final 1e-9
relative and every state entry within 1e-6 of the oracle's three passes, which must succeed.

Cases (4 pinhole-radtan cameras, C = 50: a 6-wave block, two blocks per CU, so ceil(F / 512) frames per block):
  n4 f301   301 frames: one frame per block, so the host keeps the table off (kb_build_layout.h viewtab_pays)
  n4 f200   200 frames: one frame per block, table off
  n4 f601   601 frames: two frames per block and the table, also run with the table forced off: the smallest block
            in which a frame's tile holds the rows of the frame before, and the case with the table on
  weighted  n4 f301 and n4 f601 through the weighted instantiation (kb_set_robust_build pipe mode) with identity
            per-corner factors, which scale by sqrt(1) * 1 and 1 * x + 0 * y (exact): the oracle's unweighted
            system is the reference
  refresh   5 cameras (C = 64, four frame waves: one block per CU), 16,400 frames of 12 corners per view, table
            off: 65 frames per block, so frame 64 of a block comes from the refreshed vector
"""
import dataclasses

import numpy as np
import pytest

from kalibr_amd import synth

pytestmark = pytest.mark.gpu

GN = dict(policy="gn", max_iterations=3)
PR = synth.PINHOLE_RADTAN
BLOCKS = ("Hff", "Hfc", "gf", "Hcc", "gc")
COUNTS = (1, 7, 8, 9, 56, 57, 63, 64, 65, 71, 72, 73, 120)
_cache = {}


def keep_corners(p, pick):
    """p with view v's corner list reduced to its entries pick(v, available count) (an index array)"""
    off = np.asarray(p.view_offset, dtype=np.int64)
    idx = [off[v] + np.asarray(pick(v, int(off[v + 1] - off[v])), dtype=np.int64) for v in range(p.n_views)]
    counts = [len(i) for i in idx]
    sel = np.concatenate(idx)
    return dataclasses.replace(
        p, view_offset=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
        corner_id=np.ascontiguousarray(p.corner_id[sel], dtype=np.int32), y=np.ascontiguousarray(p.y[sel]))


def truncated(n_frames):
    """Every view keeps the first n corners of its list, n cycling through COUNTS by frame and camera (cameras of a
    frame differ: 3 c mod 13 is distinct for c < 13); the frame's view with the most corners, camera f mod N on a
    tie, keeps them all, so that the next frame's view of that camera is the cycle's."""
    p = synth.make_problem([PR] * 4, n_frames, seed=20261020 + 4, name=f"4-cam pinhole-radtan rig, {n_frames} frames")
    N = p.n_cams
    avail = np.diff(np.asarray(p.view_offset, dtype=np.int64))
    vf, vc = np.asarray(p.view_frame), np.asarray(p.view_cam)
    keeper = {}
    for v in range(p.n_views):
        f = int(vf[v])
        key = (int(avail[v]), -((int(vc[v]) - f) % N))
        if f not in keeper or key > keeper[f][0]:
            keeper[f] = (key, v)
    full = {v for _, v in keeper.values()}

    def pick(v, n):
        want = n if v in full else COUNTS[(5 * int(vf[v]) + 3 * int(vc[v])) % len(COUNTS)]
        return np.arange(min(n, want))

    return keep_corners(p, pick)


def refresh_problem():
    """41 frames of a 5-camera rig, 12 corners per view spread over the view's list, repeated 400 times"""
    small = synth.make_problem([PR] * 5, 41, seed=20261020 + 5, name="5-cam pinhole-radtan rig, 41 frames")
    small = keep_corners(small, lambda v, n: (np.arange(12) * n) // 12)
    rep, F = 400, small.n_frames
    so = small.n_cams * synth.MAX_INTR + synth.POSE * (small.n_cams - 1)
    cnt = np.diff(np.asarray(small.view_offset, dtype=np.int64))

    def st(s):
        return np.concatenate([s[:so]] + [s[so:]] * rep)

    return dataclasses.replace(
        small, view_frame=np.concatenate([small.view_frame + F * r for r in range(rep)]).astype(np.int32),
        view_cam=np.tile(small.view_cam, rep), corner_id=np.tile(small.corner_id, rep), y=np.tile(small.y, (rep, 1)),
        view_offset=np.concatenate([[0], np.cumsum(np.tile(cnt, rep))]).astype(np.int32),
        state_truth=st(small.state_truth), state_init=st(small.state_init), name="5-cam rig, 16400 frames of 12 corners")


PROBLEMS = {"n4 f301": (lambda: truncated(301), 1), "n4 f200": (lambda: truncated(200), 1),
            "n4 f601": (lambda: truncated(601), 2)}


@pytest.fixture(scope="module")
def capi():
    from kalibr_amd import capi as K
    return K


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


def _problem(name):
    if ("p", name) not in _cache:
        _cache["p", name] = refresh_problem() if name == "refresh" else PROBLEMS[name][0]()
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


def _frames_per_block(p):
    nbz = (p.cam_cols + 16) // 16
    nf = 2 if (nbz * (nbz + 1) // 2 + 1) // 2 <= 5 else 4
    bpc = 2 if p.n_cams + nf <= 6 else 1
    return (p.n_frames + 256 * bpc - 1) // (256 * bpc)


def _solver(capi, monkeypatch, p, table, weighted=False):
    if table:
        monkeypatch.delenv("KB_BUILDP_VIEWTAB", raising=False)
    else:
        monkeypatch.setenv("KB_BUILDP_VIEWTAB", "0")
    g = capi.Solver(p)
    monkeypatch.delenv("KB_BUILDP_VIEWTAB", raising=False)
    if weighted:
        g.set_robust_build("pipe")
        g.set_corner_invR(np.tile([1.0, 0.0, 1.0], (p.n_corners, 1)))
    assert g.build_kernel_name() == "k_buildp"
    assert g.build_viewtab() is (table and _frames_per_block(p) >= 2)
    return g


# (problem, table asked for, weighted handle)
HANDLES = [("n4 f301", True, False), ("n4 f200", False, False), ("n4 f601", True, False), ("n4 f601", False, False),
           ("n4 f301", True, True), ("n4 f601", True, True)]
IDS = [f"{n} table {'on' if t else 'off'}{' weighted' if w else ''}" for n, t, w in HANDLES]


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_problems_have_the_shapes_they_are_there_for(oracle_mod, name):
    p, _, st_o, r_o = _case(oracle_mod, name)
    assert p.n_cams == 4 and p.cam_cols == 50 and _frames_per_block(p) == PROBLEMS[name][1]
    n = np.diff(np.asarray(p.view_offset, dtype=np.int64))
    vf, vc = np.asarray(p.view_frame), np.asarray(p.view_cam)
    assert set(COUNTS) <= set(n.tolist())
    assert ((n >= 65) & (n <= 71)).any()  # 1 .. 7 valid rows in the second pass, the first pass's rows under them
    best = np.zeros(p.n_frames, dtype=np.int64)
    np.maximum.at(best, vf, n)
    assert best.min() >= 56  # every frame's 6 x 6 block stays positive definite ...
    assert r_o["iterations"] == 3 and r_o["failed_iterations"] == 0 and np.isfinite(st_o).all()  # ... for the oracle
    cnt = -np.ones((p.n_frames, p.n_cams), dtype=np.int64)
    cnt[vf, vc] = n
    for f in range(p.n_frames):  # the cameras of a frame differ (two of the four may both have kept all they saw)
        assert len(set(cnt[f].tolist())) >= 3, (f, cnt[f])
    gf = _frames_per_block(p)
    if gf >= 2:  # a short view behind a 120-corner view of its camera, inside one block
        f = np.arange(p.n_frames - 1)
        f = f[f % gf != gf - 1]
        stale = (cnt[f] == 120) & (cnt[f + 1] >= 0) & (cnt[f + 1] < 56)
        print(name, "short views behind a full view of the same camera in the same block:", int(stale.sum()))
        assert stale.sum() >= 8


@pytest.mark.parametrize("name,table,weighted", HANDLES, ids=IDS)
def test_per_call_build(capi, oracle_mod, monkeypatch, name, table, weighted):
    p, A, _, _ = _case(oracle_mod, name)
    g = _solver(capi, monkeypatch, p, table, weighted)
    g.set_state(p.state_init)
    g.build()
    B = g.normal_blocks()
    figs = {k: _rel(B[k], A[k]) for k in BLOCKS}
    figs["rhs"] = _rel(g.rhs(), A["rhs"])
    figs["cost"] = abs(B["cost"] - A["cost"]) / A["cost"]
    g.close()
    print(name, table, weighted, "per-call build vs oracle:", " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    for k in BLOCKS + ("rhs",):
        assert figs[k] < 1e-10, k
    assert figs["cost"] <= 1e-12


@pytest.mark.parametrize("name,table,weighted", HANDLES, ids=IDS)
def test_fused_gn_three_passes(capi, oracle_mod, monkeypatch, name, table, weighted):
    p, _, st_o, r_o = _case(oracle_mod, name)
    assert r_o["iterations"] == 3 and r_o["failed_iterations"] == 0 and np.isfinite(st_o).all()
    g = _solver(capi, monkeypatch, p, table, weighted)
    g.set_state(p.state_init)
    r_g = g.optimize(**GN)
    st_g = g.get_state()
    g.set_state(p.state_init)
    g.run_gn(3)
    st_r = g.get_state()
    g.close()
    print(f"{name} {table} {weighted}: J_final {r_g['J_final']:.15g}/{r_o['J_final']:.15g} "
          f"max|state - oracle| optimize {np.abs(st_g - st_o).max():.3e} run_gn(3) {np.abs(st_r - st_o).max():.3e}")
    assert r_g["iterations"] == 3 and r_g["failed_iterations"] == 0
    assert abs(r_g["J_final"] - r_o["J_final"]) <= 1e-9 * r_o["J_final"]
    assert np.abs(st_g - st_o).max() < 1e-6
    assert np.abs(st_r - st_o).max() < 1e-6


def test_blocks_of_more_than_64_frames(capi, oracle_mod, monkeypatch):
    p = _problem("refresh")
    assert p.n_frames == 16400 and p.cam_cols == 64 and _frames_per_block(p) == 65
    assert (np.diff(p.view_offset) == 12).all()
    A = oracle_mod.Oracle(p).arrow(p.state_init, nthreads=8)
    g = _solver(capi, monkeypatch, p, False)
    g.set_state(p.state_init)
    g.build()
    B = g.normal_blocks()
    figs = {k: _rel(B[k], A[k]) for k in BLOCKS}
    figs["rhs"] = _rel(g.rhs(), A["rhs"])
    figs["cost"] = abs(B["cost"] - A["cost"]) / A["cost"]
    g.close()
    print("65 frames per block, per-call build vs oracle:", " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    # per frame as well: a wrong corner range in one frame of 16,400 must not hide under the largest block
    for k in ("Hff", "Hfc", "gf"):
        a, b = np.asarray(A[k]).reshape(p.n_frames, -1), np.asarray(B[k]).reshape(p.n_frames, -1)
        worst = float((np.abs(a - b).max(axis=1) / np.abs(a).max(axis=1)).max())
        print(k, "worst frame", worst)
        assert worst < 1e-10, k
    for k in BLOCKS + ("rhs",):
        assert figs[k] < 1e-10, k
    assert figs["cost"] <= 1e-12
