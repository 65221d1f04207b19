"""k_buildp's per-view table against the CPU oracle, and against the same handle with the
table forced off.

With the table a block computes each view's rigid transform T_cam_w = L_cam T_f^-1 and chain G once, one view per
lane, into LDS (kb_build_layout.h: [frames of the block][cameras] records of 49 doubles), and the view waves read them
at the top of each frame; without it (KB_BUILDP_VIEWTAB=0 at kb_create, or no room) every lane of every view wave
recomputes them per frame.  Every case asserts that the handle builds with k_buildp and carries the table, checks it
against the oracle, then repeats with the table off and holds the two device results to the same bars; whether they
are bitwise equal is printed, not asserted (chain_entry at constant indices and chain_entry_reg by 0/1 weights form
the same products, but the compiler may contract them differently).

Bars (tests/test_gpu_buildp_frames.py): normal-equation blocks and rhs 1e-10 of the block maximum, cost 1e-12
relative; after three undamped Gauss-Newton passes J_final 1e-9 relative and every state entry within 1e-6 of the
oracle's three passes, which must succeed.  Weighted handles (tests/test_gpu_robust_pipe.py): device against device
2e-10 / 2e-11 / 2e-9 / 2e-6, since each kernel carries one bar against the exact answer.

Cases (frames per block = ceil(F / (256 * blocks per CU)); a 6-wave one-model block runs two per CU):
  n8 f515     8 pinhole-radtan cameras, 515 frames, p_view 0.7: three frames per block, a short last block of 2, the
              flagship instantiation, views without corners, the expanded path (C = 106)
  n4 f301     4 cameras, 301 frames, C = 50, two frame waves, not the expanded path; two blocks per CU, so one frame
              per block: the host keeps the table off there (a one-frame block cannot earn the fill back,
              kb_build_layout.h viewtab_pays), which the case asserts; on and off are then the same launch
  n4 f601     the same rig at 601 frames: two frames per block and a last block of 1, with the table
  n4 f1540    4 cameras, 1540 frames, p_view 0.5: four frames per block on a 6-wave block at two blocks per CU
  mix4 f1540  [PR, EU, PR, EU], 1540 frames, p_view 0.5: the 8-wave instantiation runs one block per CU, so 7 frames
              per block on a 6-wave block: the prologue's "more frames than waves" loop stages poses the fill reads
  mix6 f515   [PR, EU, PR, PR, EU, PR], 515 frames: a 12-wave multi-model instantiation
"""
import numpy as np
import pytest

from kalibr_amd import synth

from . import robust_ref as R
from . import test_gpu_robust as T

pytestmark = pytest.mark.gpu

GN = dict(policy="gn", max_iterations=3)
PR, EU = synth.PINHOLE_RADTAN, synth.EUCM
BLOCKS = ("Hff", "Hfc", "gf", "Hcc", "gc")
_cache = {}

# name -> (problem, C, frames per block, frames of the last block)
PROBLEMS = {
    "n8 f515": (lambda: synth.make_problem([PR] * 8, 515, seed=20261020 + 8, p_view=0.7,
                                           name="8-cam pinhole-radtan rig, 515 frames"), 106, 3, 2),
    "n4 f301": (lambda: synth.make_problem([PR] * 4, 301, seed=20261020 + 4,
                                           name="4-cam pinhole-radtan rig, 301 frames"), 50, 1, 1),
    "n4 f601": (lambda: synth.make_problem([PR] * 4, 601, seed=20261020 + 4,
                                           name="4-cam pinhole-radtan rig, 601 frames"), 50, 2, 1),
    "n4 f1540": (lambda: synth.make_problem([PR] * 4, 1540, seed=20261020 + 4, p_view=0.5,
                                            name="4-cam pinhole-radtan rig, 1540 frames"), 50, 4, 4),
    "mix4 f1540": (lambda: synth.make_problem([PR, EU, PR, EU], 1540, seed=20261020 + 44, p_view=0.5,
                                              name="4-cam pinhole-radtan + EUCM rig, 1540 frames"), 46, 7, 7),
    "mix6 f515": (lambda: synth.make_problem([PR, EU, PR, PR, EU, PR], 515, seed=20261020, p_view=0.8,
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


def _solver(capi, monkeypatch, p, table, setup=None, pays=True):
    """a handle with the table on (the default where it fits and the block has two frames or more: `pays`) or forced
    off by the switch kb_create reads"""
    if table:
        monkeypatch.delenv("KB_BUILDP_VIEWTAB", raising=False)
    else:
        monkeypatch.setenv("KB_BUILDP_VIEWTAB", "0")
    g = capi.Solver(p)
    monkeypatch.delenv("KB_BUILDP_VIEWTAB", raising=False)
    if setup:
        setup(g)
    assert g.build_kernel_name() == "k_buildp"
    assert g.build_viewtab() is (table and pays)
    return g


def _bitwise(what, pairs):
    same = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in pairs)
    print(f"{what}: table on vs off bitwise equal: {same}")


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_problems_have_the_block_geometry_they_are_there_for(name):
    p = _problem(name)
    _, C, per_block, last = PROBLEMS[name]
    assert p.cam_cols == C
    nbz = (C + 16) // 16
    nf = 2 if (nbz * (nbz + 1) // 2 + 1) // 2 <= 5 else 4
    wide = len(set(p.cam_model.tolist() if hasattr(p.cam_model, "tolist") else p.cam_model)) >= 2 and p.n_cams + nf <= 8
    bpc = 2 if p.n_cams + nf <= 6 and not wide else 1
    gf = (p.n_frames + 256 * bpc - 1) // (256 * bpc)
    assert gf == per_block
    assert (p.n_frames - 1) % gf + 1 == last
    if name == "mix4 f1540":
        assert gf > p.n_cams + nf  # more frames than waves
    if name == "n8 f515":
        seen = set(zip(p.view_frame.tolist(), p.view_cam.tolist()))
        assert len(seen) < p.n_frames * p.n_cams or (np.diff(p.view_offset) == 0).any()


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_per_call_build(capi, oracle_mod, monkeypatch, name):
    p, A, _, _ = _case(oracle_mod, name)
    out = {}
    for table in (True, False):
        g = _solver(capi, monkeypatch, p, table, pays=PROBLEMS[name][2] >= 2)
        assert g.C == PROBLEMS[name][1]
        g.set_state(p.state_init)
        g.build()
        B = g.normal_blocks()
        out[table] = dict(B, rhs=g.rhs())
        g.close()
    for table, B in out.items():
        figs = {k: _rel(B[k], A[k]) for k in BLOCKS + ("rhs",)}
        figs["cost"] = abs(B["cost"] - A["cost"]) / A["cost"]
        print(name, "table", "on" if table else "off", "per-call build vs oracle:",
              " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        for k in BLOCKS + ("rhs",):
            assert figs[k] < 1e-10, (table, k)
        assert figs["cost"] <= 1e-12
    on, off = out[True], out[False]
    figs = {k: _rel(on[k], off[k]) for k in BLOCKS + ("rhs",)}
    print(name, "table on vs off:", " ".join(f"{k} {v:.2e}" for k, v in figs.items()), "cost", on["cost"], off["cost"])
    _bitwise(name + " per-call build", [(on[k], off[k]) for k in BLOCKS + ("rhs", "cost")])
    for k in BLOCKS + ("rhs",):
        assert figs[k] < 1e-10, k
    assert abs(on["cost"] - off["cost"]) <= 1e-12 * off["cost"]


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_fused_gn_three_passes(capi, oracle_mod, monkeypatch, name):
    p, _, st_o, r_o = _case(oracle_mod, name)
    assert r_o["iterations"] == 3 and r_o["failed_iterations"] == 0 and np.isfinite(st_o).all()
    out = {}
    for table in (True, False):
        g = _solver(capi, monkeypatch, p, table, pays=PROBLEMS[name][2] >= 2)
        g.set_state(p.state_init)
        r_g = g.optimize(**GN)
        st_g = g.get_state()
        g.set_state(p.state_init)
        g.run_gn(3)
        st_r = g.get_state()
        g.close()
        print(f"{name} table {'on' if table else 'off'}: J_final {r_g['J_final']:.15g}/{r_o['J_final']:.15g} "
              f"max|state - oracle| optimize {np.abs(st_g - st_o).max():.3e} run_gn(3) {np.abs(st_r - st_o).max():.3e}")
        assert r_g["iterations"] == 3 and r_g["failed_iterations"] == 0
        assert abs(r_g["J_final"] - r_o["J_final"]) <= 1e-9 * r_o["J_final"]
        assert np.abs(st_g - st_o).max() < 1e-6
        assert np.abs(st_r - st_o).max() < 1e-6
        out[table] = (r_g["J_final"], st_g, st_r)
    (ja, sa, ra), (jb, sb, rb) = out[True], out[False]
    print(f"{name} table on vs off: J_final {abs(ja - jb) / jb:.2e} state {np.abs(sa - sb).max():.3e} "
          f"run_gn {np.abs(ra - rb).max():.3e}")
    _bitwise(name + " three GN passes", [(sa, sb), (ra, rb), (ja, jb)])
    assert abs(ja - jb) <= 1e-9 * jb
    assert np.abs(sa - sb).max() < 1e-6 and np.abs(ra - rb).max() < 1e-6


def test_graph_equals_eager(capi, monkeypatch):
    """n8 f515: the captured passes (still three launches per pass) and the eager per-pass loop give the same bits"""
    p = _problem("n8 f515")
    st = []
    for kw in (dict(use_graph=True), dict(use_graph=False, sync_every=1)):
        g = _solver(capi, monkeypatch, p, True)
        g.set_state(p.state_init)
        r = g.optimize(**GN, **kw)
        assert r["iterations"] == 3
        g.set_state(p.state_init)
        g.run_gn(3)  # the captured fixed-count loop
        st.append((g.get_state(), r["J_final"]))
        g.close()
    assert np.isfinite(st[0][0]).all()
    assert np.array_equal(st[0][0], st[1][0]) and st[0][1] == st[1][1]


# ---------------------------------------------------------------- the weighted instantiations (WT = true)
def _weighted(capi, monkeypatch, p, table, mode="pipe"):
    def setup(g):
        g.set_robust_build(mode)
        g.set_mestimator(*T.ESTIMATORS["huber"])
        g.set_corner_invR(T.invR_of("per_corner", p.n_corners))

    if mode == "pipe":
        return _solver(capi, monkeypatch, p, table, setup)
    g = capi.Solver(p)
    setup(g)
    assert g.build_kernel_name() == "k_build" and g.build_viewtab() is False
    return g


def test_weighted_handle(capi, monkeypatch):
    """kb_set_robust_build in pipe mode on the 8-camera case, contaminated with outliers: the per-call build and the
    fused pass of the weighted k_buildp with the table, against the same without it and against the general weighted
    build (k_build<.., WT>), device against device"""
    if "pw" not in _cache:
        _cache["pw"] = R.contaminate(_problem("n8 f515"), 20261020)[0]
    p = _cache["pw"]
    out = {}
    for key, table, mode in (("on", True, "pipe"), ("off", False, "pipe"), ("general", False, "general")):
        g = _weighted(capi, monkeypatch, p, table, mode)
        g.set_state(p.state_init)
        J = g.eval_cost()
        g.build()
        B = g.normal_blocks()
        rhs = g.rhs()
        st = None
        if mode == "pipe":
            g.run_gn(3)
            st = g.get_state()
        else:
            g.optimize(policy="gn", max_iterations=3, eps_x=1e-30, eps_j=1e-30)
            st = g.get_state()
        out[key] = dict(J=J, B=B, rhs=rhs, st=st)
        g.close()
    on = out["on"]
    for other in ("off", "general"):
        b = out[other]
        figs = {k: _rel(on["B"][k], b["B"][k]) for k in BLOCKS}
        figs["rhs"] = _rel(on["rhs"], b["rhs"])
        figs["cost"] = abs(on["B"]["cost"] - b["B"]["cost"]) / b["B"]["cost"]
        figs["state"] = float(np.abs(on["st"] - b["st"]).max())
        print("weighted, table on vs", other, " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        assert on["J"] == b["J"]  # k_cost_w on every handle
        for k in BLOCKS + ("rhs",):
            assert figs[k] < 2e-10, (other, k)
        assert figs["cost"] <= 2e-11
        assert figs["state"] <= 2e-6
    _bitwise("weighted handle", [(on["B"][k], out["off"]["B"][k]) for k in BLOCKS] + [(on["st"], out["off"]["st"])])


# ---------------------------------------------------------------- the host re-decides when the frame count changes
def test_append_and_drop_across_the_fit(capi, monkeypatch):
    """configs[3]'s rig with its 120-corner target holds the table up to 12 frames per block
    (tests/test_build_layout_viewtab.py): 3072 frames.  A handle grown from 3066 to 3076 frames (13 per block) loses
    it, dropped back it has it again; before, across and after, its
    blocks and two GN passes are those of a fresh handle at the same frame count (bitwise where the fresh handle
    takes the same path, which it does: the decision depends on the frame count alone)."""
    monkeypatch.delenv("KB_BUILDP_VIEWTAB", raising=False)
    p = synth.make_config(4, n_frames=3076, p_view=0.25)
    assert p.target.shape == (120, 3) and p.n_cams == 8 and p.cam_cols == 106

    def fresh(f1):
        sub = p.frame_slice(0, f1)
        g = capi.Solver(sub)
        g.set_state(sub.state_init)
        return g, sub

    def same(a, b, what):
        a.build()
        b.build()
        A, B = a.normal_blocks(), b.normal_blocks()
        for k in BLOCKS:
            assert np.array_equal(A[k], B[k]), (what, k)
        assert A["cost"] == B["cost"], what
        a.run_gn(2)
        b.run_gn(2)
        sa, sb = a.get_state(), b.get_state()
        assert np.isfinite(sa).all() and np.array_equal(sa, sb), what

    g, _ = fresh(3066)
    assert g.build_kernel_name() == "k_buildp" and g.build_viewtab() is True
    ref, sub = fresh(3066)
    same(g, ref, "before")
    ref.close()
    g.append_frames(p.frame_slice(3066, 3076))
    assert g.build_viewtab() is False and g.build_kernel_name() == "k_buildp"
    ref, sub = fresh(3076)
    assert ref.build_viewtab() is False
    g.set_state(sub.state_init)
    same(g, ref, "across: 13 frames per block, no table")
    g.drop_last_frames(10)
    assert g.build_viewtab() is True
    ref2, sub2 = fresh(3066)
    g.set_state(sub2.state_init)
    same(g, ref2, "after")
    for h in (g, ref, ref2):
        h.close()
