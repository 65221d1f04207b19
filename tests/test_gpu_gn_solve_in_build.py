"""The fused Gauss-Newton pass in two launches: the camera solve of pass i at the head of pass i + 1's k_buildp
(k_buildp<.., SIB = true>), against the same handle type with the switch off (KB_GN_SOLVE_IN_BUILD=0 at
kb_create: three launches per pass) and against the CPU oracle.

Every block of the fused kernel stages the k_solve image and runs solve_body<0> itself, with the instructions of
k_solve<0>'s solve on the same operands, so the expectation is bitwise: state (camera and frame part), the chains of
both slots (kb_debug_chains), the cost trace and the iteration count.  The frame poses are the witness that every
block's copy of dx_c agrees: each block steps its own frames with its own copy.  (dx itself has no getter in the
C-ABI for the loop's last step; the camera part of the state is state + dx_c and the chains are functions of it.)

Shapes (pinhole-radtan rigs, the flagship's instantiation family):
  n8 f16    8 cameras x 16 frames: one-frame blocks, the table-less instantiation, C = 106
  n8 f520   8 cameras x 520 frames: three frames per block, the last block one frame, the per-view table
  n6 f24    6 cameras x 24 frames: C = 78, five panels, ten waves (waves 8 and 9 take the solve's barriers, no role)
"""
import dataclasses
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from kalibr_amd import synth

from . import test_gpu_robust as T

pytestmark = pytest.mark.gpu

PR = synth.PINHOLE_RADTAN
SEED = 20261021
# name -> (problem, C, frames per block, frames of the last block, carries the per-view table)
PROBLEMS = {
    "n8 f16": (lambda: synth.make_problem([PR] * 8, 16, seed=SEED + 8, name="8-cam pinhole-radtan rig, 16 frames"),
               106, 1, 1, False),
    "n8 f520": (lambda: synth.make_problem([PR] * 8, 520, seed=SEED + 8, p_view=0.7,
                                           name="8-cam pinhole-radtan rig, 520 frames"), 106, 3, 1, True),
    "n6 f24": (lambda: synth.make_problem([PR] * 6, 24, seed=SEED + 6, name="6-cam pinhole-radtan rig, 24 frames"),
               78, 1, 1, False),
}
PASSES = (1, 2, 7, 8, 9, 17)
_cache = {}


@pytest.fixture(scope="module")
def capi():
    from kalibr_amd import capi as K
    return K


def _problem(name):
    if ("p", name) not in _cache:
        _cache["p", name] = PROBLEMS[name][0]()
    return _cache["p", name]


def _solver(capi, monkeypatch, p, on):
    """a handle on the two-launch path (the default where the handle takes it) or with the switch kb_create reads off"""
    if on:
        monkeypatch.delenv("KB_GN_SOLVE_IN_BUILD", raising=False)
    else:
        monkeypatch.setenv("KB_GN_SOLVE_IN_BUILD", "0")
    g = capi.Solver(p)
    monkeypatch.delenv("KB_GN_SOLVE_IN_BUILD", raising=False)
    assert g.build_kernel_name() == "k_buildp"
    assert g.gn_solve_in_build() is on
    return g


def _pair(capi, monkeypatch, name):
    """the on and the off handle of a shape, created once for the module"""
    if ("g", name) not in _cache:
        p = _problem(name)
        _cache["g", name] = (_solver(capi, monkeypatch, p, True), _solver(capi, monkeypatch, p, False))
    return _cache["g", name]


def _trace(capi, g, cap=64):
    tr = np.zeros((cap, 4))
    n = capi._check(capi.lib().kb_get_trace(g.h, capi._d(tr), cap))
    return tr[:n].copy()


def _snapshot(capi, g):
    L0, K0 = g.debug_chains(0)
    L1, K1 = g.debug_chains(1)
    return dict(state=g.get_state(), L0=L0, K0=K0, L1=L1, K1=K1, trace=_trace(capi, g))


def _same(a, b, what, finite=True):
    for k in a:
        assert not finite or np.isfinite(a[k]).all(), (what, k)
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_problems_have_the_geometry_they_are_there_for(capi, monkeypatch, name):
    p = _problem(name)
    _, C, per_block, last, table = PROBLEMS[name]
    assert p.cam_cols == C and C > 64
    gf = (p.n_frames + 255) // 256
    assert gf == per_block and (p.n_frames - 1) % gf + 1 == last
    on, off = _pair(capi, monkeypatch, name)
    assert on.build_viewtab() is table and off.build_viewtab() is table


@pytest.mark.parametrize("n", PASSES)
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_passes_are_bitwise_those_of_three_launches(capi, monkeypatch, name, n):
    p = _problem(name)
    on, off = _pair(capi, monkeypatch, name)
    out = []
    for g in (on, off):
        g.set_state(p.state_init)
        g.run_gn(n)  # fails unless ctrl.iterations == n
        out.append(_snapshot(capi, g))
    assert len(out[0]["trace"]) == n
    so = p.n_cams * synth.MAX_INTR + 7 * (p.n_cams - 1)
    assert not np.array_equal(out[0]["state"][:so], p.state_init[:so])      # the cameras moved
    assert not np.array_equal(out[0]["state"][so:], p.state_init[so:])      # and every block's frames
    _same(out[0], out[1], (name, n))


def test_eager_batches_are_bitwise_the_graphs(capi, monkeypatch):
    """optimize without graphs enqueues the same two-launch batches eagerly"""
    name = "n8 f520"
    p = _problem(name)
    on, off = _pair(capi, monkeypatch, name)
    res = []
    for g, kw in ((on, dict(use_graph=False)), (on, dict(use_graph=True)), (off, dict(use_graph=True))):
        g.set_state(p.state_init)
        r = g.optimize(policy="gn", max_iterations=5, eps_x=1e-30, eps_j=1e-30, sync_every=5, **kw)
        res.append((r, _snapshot(capi, g)))
    for r, s in res[1:]:
        assert r["iterations"] == res[0][0]["iterations"] == 5 and r["J_final"] == res[0][0]["J_final"]
        _same(res[0][1], s, "eager vs graph")


def test_convergence_inside_a_captured_graph(capi, monkeypatch):
    """a step threshold between the step sizes of passes 2 and 3, so the loop ends at pass 3 of an 8-pass graph: the
    fused kernels of passes 4..8 find the loop done (at their solve's finish_prev, then at entry) and change nothing"""
    name = "n8 f16"
    p = _problem(name)
    on, off = _pair(capi, monkeypatch, name)
    off.set_state(p.state_init)
    r = off.optimize(policy="gn", max_iterations=8, eps_x=1e-30, eps_j=1e-30, sync_every=8)
    dX = r["trace"][:, 2]
    assert r["iterations"] == 8 and dX[0] > dX[1] > dX[2] > 0.0
    eps_x = float(np.sqrt(dX[1] * dX[2]))
    out = []
    for g in (on, off):
        g.set_state(p.state_init)
        r = g.optimize(policy="gn", max_iterations=8, eps_x=eps_x, eps_j=1e-30, sync_every=8, use_graph=True)
        out.append((r, _snapshot(capi, g)))
    (ra, sa), (rb, sb) = out
    print("converged:", {k: ra[k] for k in ra if k != "trace"})
    assert ra["iterations"] == rb["iterations"] == 3 and len(ra["trace"]) == 3
    for k in ra:  # (bytes: a failed pass's trace row carries a NaN cost)
        assert np.asarray(ra[k]).tobytes() == np.asarray(rb[k]).tobytes(), k
    _same(sa, sb, "converged at pass 3 of 8")


def _blind_camera(p, cam):
    """problem in which camera `cam` sees no corner (its views stay, empty): its intrinsic and baseline columns of the
    camera block are zero, so the undamped camera system is rank deficient"""
    o = p.view_offset
    keep = np.array([0 if c == cam else o[v + 1] - o[v] for v, c in enumerate(p.view_cam.tolist())])
    idx = np.concatenate([np.arange(o[v], o[v] + keep[v]) for v in range(p.n_views)])
    return dataclasses.replace(p, corner_id=p.corner_id[idx].astype(np.int32), y=p.y[idx].copy(),
                               view_offset=np.concatenate([[0], np.cumsum(keep)]).astype(np.int32))


def test_non_positive_pivot_ends_the_pass_as_three_launches_do(capi, monkeypatch):
    """GN (lambda = 0) on a rank-deficient camera block: the solve at the head of pass 2's build meets the zero pivot.
    solve_ok, the failed-iteration bookkeeping, the trace and the state are those of the switch-off run"""
    p = _blind_camera(_problem("n8 f16"), 7)
    out = []
    for on in (True, False):
        g = _solver(capi, monkeypatch, p, on)
        g.set_state(p.state_init)
        r = g.optimize(policy="gn", max_iterations=4, eps_x=1e-30, eps_j=1e-30, sync_every=4, use_graph=True)
        out.append((r, _snapshot(capi, g)))
        g.close()
    (ra, sa), (rb, sb) = out
    print("rank-deficient:", {k: rb[k] for k in rb if k != "trace"})
    assert rb["failed_iterations"] >= 1  # the case is what it is there for
    for k in ra:  # (bytes: a failed pass's trace row carries a NaN cost)
        assert np.asarray(ra[k]).tobytes() == np.asarray(rb[k]).tobytes(), k
    _same(sa, sb, "non-positive pivot", finite=False)


def test_handle_state_after_fused_passes(capi, monkeypatch):
    """after fused passes the HBM copies that only block 0 wrote are complete: the per-call build and solve, the
    covariance and an LM optimize on the same handle give what they give after switch-off passes"""
    name = "n8 f16"
    p = _problem(name)
    on, off = _pair(capi, monkeypatch, name)
    out = []
    for g in (on, off):
        g.set_state(p.state_init)
        g.run_gn(3)
        g.build()
        B = g.normal_blocks()
        g.set_constant_conditioner(1.0)
        ok, dx = g.solve()
        assert ok
        cok, cov = g.covariance(cross=True)
        assert cok
        r = g.optimize(policy="lm", lambda0=10.0, max_iterations=4, eps_x=1e-30, eps_j=1e-30)
        out.append(dict({k: np.asarray(v) for k, v in B.items()}, dx=dx, lm_state=g.get_state(), lm_trace=r["trace"],
                        **cov))
    _same(out[0], out[1], "handle state after fused passes")


def test_sharded_and_weighted_handles_keep_three_launches(capi, monkeypatch):
    monkeypatch.delenv("KB_GN_SOLVE_IN_BUILD", raising=False)
    p = _problem("n8 f16")
    # a weighted handle (pipe mode has the fused GN pass): the query says 0 and the passes are the parent's
    ref = []
    for env in (None, "0"):
        if env is not None:
            monkeypatch.setenv("KB_GN_SOLVE_IN_BUILD", env)
        g = capi.Solver(p)
        monkeypatch.delenv("KB_GN_SOLVE_IN_BUILD", raising=False)
        g.set_robust_build("pipe")
        g.set_mestimator(*T.ESTIMATORS["huber"])
        assert g.gn_solve_in_build() is False
        g.set_state(p.state_init)
        g.run_gn(3)
        ref.append(_snapshot(capi, g))
        g.set_mestimator("none")  # unweighted again: the path comes back with the kernels
        assert g.gn_solve_in_build() is (env is None)
        g.close()
    _same(ref[0], ref[1], "weighted")
    # a sharded in-process group: 0 on every rank, and the ranks' states are those with the switch off
    states = []
    for env in (None, "0"):
        if env is not None:
            monkeypatch.setenv("KB_GN_SOLVE_IN_BUILD", env)
        subs = [p.frame_slice(0, 7), p.frame_slice(7, p.n_frames)]
        solvers = [capi.Solver(s) for s in subs]
        monkeypatch.delenv("KB_GN_SOLVE_IN_BUILD", raising=False)
        capi.comm_init_local(solvers)
        for s, sub in zip(solvers, subs):
            assert s.gn_solve_in_build() is False
            s.set_state(sub.state_init)
        with ThreadPoolExecutor(max_workers=2) as ex:
            futs = [ex.submit(lambda s: s.optimize(policy="gn", max_iterations=3, eps_x=1e-30, eps_j=1e-30), s)
                    for s in solvers]
            rs = [f.result(timeout=300) for f in futs]
        assert all(r["iterations"] == 3 for r in rs)
        states.append([s.get_state() for s in solvers])
        for s in solvers:
            s.close()
    for a, b in zip(*states):
        assert np.isfinite(a).all() and np.array_equal(a, b)


def test_against_the_oracle(capi, oracle_mod, monkeypatch):
    """GN on the 8 x 16 rig through the two-launch passes, against the CPU oracle at the bars of
    tests/test_gpu_fullsize.py: J_final 1e-9 relative, intrinsics, baselines and every frame pose within 1e-6"""
    name = "n8 f16"
    p = _problem(name)
    on, _ = _pair(capi, monkeypatch, name)
    kw = dict(policy="gn", max_iterations=20, eps_x=1e-3, eps_j=1.0)
    st_o, r_o = oracle_mod.Oracle(p).optimize(p.state_init, nthreads=8, **kw)
    on.set_state(p.state_init)
    r_g = on.optimize(**kw)
    st_g = on.get_state()
    so = p.n_cams * synth.MAX_INTR + 7 * (p.n_cams - 1)
    print(f"J_final {r_g['J_final']:.15g}/{r_o['J_final']:.15g} iterations {r_g['iterations']}/{r_o['iterations']} "
          f"cal {np.abs(st_g[:so] - st_o[:so]).max():.3e} all {np.abs(st_g - st_o).max():.3e}")
    assert r_g["iterations"] == r_o["iterations"] and r_g["iterations"] >= 2  # at least one fused kernel ran
    assert abs(r_g["J_final"] - r_o["J_final"]) <= 1e-9 * r_o["J_final"]
    assert np.abs(st_g[:so] - st_o[:so]).max() < 1e-6
    assert np.abs(st_g - st_o).max() < 1e-6


def test_close_the_module_handles():
    for k in [k for k in _cache if k[0] == "g"]:
        for g in _cache.pop(k):
            g.close()
