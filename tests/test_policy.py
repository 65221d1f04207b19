"""The dog-leg arithmetic of kalibr_amd/csrc/kb_policy.h (the one statement the device kernels and the spline host
loops call) against the restatement in tests/dogleg_ref.py, on the CPU: tests/cpp/test_policy.cpp (g++, no HIP: that
it compiles is the check that the header is free of HIP) runs dl_start, dl_set_sd, dl_sd_branch, dl_hold_gn, dl_select
and dl_radius over one case per pass of the reference's run on c1_12, with the two settings of
tests/test_host_dogleg.py (step strings DGGG and SSSSDDDDDGGG).  Those two runs take S, G and D steps and the
delta == 0 first step, but the reference accepts every one of their passes; the rejected passes (the radius update at
rho <= 0, after a GN step and after halving, and a selection on a held system with the rejected candidate's cost) come
from a third run, tests/test_gpu_dogleg.py's test_reuse_after_rejection on c6_small (SSSDDDDDDDGGGGGG, the last four
rejected).

Every case carries the reference's numbers alone: the radius the pass starts with, the cost, and the four sums the
header's scalar form works on, gg = g.g, ghg = g^T (J^T J) g, gn2 = dx_gn.dx_gn, ggn = g.dx_gn, formed here from the
reference's own vectors with dogleg_ref._sum; the gain ratio is the one the reference's next pass finds, and
dl_radius runs on the state the header's own selection left (the previous step type of the update is that selection's,
asserted equal to the reference's).

Bound: rel 1e-12, test_host_dogleg.py's for restated arithmetic.  The header never forms dx_sd: it takes
c = dx_sd.(dx_gn - dx_sd) as s p - s^2 gg and |dx_gn - dx_sd|^2 as n - 2 s p + s^2 gg (s = sd_scale, p = ggn, n = gn2),
where the reference sums over the difference vector.  The precondition keeps the cancellation of the scalar form at a
factor 100 over a few ulp, which the bound covers; it is asserted on the reference's numbers before anything is
compared.  A run that broke it would get another delta_init, not a wider bound.
"""
import os
import subprocess

import numpy as np
import pytest

from kalibr_amd import synth

from . import dogleg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1_12 = dict(idx=1, n_frames=12)
C6_SMALL = dict(idx=6, n_frames=40, p_view=0.8)
RUNS = [(C1_12, (0.0, 1e-3, 1.0, 25), "DGGG", "1111"), (C1_12, (1e-3, 1e-9, 1e-3, 25), "SSSSDDDDDGGG", "1" * 12),
        (C6_SMALL, (1e-3, 1e-9, 1e-3, 16), "SSSDDDDDDDGGGGGG", "1111111111110000")]
REL = 1e-12
COLS = ("sd_branch", "type", "delta", "beta", "L0", "sd_scale", "sdn", "a", "b", "dx_norm", "radius")


class Recording:
    """The oracle with the vectors of the reference's run kept: per arrow() the system, per solve() the GN step and
    the system it belongs to, per apply_update() the step taken."""

    def __init__(self, oracle):
        self.o, self.systems, self.gn, self.dx = oracle, [], [], []

    def cost(self, state):
        return self.o.cost(state)

    def arrow(self, state):
        self.systems.append(self.o.arrow(state))
        return self.systems[-1]

    def solve(self, A, lam):
        assert A is self.systems[-1] and lam == 0.0
        ok, sol = self.o.solve(A, lam)
        assert ok
        self.gn.append((len(self.systems) - 1, np.array(sol, dtype=np.float64)))
        return ok, sol

    def apply_update(self, state, dx):
        self.dx.append(np.array(dx, dtype=np.float64))
        return self.o.apply_update(state, dx)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("policy")), "test_policy")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "test_policy.cpp")], check=True)
    return out


def _cases(ref, rec, delta_init):
    """one case per pass of the reference's run, none left out"""
    passes = ref["passes"]
    assert all(q["type"] >= 0 for q in passes) and len(rec.dx) == len(passes)
    cases, n_sys, n_gn = [], 0, 0
    for k, q in enumerate(passes):
        n_sys += q["built"]
        n_gn += q["solved"]
        A = rec.systems[n_sys - 1]
        g = A["rhs"]
        _, sd_scale, _, sdn = R.steepest_descent(A)
        assert sdn == q["sdn"]
        c = dict(delta=delta_init if k == 0 else q["delta"], J=passes[k - 1]["J"] if k else ref["J_start"], g=g,
                 gg=R._sum(g * g), ghg=R.g_h_g(A), sd_scale=sd_scale, have_gn=0, gn2=0.0, ggn=0.0,
                 dx_gn=np.zeros_like(g), dx=rec.dx[k], have_rho=int(k + 1 < len(passes)),
                 rho=passes[k + 1]["rho"] if k + 1 < len(passes) else 0.0)
        if k:  # past the first step the selection leaves delta alone: the recorded one is what the pass started with
            assert c["delta"] != 0
        if n_gn and rec.gn[n_gn - 1][0] == n_sys - 1:  # the reference holds the GN step of this system by now
            dx_gn = rec.gn[n_gn - 1][1]
            c.update(have_gn=1, dx_gn=dx_gn, gn2=R._sum(dx_gn * dx_gn), ggn=R._sum(g * dx_gn))
        cases.append(c)
    return cases


@pytest.fixture(scope="module")
def runs(oracle_mod, driver):
    """per setting: (the reference's run, its cases, the driver's rows)"""
    out = []
    for prob, (delta_init, eps_x, eps_j, max_it), steps, accepted in RUNS:
        p = synth.make_config(**prob)
        rec = Recording(oracle_mod.Oracle(p))
        ref = R.run(rec, p.state_init, delta_init, eps_x, eps_j, max_it)
        R.assert_not_marginal(ref)
        assert ref["steps"] == steps and ref["accepted"] == accepted
        cases = _cases(ref, rec, delta_init)
        text = "".join("%r %r %r %r %d %r %r %d %r\n" % (float(c["delta"]), float(c["J"]), c["gg"], c["ghg"], c["have_gn"],
                                                         c["gn2"], c["ggn"], c["have_rho"], float(c["rho"])) for c in cases)
        r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stderr)
        rows = [dict(zip(COLS, map(float, line.split()))) for line in r.stdout.strip().split("\n")]
        assert len(rows) == len(cases) == len(ref["passes"])  # no pass skipped
        out.append((ref, cases, rows))
    return out


def test_the_runs_cover_every_branch(runs):
    types = {q["type"] for ref, _, _ in runs for q in ref["passes"]}
    assert types == {R.SD, R.GN, R.DL}
    # rejected passes, one of them followed by a pass on the held system after each kind of step it can follow
    rejected = [(ref["passes"][k]["type"], k + 1 < len(ref["passes"])) for ref, _, _ in runs
                for k in range(len(ref["passes"])) if ref["passes"][k]["accepted"] == 0]
    assert len(rejected) == 4 and (R.GN, True) in rejected
    assert runs[0][1][0]["delta"] == 0 and runs[0][0]["passes"][0]["delta"] > 0  # the delta == 0 first step


def _assert_precondition(runs):
    """the precondition of the bound, on the reference's numbers alone"""
    n_dl = 0
    for ref, cases, _ in runs:
        for q, c in zip(ref["passes"], cases):
            if q["type"] != R.DL:
                continue
            n_dl += 1
            s, gg, p, n = c["sd_scale"], c["gg"], c["ggn"], c["gn2"]
            cc = s * p - s * s * gg
            dn2 = n - 2 * s * p + s * s * gg
            print("DL pass: |c| / (|s p| + s^2 gg) = %.3g, dn2 / (n + s^2 gg) = %.3g"
                  % (abs(cc) / (abs(s * p) + s * s * gg), dn2 / (n + s * s * gg)))
            assert abs(cc) / (abs(s * p) + s * s * gg) >= 1e-2
            assert dn2 / (n + s * s * gg) >= 1e-2
    assert n_dl == 13  # D + DDDDD + DDDDDDD


def test_the_scalar_form_is_well_conditioned_on_the_reference(runs):
    _assert_precondition(runs)


def test_header_matches_the_restatement(runs):
    _assert_precondition(runs)  # checked before any comparison
    worst = 0.0
    for ref, cases, rows in runs:
        passes = ref["passes"]
        for k, (q, c, r) in enumerate(zip(passes, cases, rows)):
            assert int(r["type"]) == q["type"], k
            assert bool(r["sd_branch"]) == (q["sdn"] >= c["delta"] and c["delta"] != 0) == (q["type"] == R.SD), k
            pairs = [(r["delta"], q["delta"]), (r["L0"], q["L0"]), (r["sd_scale"], c["sd_scale"]), (r["sdn"], q["sdn"])]
            if q["type"] == R.DL:
                pairs.append((r["beta"], q["beta"]))
            if c["have_rho"]:
                pairs.append((r["radius"], passes[k + 1]["delta"]))  # the radius the next pass starts with
            for got, want in pairs:
                worst = max(worst, abs(got - want) / abs(want))
            dx = r["a"] * c["g"] + r["b"] * c["dx_gn"]
            worst = max(worst, np.abs(dx - c["dx"]).max() / np.abs(c["dx"]).max())
    print("worst rel", worst)
    assert worst <= REL
