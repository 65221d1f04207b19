"""The one-model rigs of the six camera models that no other module launches -- omni-radtan, EUCM, omni, double-sphere,
pinhole-equidistant, pinhole-FOV -- and the crafted states that reach the limit branches of the device maths: shared by
test_model_set_cases.py (the preconditions, from synth and the oracle alone) and test_gpu_model_sets.py (the device
against the oracle).

A rig of one camera model gets the build kernels of that model's own translation unit (kb_build_tu.hip, KB_TU_ID
1 .. 6): the intrinsic count is a compile-time constant there (9 | 6 | 5 | 6 | 8 | 5), which drops operand columns and
fixes `model` inside project / project_jac.  Every rig is synth.make_problem([m] * N, F, seed=20261101 + m, p_view)
with synth's default intrinsics; the table records what a rig is there to reach (C, the build kernel), and
test_model_set_cases.py asserts C, so a change to synth cannot move a rig to another kernel unnoticed.

  x1   N = 1, F = 12: k_build<1>, four waves on one camera, C = 5 .. 9
  x4   N = 4, F = 24: k_buildp<5, .., 12>, two blocks per CU, non-expanded partials, C = 38 .. 54
  x8   N = 8, F = 16: k_buildp<7, .., 12>, four frame waves, expanded partials in the fused pass (C > 64),
       C = 82 .. 106; omni-radtan takes N = 7 (C = 99: 8 * 9 + 42 > 111, the widest camera block)
  double-sphere takes F = 60 (x4) and F = 40 (x8): at 24 and 16 frames the oracle's own three Gauss-Newton passes move
  by 2e-5 and 5e-7 with the summation order, so it could not referee the 1e-6 state bar (GN_SPREAD_MAX below)
  large  FOV, EUCM, omni-radtan (5, 6, 9 intrinsics): x4 f515 at p_view 0.7 (two frames per block at two blocks per
       CU, a last block of one) and x8 f257 / x7 f257 (two frames per block at one block per CU, a last block of one)
"""
import functools
from dataclasses import dataclass

import numpy as np

from kalibr_amd import synth

OR, EU, OM, DS, EQ, FV = (synth.OMNI_RADTAN, synth.EUCM, synth.OMNI, synth.DS, synth.PINHOLE_EQUI,
                          synth.PINHOLE_FOV)
MODELS = (OR, EU, OM, DS, EQ, FV)
SEED = 20261101
GN = dict(policy="gn", max_iterations=3)
# A rig takes the three-pass Gauss-Newton comparison only if the oracle's own three passes, summed by 1 thread and by
# 8, agree to this in every state entry: 100 times below the 1e-6 bar on the device's state, so the reference's
# sensitivity to summation order cannot decide the test (test_model_set_cases.py asserts it for every admitted rig)
GN_SPREAD_MAX = 1e-8
FLOOR_MAX = 1e-9  # the oracle's Schur solve against its dense solve at lambda = 10, relative to max|dx|


@dataclass(frozen=True)
class Rig:
    name: str
    model: int
    n: int           # cameras
    n_frames: int
    C: int           # camera columns
    kernel: str      # what build_kernel_name() reports on a fresh handle
    p_view: float = 0.8
    gframes: int = 1  # frames per build block


def _rigs():
    small, large = [], []
    for m in MODELS:
        nm, ni = synth.MODEL_NAMES[m], synth.NINTR[m]
        n8 = 7 if m == OR else 8
        small += [Rig(f"{nm} x1", m, 1, 12, ni, "k_build"),
                  Rig(f"{nm} x4", m, 4, 60 if m == DS else 24, 4 * ni + 18, "k_buildp"),
                  Rig(f"{nm} x{n8}", m, n8, 40 if m == DS else 16, n8 * ni + 6 * (n8 - 1), "k_buildp")]
    for m in (FV, EU, OR):
        nm, ni = synth.MODEL_NAMES[m], synth.NINTR[m]
        n8 = 7 if m == OR else 8
        large += [Rig(f"{nm} x4 f515", m, 4, 515, 4 * ni + 18, "k_buildp", 0.7, 2),
                  Rig(f"{nm} x{n8} f257", m, n8, 257, n8 * ni + 6 * (n8 - 1), "k_buildp", 0.8, 2)]
    return small, large


_SMALL, _LARGE = _rigs()
RIGS = {r.name: r for r in _SMALL + _LARGE}
SMALL = [r.name for r in _SMALL]                      # the 18 rigs of the per-call check
LARGE = [r.name for r in _LARGE]                      # frames per block and the per-view table
PIPED = [r.name for r in _SMALL if r.n > 1]           # the 12 rigs that pipeline: also run with k_build
X4 = [r.name for r in _SMALL if r.n == 4]             # the weighted instantiations
# the camera-block widths the table is there for (asserted by test_model_set_cases.py)
C_X1, C_X4, C_X8 = (5, 5, 6, 6, 8, 9), (38, 38, 42, 42, 50, 54), (82, 82, 90, 90, 99, 106)

# Undamped Gauss-Newton is not defined on a rig of omni-radtan cameras (tests/test_gpu_buildp_tail.py): the oracle's
# own passes take one accepted step and three failed ones from the initial state and from the truth alike.  Measured
# with the oracle, 1 thread against 8 (max over the state after three passes):
#   omni-radtan x1 / x4 / x7 / x4 f515 / x7 f257   2 + 3 failed or 1 + 3 failed iterations: not defined
#   ds x1                                          8.8e-06: above GN_SPREAD_MAX, left out
#   eucm, omni, pinhole-equi, pinhole-fov x1       1.1e-13 .. 2.3e-13
#   eucm, omni, pinhole-equi, pinhole-fov x4, x8   1.7e-13 .. 2.1e-11
#   ds x4 (60 frames), ds x8 (40 frames)           5.2e-09, 4.4e-09
#   pinhole-fov x4 f515, x8 f257                   8.0e-13, 2.6e-11
#   eucm x4 f515, x8 f257                          1.1e-13, 4.5e-13
# The list is written out, not computed, so that it cannot shrink silently.
GN_ADMITTED = (
    "eucm x1", "eucm x4", "eucm x8",
    "omni x1", "omni x4", "omni x8",
    "ds x4", "ds x8",
    "pinhole-equi x1", "pinhole-equi x4", "pinhole-equi x8",
    "pinhole-fov x1", "pinhole-fov x4", "pinhole-fov x8",
    "pinhole-fov x4 f515", "pinhole-fov x8 f257", "eucm x4 f515", "eucm x8 f257",
)
GN_LEFT_OUT = {
    "omni-radtan x1": "undamped GN not defined", "omni-radtan x4": "undamped GN not defined",
    "omni-radtan x7": "undamped GN not defined", "omni-radtan x4 f515": "undamped GN not defined",
    "omni-radtan x7 f257": "undamped GN not defined", "ds x1": "oracle spread 8.8e-06 > 1e-8",
}


@functools.lru_cache(maxsize=None)
def problem(name):
    r = RIGS[name]
    return synth.make_problem([r.model] * r.n, r.n_frames, seed=SEED + r.model, p_view=r.p_view, name=name)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


class Ref:
    """The oracle's side of a rig, each part computed once per process and not modified: the blocks and the
    lambda = 10 solve at state_init and state_truth, and the three Gauss-Newton passes."""

    def __init__(self, name):
        from oracle import oracle as O
        self.p = problem(name)
        self.o = O.Oracle(self.p)
        self._arrow, self._solve, self._gn = {}, {}, {}

    def state(self, which):
        return self.p.state_init if which == "init" else self.p.state_truth

    def arrow(self, which):
        if which not in self._arrow:
            self._arrow[which] = self.o.arrow(self.state(which), nthreads=8)
        return self._arrow[which]

    def solve(self, which, dense=False):
        """(ok, dx) of the oracle's Schur (or dense) solve at lambda = 10"""
        if (which, dense) not in self._solve:
            self._solve[which, dense] = self.o.solve(self.arrow(which), 10.0, dense=dense)
        return self._solve[which, dense]

    def gn(self, nthreads=8):
        """(state, result) of the oracle's three undamped Gauss-Newton passes from state_init"""
        if nthreads not in self._gn:
            self._gn[nthreads] = self.o.optimize(self.p.state_init, nthreads=nthreads, **GN)
        return self._gn[nthreads]


@functools.lru_cache(maxsize=None)
def ref(name):
    return Ref(name)


# ---- the branch edges of the device maths (kb_math.h) ----
# (ex, ey): the normalised coordinates x / z, y / z a crafted corner is moved to.  Every r^2 stays a factor 2 or more
# from FOV's limit r^2 < 1e-5 and every r a factor 2 or more from the equidistant limit r <= 1e-8, so the device and the
# oracle cannot fall on different sides of a threshold by rounding.  r = 0 exactly is left out: the equidistant
# Jacobian is 0 / 0 there in the reference, the oracle and the device alike.
EDGE_POINTS = (
    (1e-3, -2e-3),   # r^2 = 5e-6: inside FOV's limit (constant scale, constant w column in both rows)
    (4e-3, 3e-3),    # r^2 = 2.5e-5: outside it
    (1e-9, 2e-9),    # r^2 = 5e-18, r = 2.2e-9: inside the equidistant limit (scale 1)
    (1e-6, -1e-6),   # r^2 = 2e-12, r = 1.4e-6: outside it
)
# rig -> ((camera whose view is crafted, first of its four frames), ...).  In configs 6 ([DS, EQ, FV, OM]: the
# all-models instantiation, which tells equidistant from FOV at run time) camera 0 is a double-sphere, which has none
# of these branches, so there the equidistant camera takes frames 0 .. 3 and the FOV camera frames 4 .. 7.
EDGE_RIGS = {
    "fov x4": ((0, 0),),
    "equi x4": ((0, 0),),
    "c6": ((1, 0), (2, 4)),
}
# FOV's w^2 < 1e-5 limit (identity, zero w column): w per FOV camera, w^2 = 1e-6 and 9e-6.  configs 6 has one FOV
# camera (2), which takes each value in a state of its own
SMALL_W = {
    "fov x4": ({0: 1e-3, 1: 3e-3},),
    "c6": ({2: 1e-3}, {2: 3e-3}),
}


@functools.lru_cache(maxsize=None)
def edge_problem(name):
    if name == "fov x4":
        return synth.make_problem([FV] * 4, 24, seed=SEED + FV, p_view=1.0, name="pinhole-fov x4, every view")
    if name == "equi x4":
        return synth.make_problem([EQ] * 4, 24, seed=SEED + EQ, p_view=1.0, name="pinhole-equi x4, every view")
    assert name == "c6"
    return synth.make_config(6, n_frames=24)


def _cam_from_c0(p, state, cam):
    """T_{cam, c0} at `state`: the chain of baselines B_{cam-1} .. B_0"""
    T = np.eye(4)
    for j in range(cam):
        o = p.n_cams * synth.MAX_INTR + synth.POSE * j
        T = synth.pose_to_T(state[o: o + synth.POSE]) @ T
    return T


def _frame_offset(p, f):
    return p.n_cams * synth.MAX_INTR + synth.POSE * (p.n_cams - 1) + synth.POSE * f


def first_corner(p, f, cam):
    """the target point of the first corner of the view (f, cam)"""
    v = int(np.nonzero((p.view_frame == f) & (p.view_cam == cam))[0][0])
    return p.target[int(p.corner_id[int(p.view_offset[v])])]


def normalised(p, state, f, cam, P):
    """(x / z, y / z, z) of the target point P seen by `cam` in frame f at `state` (numpy, synth's conventions:
    p_c0 = T_f^-1 P, p_cam = T_{cam, c0} p_c0)"""
    o = _frame_offset(p, f)
    Tf = synth.pose_to_T(state[o: o + synth.POSE])
    pc = _cam_from_c0(p, state, cam) @ synth.inv_T(Tf) @ np.append(P, 1.0)
    return pc[0] / pc[2], pc[1] / pc[2], pc[2]


def edge_state(name):
    """state_init with the translations of the crafted frames moved so that the first corner of the crafted camera's
    view sits at EDGE_POINTS, at its current depth z: with the frame pose (R, t) and T_{cam, c0} = (Rc, tc),
    t' = P - R Rc^T ((ex z, ey z, z) - tc)"""
    p = edge_problem(name)
    st = p.state_init.copy()
    for cam, f0 in EDGE_RIGS[name]:
        Tc = _cam_from_c0(p, st, cam)
        for k, (ex, ey) in enumerate(EDGE_POINTS):
            f = f0 + k
            P = first_corner(p, f, cam)
            z = normalised(p, st, f, cam, P)[2]
            o = _frame_offset(p, f)
            R = synth.quat2r(st[o: o + 4])
            st[o + 4: o + 7] = P - R @ (Tc[:3, :3].T @ (np.array([ex * z, ey * z, z]) - Tc[:3, 3]))
    return st


def w_column(p, cam):
    """the camera column of FOV camera cam's w (its fifth intrinsic)"""
    return int(sum(synth.NINTR[int(m)] for m in p.cam_model[:cam])) + 4


def small_w_states(name):
    """[(state, {camera: w})]: state_init with FOV's w set below the w^2 < 1e-5 limit"""
    p = edge_problem(name)
    out = []
    for ws in SMALL_W[name]:
        st = p.state_init.copy()
        for cam, w in ws.items():
            assert int(p.cam_model[cam]) == FV
            st[cam * synth.MAX_INTR + 4] = w
        out.append((st, ws))
    return out


# update_pose's series branch (theta < 2^-13): rotation steps of these norms on the first frames (and, where there is
# one, the first baseline); 0 exactly, well inside, and either side of 2^-13 = 1.2207e-4
ROT_NORMS = (0.0, 1e-5, 1.0e-4, 1.5e-4)


def pose_steps(p, seed=3):
    """a step of test_update_revert's size (normal, 1e-3) whose rotation parts on frames 0 .. 3 and 4 .. 7 have the
    norms ROT_NORMS (two directions each) and on baseline k the norm ROT_NORMS[k]"""
    rng = np.random.default_rng(seed)
    dx = rng.normal(scale=1e-3, size=p.total_cols)
    C = p.cam_cols

    def put(col, norm):
        a = rng.normal(size=3)
        dx[col: col + 3] = norm * a / np.linalg.norm(a)

    for k in range(8):
        put(C + 6 * k, ROT_NORMS[k % 4])
    for j in range(min(p.n_cams - 1, 4)):
        put(C - 6 * (p.n_cams - 1) + 6 * j, ROT_NORMS[j])
    return dx
