"""The solve window of k_buildp's solve-at-the-head instantiations in the launch layout
(kalibr_amd/csrc/kb_build_layout.h: solve_carve, solve_window, tiles_region, prologue_region, sib_lds, sib_fits), on
the CPU, by tests/cpp/test_sib_layout.cpp (g++, no HIP).

The block runs the previous pass's camera solve before its build.  The solve's LDS overlays the start of the build's
dynamic LDS: first the solve's arrays (SolveCarve, 16768 B: control block, dx_c, candidate intrinsics and chains),
which the build's prologue still reads while it writes its own tables, then solve_body<0>'s image map, which is dead
once the solve returns.  So:
  * nothing is live ACROSS the solve: the block issues its build loads behind it;
  * live from the solve to the prologue barrier: the carve.  Everything the prologue writes meanwhile (chain table K,
    target, staged poses, per-view table) lies behind the view waves' tiles, and the carve lies inside the tiles,
    which are first written behind that barrier;
  * the launch asks for max(build, window), and static + dynamic stay within the block's share of the CU.
The figures are worked out here from the LDS maps, not taken from the header.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 160 * 1024
STATIC = 4096
CARVE = 16768
# intrinsics per camera of the one-model sets (pinhole-radtan / -equi 8, omni-radtan 9, EUCM / DS 6, omni / FOV 5) and
# the configs[2] mix (omni-radtan + EUCM alternating)
MODEL_SETS = {"pr": lambda i: 8, "or": lambda i: 9, "eucm": lambda i: 6, "omni": lambda i: 5,
              "or+eucm": lambda i: 9 if i % 2 == 0 else 6}
K = 144


def cam_cols(N, nintr):
    return sum(nintr(i) for i in range(N)) + 6 * (N - 1)


def nb(C):
    return (C + 16) // 16


def lds_solve_image(N, C):
    """solve_body<0>'s dynamic map: image (tiles | aux) + 2 | Dfac, Xinv [nb][272] | rDv [16 nb] | ci [C] ints"""
    img_n = 272 * nb(C) * (nb(C) + 1) // 2 + 16 * nb(C) + 2 + 64
    return 8 * (img_n + 2 + 2 * nb(C) * 272 + 16 * nb(C)) + 4 * C


def build_doubles(N, C, gf, vt):
    CZ = 16 * nb(C)
    vbs = 44 * N + 6 * CZ
    head = N * 64 * 17 + N * 256 + N * 36 + vbs + 40 + 6 * CZ          # tiles .. frame-wave buffers
    base = head + 36 * N * (N - 1) // 2 + 8 * gf + vbs                  # + K | poses | second view-output buffer
    tg = 3 * K if 8 * (base + 3 * K) + STATIC <= LIMIT else 0
    return head, base + tg + (49 * gf * N if vt else 0)


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("sib_layout")), "test_sib_layout")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "test_sib_layout.cpp")], check=True)
    cases = [(N, name, cam_cols(N, f), bpc, gf, vt) for N in range(4, 9) for name, f in MODEL_SETS.items()
             for bpc in (1, 2) for gf in range(1, 66) for vt in (0, 1)]
    inp = "".join(f"{N} {C} {K} {bpc} {256 * bpc * gf} {vt}\n" for N, _, C, bpc, gf, vt in cases)
    r = subprocess.run([out], input=inp, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    vals = [tuple(int(t) for t in line.split()) for line in r.stdout.strip().split("\n")]
    assert len(vals) == len(cases)
    return list(zip(cases, vals))


def test_the_regions_are_the_hand_figures(rows):
    for (N, name, C, bpc, gf, vt), (g, fits, carve, window, tiles, plo, phi, sib, total) in rows:
        assert g == gf and carve == CARVE and tiles == 8 * N * 64 * 17
        head, tot = build_doubles(N, C, gf, vt)
        assert (plo, phi, total) == (8 * head, 8 * tot, 8 * tot), (N, name, gf, vt)
        if C > 64:
            assert window == CARVE + lds_solve_image(N, C)
        assert sib == max(total, window)


def test_flagship_figures(rows):
    """configs[3]: N = 8, C = 106 (nb = 7), 8 frames per block with the table: the image map is 8 * (7794 + 2 + 3808 +
    112) + 424 = 94152 B, the window 110920 B, inside the 147520 B the launch asks for anyway; the carve ends at
    16768 B, inside the 69632 B of tiles, and the prologue writes from 102208 B on"""
    got = {(N, name, bpc, gf, vt): v for (N, name, C, bpc, gf, vt), v in rows}
    g, fits, carve, window, tiles, plo, phi, sib, total = got[8, "pr", 1, 8, 1]
    assert lds_solve_image(8, 106) == 94152
    assert (fits, window, tiles, plo, total, sib) == (1, 110920, 69632, 102208, 147520, 147520)


def test_every_shape_the_host_takes_is_safe(rows):
    taken = 0
    for (N, name, C, bpc, gf, vt), (g, fits, carve, window, tiles, plo, phi, sib, total) in rows:
        if not fits:
            continue
        taken += 1
        assert C > 64                                   # the blocked solve: the C <= 64 kernels keep three launches
        assert carve <= tiles                           # live to the prologue barrier: inside the tiles, ...
        assert carve <= plo                             # ... below everything the prologue writes meanwhile
        assert window <= sib and total <= sib           # the launch covers the window and the build
        assert sib + STATIC <= LIMIT // bpc             # within the block's share of the CU
    assert taken > 0


def test_what_does_not_fit_keeps_three_launches(rows):
    for (N, name, C, bpc, gf, vt), (g, fits, carve, window, tiles, plo, phi, sib, total) in rows:
        ok = C > 64 and carve <= tiles and carve <= plo and sib + STATIC <= LIMIT // bpc
        assert bool(fits) == ok, (N, name, bpc, gf, vt)
    got = {(N, name, bpc, gf, vt): v for (N, name, C, bpc, gf, vt), v in rows}
    assert got[8, "pr", 1, 12, 1][1] == 0 and got[8, "pr", 1, 12, 0][1] == 1   # 12 frames per block: no table, no window
    assert got[4, "pr", 1, 8, 1][1] == 0                                       # C = 50: k_solve<64>
    assert got[8, "pr", 2, 1, 0][1] == 0                                       # two blocks per CU: half the LDS each
