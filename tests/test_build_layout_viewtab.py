"""k_buildp's per-view table in the launch layout (kalibr_amd/csrc/kb_build_layout.h), on the CPU.

The table holds one record of 48 doubles, R (9) | t (3) | G (36), per (frame of the block, camera) at a stride of 49
doubles, behind every other region of k_buildp's dynamic LDS.  The host switches it on per handle where dynamic LDS +
table + the kernel's 4096 B of static LDS stay within the block's share of the CU's 160 KiB: all of it at one block per
CU, half at two, and where a block has at least two frames: the fill costs a block about what one frame gives back, so
a one-frame block (the 8-way shard of configs[3]) would only lose.  Where it does not fit the launch is exactly the one without it, so build_lds and build_fits must not
know the table.  The figures are worked out by hand from the LDS map, as tests/test_build_layout.py
does, not taken from the header.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 160 * 1024 // 8  # doubles of LDS per CU
STATIC = 4096 // 8       # k_buildp's static LDS, doubles


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    d = tmp_path_factory.mktemp("build_layout_viewtab")
    outs = {}
    for name in ("test_build_layout_viewtab", "test_build_layout"):
        outs[name] = str(d / name)
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", outs[name],
                        os.path.join(ROOT, "tests", "cpp", name + ".cpp")], check=True)
    return outs


@pytest.fixture(scope="module")
def layout(progs):
    def run(N, C, K, wpb, bpc, F):
        r = subprocess.run([progs["test_build_layout_viewtab"], *map(str, (N, C, K, wpb, bpc, F))],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        v = [int(x) for x in r.stdout.split()]
        return dict(gf=v[0], tab=v[1], total=v[2], fits=bool(v[3]), lds_p=v[4], fits_p=bool(v[5]), tg=v[6],
                    pays=bool(v[7]))

    return run


@pytest.fixture(scope="module")
def layout_before(progs):
    """tests/cpp/test_build_layout.cpp, the program of the existing layout test: what build_lds / build_fits say"""
    def run(N, C, K, wpb, bpc, F):
        r = subprocess.run([progs["test_build_layout"], *map(str, (N, C, K, wpb, bpc, F))], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        v = [int(x) for x in r.stdout.split()]
        return dict(fits_p=bool(v[0]), lds_p=v[4], tg=v[6])

    return run


# configs[3]'s rig: 8 pinhole-radtan cameras, C = 106, a 12 x 12 target, one block per CU
C4 = dict(N=8, C=106, K=144, wpb=8, bpc=1)
# k_buildp there without target and poses (tests/test_build_layout.py): tiles 8*64*17 + H 8*256 + chains 8*36 + two
# view-output buffers 2*(44*8 + 6*112) + 40 + 6*112 + 36*28
KBUILDP_C4 = 8704 + 2048 + 288 + 2048 + 40 + 672 + 1008
# four pinhole-radtan cameras, C = 4*8 + 3*6 = 50 (CZ = 64), 6 waves per block, two blocks per CU:
# tiles 4*64*17 + H 4*256 + chains 4*36 + 2*(44*4 + 6*64) + 40 + 6*64 + 36*6
N4 = dict(N=4, C=50, K=144, wpb=4, bpc=2)
KBUILDP_N4 = 4352 + 1024 + 144 + 1120 + 40 + 384 + 216


def test_hand_figures():
    assert KBUILDP_C4 == 14808 and KBUILDP_N4 == 7280


def test_table_size(layout):
    # 2000 frames over 256 blocks: 8 frames per block, 64 views, 49 doubles each
    r = layout(F=2000, **C4)
    assert r["gf"] == 8 and r["tab"] == 8 * (8 * 8 * 49) == 25088
    # 515 frames: 3 per block
    assert layout(F=515, **C4)["tab"] == 8 * (3 * 8 * 49)
    # two blocks per CU: 512 blocks, 301 frames are one per block
    r = layout(F=301, **N4)
    assert r["gf"] == 1 and r["tab"] == 8 * 4 * 49


def test_total_lds_at_configs3(layout):
    r = layout(F=2000, **C4)
    dyn = KBUILDP_C4 + 3 * 144 + 8 * 8  # + target + 8 staged poses
    assert r["lds_p"] == 8 * dyn == 122432
    assert r["total"] == 8 * (dyn + 3136) == 147520
    assert r["fits"] and r["total"] + 4096 == 151616 <= 160 * 1024


def test_most_frames_per_block_at_configs3_rig(layout):
    """per frame of the block: 8 pose doubles + 8 records of 49; beside 14808 + 432 + 512 static that is
    400 gf <= 20480 - 15752 = 4728: 11 frames per block fit, 12 do not"""
    assert KBUILDP_C4 + 432 + STATIC + 400 * 11 <= LIMIT < KBUILDP_C4 + 432 + STATIC + 400 * 12
    at = layout(F=256 * 11, **C4)
    over = layout(F=256 * 11 + 1, **C4)
    assert (at["gf"], over["gf"]) == (11, 12)
    assert at["fits"] and not over["fits"]
    assert at["total"] == 8 * (KBUILDP_C4 + 432 + 400 * 11)
    # the launch without the table is still fine there
    assert over["fits_p"] and over["tg"] == 1 and over["lds_p"] == 8 * (KBUILDP_C4 + 432 + 8 * 12)


def test_most_frames_per_block_with_the_synthetic_target(layout):
    """the synthetic configs[3] problem has a 120-corner target: 14808 + 360 + 512 + 400 gf <= 20480 holds with
    equality at 12 frames per block (3072 frames), the most an 8-camera rig gets; 13 do not fit"""
    assert KBUILDP_C4 + 360 + STATIC + 400 * 12 == LIMIT
    rig = dict(C4, K=120)
    at, over = layout(F=3072, **rig), layout(F=3073, **rig)
    assert (at["gf"], over["gf"]) == (12, 13)
    assert at["fits"] and at["total"] + 4096 == 160 * 1024
    assert not over["fits"] and over["fits_p"]


def test_one_frame_blocks_do_not_take_the_table(layout):
    # configs[3]'s rig: up to 256 frames are one per block; the 250-frame shard of the 8-way split is such a handle
    assert [layout(F=F, **C4)["gf"] for F in (250, 256, 257)] == [1, 1, 2]
    assert [layout(F=F, **C4)["pays"] for F in (250, 256, 257, 2000)] == [False, False, True, True]
    assert layout(F=250, **C4)["fits"]  # room is not the reason
    # two blocks per CU: one frame per block up to 512 frames
    assert [layout(F=F, **N4)["pays"] for F in (301, 512, 513)] == [False, False, True]


def test_two_blocks_per_cu_share_the_lds(layout):
    """bpc = 2: each block has 10240 doubles.  7280 + 432 + 512 + (8 + 4*49) gf: 204 gf <= 2016, so 9 frames per
    block (4608 frames) fit and 10 do not, although the whole LDS would hold them: at one block per CU the same
    10 frames per block fit."""
    assert KBUILDP_N4 + 432 + STATIC + 204 * 9 <= LIMIT // 2 < KBUILDP_N4 + 432 + STATIC + 204 * 10
    at = layout(F=512 * 9, **N4)
    over = layout(F=512 * 9 + 1, **N4)
    assert (at["gf"], over["gf"]) == (9, 10)
    assert at["fits"] and not over["fits"] and over["fits_p"]
    assert over["total"] == 8 * (KBUILDP_N4 + 432 + 204 * 10) and over["total"] + 4096 <= 160 * 1024
    one = layout(F=256 * 10, **dict(N4, bpc=1))
    assert one["gf"] == 10 and one["fits"]


@pytest.mark.parametrize("rig,F", [(C4, 2000), (C4, 256 * 11 + 1), (C4, 515), (N4, 301), (N4, 512 * 9 + 1),
                                   (dict(C4, K=512), 256 * 453 + 1)])
def test_the_layout_without_the_table_is_unchanged(layout, layout_before, rig, F):
    """build_lds, build_fits and the staged-target decision are what the existing layout program reports, whether
    the table fits (on) or not (off)"""
    a, b = layout(F=F, **rig), layout_before(F=F, **rig)
    assert (a["lds_p"], a["fits_p"], a["tg"]) == (b["lds_p"], b["fits_p"], b["tg"])
    assert a["total"] == a["lds_p"] + a["tab"]
