"""The build kernels' launch layout (kalibr_amd/csrc/kb_build_layout.h), on the CPU.

kb_create, kb_append_frames / kb_drop_last_frames and the robust setters (kb_set_mestimator, kb_set_corner_invR) all
decide from this arithmetic whether a rig fits k_buildp (the default from four cameras on) or k_build (every weighted
handle).  The two differ: k_build always stages a target of 3 K <= 1536 doubles in LDS, k_buildp only when there is
room.  So a rig that kb_create accepts can be refused by the setters, which must then leave the handle as it was: they
ask kb_blay::build_fits before they change anything.  The figures below are worked out by hand from the kernels' LDS
maps, not taken from the header.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 160 * 1024 // 8  # doubles of LDS per block


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("build_layout") / "test_build_layout")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "test_build_layout.cpp")], check=True)

    def run(N, C, K, wpb, bpc, F):
        r = subprocess.run([out, *map(str, (N, C, K, wpb, bpc, F))], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        v = [int(x) for x in r.stdout.split()]
        return dict(fits_p=bool(v[0]), fits_b=bool(v[1]), thr_p=v[2], thr_b=v[3], lds_p=v[4], lds_b=v[5], tg=v[6])

    return run


# configs[3]'s rig shape: 8 pinhole-radtan cameras, C = 8 * 8 + 7 * 6 = 106, one view wave per camera
C4 = dict(N=8, C=106, wpb=8, bpc=1)
# k_build at N = 8, C = 106 without target and poses: tiles 8*64*17 + H 8*256 + per-camera 8*656 + 36 + Schur rows
# 16*112 + pairs 18*56
KBUILD_C4 = 8704 + 2048 + 5248 + 36 + 1792 + 1008
# k_buildp there: tiles + H + chains 8*36 + two view-output buffers 2*(44*8 + 6*112) + 40 + 6*112 + 36*28
KBUILDP_C4 = 8704 + 2048 + 288 + 2048 + 40 + 672 + 1008


def test_hand_figures():
    assert KBUILD_C4 == 18836 and KBUILDP_C4 == 14808


def test_lds_of_both_kernels_at_c4(layout):
    r = layout(K=144, F=2000, **C4)  # configs[3]: 2000 frames, a 12 x 12 corner target
    assert r["lds_b"] == 8 * (KBUILD_C4 + 3 * 144 + 8 * 4)   # 4 frames per block of 512 blocks
    assert r["lds_p"] == 8 * (KBUILDP_C4 + 3 * 144 + 8 * 8)  # 8 frames per block of 256 blocks
    assert r["tg"] == 1 and r["fits_p"] and r["fits_b"]


def test_threads(layout):
    r = layout(K=144, F=2000, **C4)
    # k_buildp: 8 view waves + 4 frame waves (28 Schur tiles, more than 2 * 5); k_build: one wave per camera
    assert (r["thr_p"], r["thr_b"]) == (768, 512)
    # two cameras, C = 22: 3 Schur tiles, two frame waves; k_build splits each camera over two waves
    r = layout(N=2, C=22, K=144, wpb=4, bpc=2, F=12)
    assert (r["thr_p"], r["thr_b"]) == (256, 256)
    # four cameras, C = 50: 10 tiles, two frame waves
    r = layout(N=4, C=50, K=144, wpb=4, bpc=2, F=12)
    assert (r["thr_p"], r["thr_b"]) == (384, 256)


def test_a_rig_kb_create_takes_can_be_too_large_for_the_weighted_build(layout):
    """N = 8, C = 106, K = 512 (3 K = 1536, the largest staged target): k_build needs 18836 + 1536 + 8 ceil(F / 512)
    doubles against 20480, so it fits up to 13 frames per block, F <= 6656.  k_buildp drops the staged target when it
    does not fit and takes the rig far beyond that.  The robust setters have to refuse such a handle."""
    assert KBUILD_C4 + 1536 + 8 * 13 <= LIMIT < KBUILD_C4 + 1536 + 8 * 14
    at = layout(K=512, F=6656, **C4)
    assert at["fits_p"] and at["fits_b"]
    over = layout(K=512, F=6657, **C4)
    assert over["fits_p"] and not over["fits_b"]
    assert over["lds_b"] == 8 * (KBUILD_C4 + 1536 + 8 * 14)
    # one corner more and k_build reads the target from global memory: it fits again
    assert layout(K=513, F=6657, **C4)["fits_b"]


def test_buildp_drops_the_staged_target_before_it_gives_up(layout):
    # k_buildp with its 4096 B of static LDS: 14808 + 512 + 1536 + 8 gf <= 20480 stages the target up to gf = 453
    assert KBUILDP_C4 + 512 + 1536 + 8 * 453 <= LIMIT < KBUILDP_C4 + 512 + 1536 + 8 * 454
    a = layout(K=512, F=256 * 453, **C4)
    b = layout(K=512, F=256 * 453 + 1, **C4)
    assert a["tg"] == 1 and b["tg"] == 0 and a["fits_p"] and b["fits_p"]
    assert b["lds_p"] == 8 * (KBUILDP_C4 + 8 * 454)
    # without the target it fits up to gf = 645
    assert layout(K=512, F=256 * 645, **C4)["fits_p"]
    assert not layout(K=512, F=256 * 645 + 1, **C4)["fits_p"]


def test_the_setters_ask_before_they_change_the_handle():
    """kb_set_mestimator / kb_set_corner_invR call robust_fits (kb_blay::build_fits for the kernel the new settings
    select) before the first write to the handle; robust_relayout itself no longer checks, so no error return of the
    fit leaves build_threads, build_pipe or the kernels half-switched."""
    src = open(os.path.join(ROOT, "kalibr_amd", "csrc", "kb_capi.hip")).read()
    body = src[src.index("static int robust_relayout(kb_handle* h) {"):]
    body = body[:body.index("\n}\n")]
    assert "fail(" not in body and "build_lds_fits" not in body
    for fn, first_write in (("int kb_set_mestimator(", "h->d.rb_kind = kind;"),
                            ("int kb_set_corner_invR(", "regrow(h, &h->rb_L")):
        f = src[src.index(fn):]
        f = f[:f.index("\n}\n")]
        assert 0 < f.index("robust_fits(h, will)") < f.index(first_write), fn
