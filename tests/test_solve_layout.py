"""The reduced-system launch layout (kalibr_amd/csrc/kb_solve_layout.h), on the CPU: every figure the header exports,
printed by tests/cpp/test_solve_layout.cpp (g++, no HIP), against the independent restatements of
tests/solve_width_cases.py and tests/marginal_cases.py, for every (N, C) a handle admits and every width a rig reaches.
kb_create, kb_covariance and the marginal entry points take these figures from the header, and solve_body, k_cov_cam,
k_colimg and k_colsumx carve their LDS by it, so a figure that holds here is the one the device runs with.

What each comparison replaces (the source lines of kb_create, cov_cam_fn and kb_covariance that
test_solve_width_cases.py used to match as text):
    "if (h->C > 111) {"                                -> max_c == MAX_C
    "if (64 * d.wpb > 512) {"                          -> cams_fit, nsplit, wpb per N (the 8-camera limit)
    "h->build_pipe = d.nsplit == 1 && h->N <= ..."     -> pipe per N == build_kernel(N), buildp_max_cams
    "const int CZ = 16 * ((C + 16) / 16);", "const int nb = (C + 16) / 16, n16 = 16 * nb;"  -> nb, img_n16
    "h->lds_camexp = ..."                              -> lds_camexp
    "h->lds_schur = ..."                               -> lds_schur
    "h->lds_solve = ..." (both branches)               -> lds_solve, and the ten offsets of either map
    "d.img_n = ..."                                    -> img_n, img_ntz
    "h->lds_colimg = ..."                              -> lds_colimg
    "h->solve_threads = ..."                           -> solve_threads
    "h->fn_solve = C <= 16 ? ...", "return C <= 16 ? ... k_cov_cam ..."  -> solve_cm (one ladder for both kernels)
    "... h->ms = ts <= 1 ? 1 : ts <= 4 ? 4 : 7;"       -> schur_ms, ntiles
    "const int nct = (C + 15) / 16;"                   -> nct, nks
    "const size_t lds_frames = ..."                    -> lds_cov_frames
    "const int eoff = ..."                             -> eoff
    "const size_t lds_cam = ..."                       -> lds_cov_cam
    "constexpr int kXMaxRanks = 64;"                   -> x_max_ranks
and of kb_kernels.hip: kTS, kTileSz, kCovWaves / kCovFrames (now the header's) -> ts, tile, cov_waves, cov_frames;
k_cov_frames' "nct = (C + 15) >> 4, nks = (C + 3) >> 2" -> nct, nks.
"""
import os
import subprocess

import pytest

from . import marginal_cases as MC
from . import solve_width_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_KEYS = ("S", "bv", "gl", "Hs", "T", "K", "Dfac", "Xinv", "rDv", "ci")
# the largest static LDS (group_segment_fixed_size) of each kernel family in the code object the bounds were taken
# from; test_solve_width_cases.py and test_marginal_cases.py hold the built library to the bounds
MEASURED_STATIC = dict(solve=25824, cov_cam=912, schur=16, cov_frames=2304, colimg=0, camexpand=0, marg=9088)


def _pairs(line):
    t = line.split()
    return {t[i]: int(t[i + 1]) for i in range(0, len(t), 2)}


def run_layout(tmp_dir, shapes=()):
    """the output lines of tests/cpp/test_solve_layout.cpp (compiled into tmp_dir): the constants, then one per shape"""
    out = os.path.join(str(tmp_dir), "test_solve_layout")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "test_solve_layout.cpp")], check=True)
    r = subprocess.run([out], input="".join(f"{N} {C}\n" for N, C in shapes), capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip().split("\n")


def header_constants(tmp_dir):
    """the header's constants (the static LDS bounds st_* among them), for the tests that read the built library"""
    return _pairs(run_layout(tmp_dir)[0])


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """(constants, {(N, C): figures}) over admitted_shapes() and every reachable width at its camera counts"""
    shapes = sorted(set(W.admitted_shapes()) | {(N, C) for C in W.reachable_widths() for N in range(1, 11)
                                                if 5 * N + 6 * (N - 1) <= C <= 9 * N + 6 * (N - 1)})
    lines = run_layout(tmp_path_factory.mktemp("solve_layout"), shapes)
    assert len(lines) == 1 + len(shapes)
    rows = [_pairs(l) for l in lines[1:]]
    assert [(v["N"], v["C"]) for v in rows] == shapes
    return _pairs(lines[0]), dict(zip(shapes, rows))


def test_the_shapes_cover_what_a_handle_admits(layout):
    _, rows = layout
    assert set(W.admitted_shapes()) <= set(rows) and len(W.admitted_shapes()) == 149
    assert set(W.reachable_widths()) <= {C for _, C in rows}
    assert (8, W.MAX_C) in rows and (1, 5) in rows and (10, 104) in rows   # ten cameras: refused by their count alone


def test_constants(layout):
    k, _ = layout
    assert k["max_c"] == W.MAX_C == MC.K_CREATE_MAX_C == 111
    assert k["lds_limit"] == k["lds_limit_build"] == W.LDS_BYTES == MC.LDS_BYTES
    assert (k["ts"], k["tile"], k["x_max_ranks"]) == (W.K_TS, W.K_TILE, W.K_X_MAX_RANKS) == (17, 272, 64)
    assert (k["cov_waves"], k["cov_frames"]) == (W.K_COV_WAVES, W.K_COV_FRAMES) == (4, 8)
    assert k["marg_max_c"] == MC.K_MARG_MAX_C and k["marg_lds_stage"] == MC.K_MARG_LDS_STAGE
    assert k["chain_lds"] == MC.CHAIN_LDS_BYTES and k["marg_threads_max"] == 1024
    assert k["buildp_max_cams"] == W.MAX_CAMS == 8
    # the array capacities hold every admitted width (the entry points no longer test "C > 112")
    assert k["max_c"] <= k["cov_max_c"] and k["max_c"] <= k["marg_max_c"]


def test_static_bounds_are_the_measured_sizes_rounded_up(layout):
    k, _ = layout
    for fam, size in MEASURED_STATIC.items():
        assert k["st_" + fam] == (size // 256 + 1) * 256, fam


def test_selectors(layout):
    _, rows = layout
    for (N, C), v in rows.items():
        assert (v["nb"], v["ntiles"]) == (W.nb(C), W.nb(C) * (W.nb(C) + 1) // 2), (N, C)
        assert (v["solve_cm"], v["solve_threads"], v["schur_ms"]) == (W.solve_cm(C), W.solve_threads(C), W.schur_ms(C))
        assert (v["nks"], v["nct"]) == W.cov_frames_steps(C), C
        assert bool(v["pipe"]) == (W.build_kernel(N) == "k_buildp") and bool(v["cams_fit"]) == (N <= W.MAX_CAMS)
        assert (v["nsplit"], v["wpb"]) == (max(1, -(-4 // N)), N * max(1, -(-4 // N)))
    assert [rows[1, 5]["solve_cm"], rows[8, 111]["solve_cm"], rows[5, 64]["solve_cm"], rows[6, 65]["solve_cm"]] == \
        [16, 0, 64, 0]


def test_image(layout):
    _, rows = layout
    for (N, C), v in rows.items():
        assert v["img_ntz"] == W.K_TILE * W.nb(C) * (W.nb(C) + 1) // 2 and v["img_n16"] == 16 * W.nb(C)
        assert v["img_n"] == W.img_n(C), C
    assert rows[8, 111]["img_n"] == 272 * 28 + 112 + 2 + 64 and rows[6, 65]["img_n"] == 272 * 15 + 80 + 2 + 64


def test_the_map_of_solve_body(layout):
    _, rows = layout
    for (N, C), v in rows.items():
        want = W.solve_offsets(N, C)
        tag = "p" if C <= 64 else "i"
        assert {q: v[f"{tag}_{q}"] for q in MAP_KEYS} == want, (N, C)
        # the regions lie in order and end within the bytes asked for; ci holds C ints
        order = ("S", "bv", "gl", "Hs", "T", "K", "ci") if C <= 64 else ("S", "bv", "Dfac", "Xinv", "rDv", "ci")
        assert [want[q] for q in order] == sorted(want[q] for q in order)
        assert 8 * want["ci"] + 4 * C <= v["lds_solve"] == W.lds_solve(N, C)
        if C > 64:   # the image is staged whole: its tail (the slots of ranks 1 ..) reaches into Dfac, never past Xinv
            assert want["Dfac"] < v["img_n"] <= want["Xinv"]
    assert W.solve_offsets(2, 22)["ci"] == 253 + 23 + 22 + 512 + 288 and W.lds_solve(2, 22) == 8 * 1098 + 88


def test_dynamic_sizes(layout):
    _, rows = layout
    for (N, C), v in rows.items():
        assert v["lds_schur"] == W.lds_schur(C) and v["lds_camexp"] == W.lds_camexp(N)
        assert v["lds_colimg"] == W.lds_colimg(N, C) and v["lds_cov_frames"] == W.lds_cov_frames(C)
        assert v["eoff"] == W.cov_eoff(N, C) and v["lds_cov_cam"] == W.lds_cov_cam(N, C)
        # k_cov_cam's second triangle starts on a 16-byte boundary behind everything the factorisation keeps
        assert v["eoff"] % 2 == 0 and 8 * v["eoff"] >= (v["lds_solve"] if C <= 64 else 8 * W.solve_offsets(N, C)["Xinv"])
    assert rows[8, 111]["lds_cov_frames"] == W.lds_cov_frames(111) == 156424
    assert rows[8, 111]["lds_schur"] == 8 * 16 * 112 and rows[8, 111]["lds_camexp"] == 8 * (2048 + 2304)


def test_marginal(layout):
    _, rows = layout
    for (N, C), v in rows.items():
        doubles, stage = MC.marg_lds_doubles(C)
        assert (bool(v["marg_full"]), v["marg_doubles"], bool(v["marg_stage"])) == (MC.marg_full(C), doubles, stage), C
        assert v["marg_bytes"] == MC.marg_lds_bytes(C)
        assert (v["marg_threads"], v["marg_block"]) == (MC.marg_threads(C), MC.marg_block(C)), C
    assert rows[1, 5]["marg_bytes"] == MC.CHAIN_LDS_BYTES and rows[8, 111]["marg_bytes"] == 8 * (6216 + 12321 + 222)
    assert (rows[1, 5]["marg_threads"], rows[8, 111]["marg_block"]) == (64, 1024)


def test_every_admitted_shape_fits_with_the_static_bounds(layout):
    """the *_fits predicates of kb_create, kb_covariance and k_marg add the static bounds: no rig is newly refused"""
    k, rows = layout
    for (N, C), v in rows.items():
        assert v["solve_fits"] and v["cov_fits"] and v["marg_fits"], (N, C)
        for lds, st in (("lds_solve", "solve"), ("lds_cov_cam", "cov_cam"), ("lds_schur", "schur"),
                        ("lds_cov_frames", "cov_frames"), ("lds_colimg", "colimg"), ("lds_camexp", "camexpand"),
                        ("marg_bytes", "marg")):
            assert v[lds] + k["st_" + st] <= k["lds_limit"], (N, C, lds)
    tight = max(v["lds_cov_frames"] for v in rows.values()) + k["st_cov_frames"]
    assert k["lds_limit"] - tight == 163840 - 156424 - 2560
