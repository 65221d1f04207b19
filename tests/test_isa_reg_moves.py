"""tools/isa_reg_moves.py's counting on a short hand-written assembly text (no compiler, no GPU): the instruction
classes, the smallest loop that holds every v_mfma_f64_4x4x4, and the assembler's register figures."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import isa_reg_moves as M  # noqa: E402

ASM = """\
_Z1kv:                                  ; @_Z1kv
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_accvgpr_write_b32 a0, v1
.LBB0_1:                                ; =>This Loop Header: Depth=1
\tv_accvgpr_read_b32 v2, a0
\tv_mfma_f64_16x16x4_f64 a[2:9], v[0:1], v[2:3], a[2:9]
.LBB0_2:                                ;   Parent Loop BB0_1 Depth=1
\tds_read_b64 v[4:5], v6
\tv_accvgpr_write_b32 a1, v4             ; a comment with v_accvgpr_read_b32 in it
\tv_mfma_f64_4x4x4_4b_f64 v[8:9], v[4:5], v[4:5], v[8:9]
\tv_readlane_b32 s2, v8, 3
\tv_mfma_f64_4x4x4_4b_f64 v[10:11], v[4:5], v[4:5], v[10:11]
\tv_accvgpr_read_b32 v4, a1
\ts_cbranch_scc1 .LBB0_2
; %bb.3:
\tv_fma_f64 v[12:13], v[8:9], v[10:11], v[12:13]
\tglobal_store_dwordx2 v6, v[12:13], s[0:1]
\ts_cbranch_vccnz .LBB0_1
; %bb.4:
\ts_endpgm
.Lfunc_end0:
; NumVgprs: 84
; NumAgprs: 72
; ScratchSize: 0
; Occupancy: 3
"""
LINES = ASM.split("\n")
END = LINES.index(".Lfunc_end0:")


def test_opcode_skips_labels_comments_and_directives():
    assert M.opcode("\tv_accvgpr_write_b32 a0, v1") == "v_accvgpr_write_b32"
    assert M.opcode(".LBB0_1:   ; loop") is None
    assert M.opcode("; %bb.0:") is None
    assert M.opcode("\t.p2align 8") is None
    assert M.opcode("") is None


def test_whole_kernel_counts():
    c = M.count(LINES, 0, END)
    assert c["all"] == 15
    assert c["accvgpr"] == 4  # the one named in a comment is not an instruction
    assert c["lane"] == 1
    assert c["mfma"] == 3
    assert c["valu"] == 9  # copies, lane move, MFMAs and the FMA
    assert c["salu"] == 4 and c["lds"] == 1 and c["vmem"] == 1


def test_both_backward_branches_are_loops():
    assert M.loops(LINES, 0, END) == [(LINES.index(l1), LINES.index(b1)) for l1, b1 in
                                      ((".LBB0_2:                                ;   Parent Loop BB0_1 Depth=1",
                                        "\ts_cbranch_scc1 .LBB0_2"),
                                       (".LBB0_1:                                ; =>This Loop Header: Depth=1",
                                        "\ts_cbranch_vccnz .LBB0_1"))]


def test_view_loop_is_the_inner_loop_with_every_4x4x4():
    span, pat, n = M.mfma_loop(LINES, 0, END)
    assert pat == "v_mfma_f64_4x4x4" and n == 2
    assert LINES[span[0]].startswith(".LBB0_2:") and LINES[span[1] - 1] == "\ts_cbranch_scc1 .LBB0_2"
    c = M.count(LINES, *span)
    assert (c["all"], c["accvgpr"], c["lane"], c["mfma"], c["lds"]) == (7, 2, 1, 2, 1)


def test_without_4x4x4_the_16x16x4_loop_is_taken():
    lines = [l for l in LINES if "4x4x4" not in l]
    span, pat, n = M.mfma_loop(lines, 0, lines.index(".Lfunc_end0:"))
    assert pat == "v_mfma_f64_16x16x4" and n == 1
    assert lines[span[0]].startswith(".LBB0_1:") and lines[span[1] - 1] == "\ts_cbranch_vccnz .LBB0_1"


def test_metadata_follows_the_kernel_body():
    assert M.metadata(LINES, END) == {"vgprs": 84, "agprs": 72, "scratch": 0, "occupancy": 3}
