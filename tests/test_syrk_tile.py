"""LDS banking of the tile of k_buildp's two-read SYRK operand fetch (kalibr_amd/csrc/kb_syrk_tile.h, the kernel's
KB_SYRK_DPP form), on the CPU.

tests/cpp/test_syrk_tile.cpp includes the index function the kernel uses and applies gfx950's bank rules for 8-byte
accesses: for every pair p = 0..7 and both operand reads, each 32-lane read group touches every bank pair at most
once (64 banks); for each of the 16 column stores, each 16-lane group does (32 banks); and the map is injective over
64 x 16 inside the wave's 64 x 17 doubles.  The row-major tile at the 17-double row stride fails the read rule
(2-way), which the second test shows to prove that the counting can tell the difference.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("syrk_tile") / "test_syrk_tile")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "test_syrk_tile.cpp")], check=True)
    return out


def test_reads_and_stores_are_conflict_free_and_the_map_is_injective(prog):
    r = subprocess.run([prog], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert [int(x) for x in r.stdout.split()[-3:]] == [1, 1, 64 * 16]


def test_the_counting_sees_the_conflict_of_the_17_double_stride(prog):
    r = subprocess.run([prog, "stride17"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    worst_read, worst_store, cells = [int(x) for x in r.stdout.split()[-3:]]
    assert (worst_read, worst_store, cells) == (2, 1, 64 * 16)
