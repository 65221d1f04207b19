"""The trailing-update schedule of the blocked LDL^T (ldl_panels, C > 64), on the CPU: the items that
kb_solve_layout.h's upd_slot / upd_first / upd_next hand to the update waves, printed by
tests/cpp/test_update_schedule.cpp (g++, no HIP), for nb = 5, 6 and 7 tile rows.  The kernel walks the same functions,
so what holds here is the order the device subtracts in.

The schedule is left-looking.  Panel q's two phases:
    A  every wave applies panel q - 1 to a tile of column q (not part of the items: wave w takes tile (q + w, q));
    B  while panel q is factored, the update waves apply the panels 0 .. q - 1 to column q + 1.
So tile (i, j), j >= 2, takes the panels 0 .. j - 2 as items of phase B of panel j - 1 and panel j - 1 in phase A of
panel j; column 1 takes panel 0 in phase A alone.  One tile is brought forward: the last diagonal tile
(nb - 1, nb - 1) takes the panels 0 .. nb - 4 one phase early, on a wave that is idle then, and panel nb - 3 alone in
its own phase (all nb - 2 on one wave there outlast that panel's factor).  The right-looking schedule before it
applied panel p to every tile right of column p + 1 while panel p + 1 was factored: the same products in the same
per-tile order, earlier than needed.

The update waves keep off the SIMDs that factor (wave w runs on SIMD w mod 4): waves 2, 3, 6, 7 while waves 0 and 1
factor, wave 5 as well once wave 0 factors alone.
"""
import os
import subprocess

import pytest

from . import solve_width_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBS = (5, 6, 7)
# tile products in phase B of the panels q = 1 .. nb - 1: q (nb - 1 - q) for column q + 1, the last diagonal tile's
# nb - 3 products moved from panel nb - 2 to panel nb - 3
PER_PHASE = {5: [3, 4 + 2, 3 - 2, 0], 6: [4, 6, 6 + 3, 4 - 3, 0], 7: [5, 8, 9, 8 + 4, 5 - 4, 0]}


@pytest.fixture(scope="module")
def items(tmp_path_factory):
    """{nb: [(q, nf, ow, wave, k, i, j, p)] in the program's order}"""
    out = os.path.join(str(tmp_path_factory.mktemp("update_schedule")), "test_update_schedule")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "test_update_schedule.cpp")], check=True)
    r = subprocess.run([out], input="".join(f"{nb}\n" for nb in NBS), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [tuple(int(t) for t in line.split()) for line in r.stdout.strip().split("\n")]
    return {nb: [row[1:] for row in rows if row[0] == nb] for nb in NBS}


@pytest.mark.parametrize("nb", NBS)
def test_every_tile_takes_every_earlier_panel_once_and_in_order(items, nb):
    got = {}
    for q, nf, ow, wave, k, i, j, p in items[nb]:
        got.setdefault((i, j), []).append((q, wave, k, p))
    for j in range(1, nb):
        for i in range(j, nb):
            seq = sorted(got.pop((i, j), []))             # by phase, then position: the order in time
            # the panels 0 .. j - 2 as items, ascending over the phases; panel j - 1 follows in phase A of panel j
            assert [p for _, _, _, p in seq] == list(range(j - 1)), (i, j)
            phases = sorted({q for q, _, _, _ in seq})
            assert phases == ([] if j == 1 else [j - 2, j - 1] if (i, j) == (nb - 1, nb - 1) else [j - 1]), (i, j)
            for ph in phases:
                part = [(wave, k) for q, wave, k, _ in seq if q == ph]
                # within a phase one wave, consecutive positions: read once, subtracted in registers, stored once
                assert len({w for w, _ in part}) == 1, (i, j, ph)
                ks = [k for _, k in part]
                assert ks == list(range(ks[0], ks[0] + len(ks))), (i, j, ph)
    assert not got                                        # no item outside the lower tiles of columns 2 .. nb - 1


@pytest.mark.parametrize("nb", NBS)
def test_a_column_is_complete_before_its_panel(items, nb):
    """column j gets its last items in phase B of panel j - 1, which ends (a block barrier) before phase A of panel j.
    What an item reads is final: the tiles (i, p) and (j, p) belong to a panel p < q, factored before phase B of
    panel q; what it writes lies right of column q, which the factor waves hold, and no two waves of a phase share a
    tile (the test above)"""
    for q, nf, ow, wave, k, i, j, p in items[nb]:
        assert 1 <= q <= nb - 2 and q < j <= i < nb and 0 <= p < q and q <= j - 1
    # a slot's tiles of one phase differ in their rows (the kernel tells a new tile by its row)
    for q in range(1, nb):
        for wave in range(8):
            tiles = []
            for qq, nf, ow, w, k, i, j, p in items[nb]:
                if (qq, w) == (q, wave) and (i, j) not in tiles:
                    tiles.append((i, j))
            assert len({i for i, _ in tiles}) == len(tiles)


@pytest.mark.parametrize("nb", NBS)
def test_the_update_waves_keep_off_the_factor_simds(items, nb):
    for q, nf, ow, wave, k, i, j, p in items[nb]:
        assert nf == (2 if nb - 1 - q > 4 else 1)
        assert wave >= 2 and wave % 4 not in range(nf), (q, wave)     # factor waves 0 .. nf - 1 on SIMDs 0 .. nf - 1
    # panel 0's factor waves are those of tests/solve_width_cases.py (the first widths of nb = 5, 6, 7)
    assert [W.factor_waves(C)[0] for C in (65, 80, 96)] == [1, 2, 2] and [W.nb(C) for C in (65, 80, 96)] == list(NBS)


@pytest.mark.parametrize("nb", NBS)
def test_counts_per_phase_and_per_wave(items, nb):
    per_q = [sum(1 for it in items[nb] if it[0] == q) for q in range(1, nb)]
    assert per_q == PER_PHASE[nb]
    # the same total as the right-looking schedule: one product per tile (i, j), j >= 2, and earlier panel p <= j - 2
    assert sum(per_q) == sum((nb - j) * (j - 1) for j in range(2, nb)) == {5: 10, 6: 20, 7: 35}[nb]
    for q in range(1, nb - 1):
        per_wave, per_simd = {}, {}
        for qq, nf, ow, wave, k, i, j, p in items[nb]:
            if qq == q:
                per_wave[wave] = per_wave.get(wave, 0) + 1
                per_simd[wave % 4] = per_simd.get(wave % 4, 0) + 1
                assert k == per_wave[wave] - 1             # positions count up from 0 within a slot
        # a wave holds one tile's products, at most q of them; two tiles only at nb = 7, q = 1 (five on four waves)
        assert max(per_wave.values()) == (2 if (nb, q) == (7, 1) else 1 if q == nb - 2 else q) <= 4, (nb, q)
        # and no SIMD more than two tiles' worth (three at nb = 7, q = 1); three tiles sit on three SIMDs
        assert max(per_simd.values()) <= (3 if (nb, q) == (7, 1) else 2 * q)
    if nb == 7:
        assert sorted(w for q, nf, ow, w, k, i, j, p in items[7] if q == 3 and p == 0) == [2, 3, 5]
        assert sorted(w for q, nf, ow, w, k, i, j, p in items[7] if q == 4 and p == 0) == [2, 3, 5]
