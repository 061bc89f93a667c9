"""tests/tx_geometry.py: the model of tx_batch_kernel's tile cuts against a
per-element count, and what the cases of tests/test_gpu_tx_sweep.py reach.
The coverage claims of that file are conditions on its inputs, so they are
asserted here, without a GPU."""
import numpy as np
import pytest

import tx_geometry as g
from tx_geometry import CASES


@pytest.mark.parametrize("es,addr16", [(2, 0), (2, 2), (2, 14), (1, 0), (1, 3), (1, 15)])
@pytest.mark.parametrize("gap,splits", [(0, (3,)), (1, (1, 2)), (903, (2, 1, 1)), (2903, (2,)), (168, (1, 1, 1))])
def test_tiles_equal_a_count_per_element(es, addr16, gap, splits):
    """every element of every row to its tile by address arithmetic alone: the
    call's row starts at element s of the address space, its tiles are the
    runs of 2,048 elements from the last multiple of 8 at or below s"""
    case = g.Case(9, sum(splits), gap, addr16=addr16, es=es, splits=splits, tail=4)
    P = case.P
    rows = case.rows()
    assert len(rows) == 9 * len(splits)
    for row in rows:
        s = addr16 // es + row.channel * case.ld + row.first_packet * P
        assert row.a == s % 8
        e = s + np.arange(row.npk * P)
        tile = (e - (s - s % 8)) // 2048
        cut = np.flatnonzero(np.diff(tile)) + 1
        np.testing.assert_array_equal(row.lo, np.concatenate([[0], cut]))
        np.testing.assert_array_equal(row.hi, np.concatenate([cut, [row.npk * P]]))
        pos = np.arange(row.npk * P)
        r = pos % P
        start, gapz = r == 0, r >= 1880
        for t in range(row.lo.size):
            lo, hi = int(row.lo[t]), int(row.hi[t])
            assert row.tile_of(lo) == t and row.tile_of(hi - 1) == t
            assert row.residue[t] == lo % P
            assert row.starts[t] == start[lo:hi].sum()
            assert row.in_gap[t] == gapz[lo:hi].all()
            near = lambda e, what: any((e + d) % P == what for d in range(-5, 6))
            assert row.near_start[t] == (near(lo, 0) or near(hi, 0))
            assert row.near_end[t] == (near(lo, 1880 % P) or near(hi, 1880 % P))
            assert row.cut[t] == (t > 0)
            assert row.first[t] == (t == 0 and row.call == 0)
            assert row.last[t] == (hi == row.npk * P)
            assert row.ragged[t] == (row.last[t] and hi - lo < 2048)
            assert row.in_last_gap[t] == (row.in_gap[t] and lo >= (row.npk - 1) * P + 1880)


def test_alignment_follows_the_element_size():
    # 6 bytes past a boundary is 3 int16 and 6 codes; rows an odd ld apart take all 8 classes
    assert g.alignment(6, 2, 0, 101) == 3 and g.alignment(6, 1, 0, 101) == 6
    assert g.alignment(6, 2, 3, 101, start=2783) == (3 + 303 + 2783) % 8
    for es in (1, 2):
        assert sorted(g.alignment(2, es, c, 5569) for c in range(8)) == list(range(8))


@pytest.mark.parametrize("gap", [0, 1, 7, 903, 2903])
def test_packets_for_every_residue_is_the_least(gap):
    """with that many packets the cuts of 8 rows of the 8 alignments cover
    0..P-1, with one fewer they do not; any address and any odd ld give those 8
    alignments.  A row's start is no cut: residue 0 needs a later tile that
    starts on a packet's first sample."""
    npk = g.packets_for_every_residue(gap)
    full = g.coverage(g.Case(8, npk, gap, addr16=2).rows())
    assert full["every_residue"] and full["alignments"] == list(range(8))
    less = g.coverage(g.Case(8, npk - 1, gap, addr16=6).rows())
    assert not less["every_residue"] and less["residues"] < less["P"]


def test_a_period_equal_to_the_tile_has_no_sweep():
    assert g.packets_for_every_residue(168) is None
    for row in CASES["s16_gap168"].rows():
        assert set(row.residue[1:]) == {(2048 - row.a) % 2048}


@pytest.mark.parametrize("name", ["s16_gap0", "s16_gap1", "s16_gap903", "alaw_gap903", "ulaw_gap1", "s16_gap2903",
                                  "s16_gap903_136ch"])
def test_the_sweeps_cut_at_every_residue(name):
    """over 8 rows of the 8 alignments together (each row alone meets about an
    eighth of the residues)"""
    case = CASES[name]
    assert case.nch in (8, 136) and case.ld % 2 == 1 and case.ld > case.n and case.splits is None
    assert case.npk == g.packets_for_every_residue(case.gap) + 1
    cov = g.coverage(case.rows())
    assert cov["every_residue"] and cov["residues"] == case.P
    assert cov["alignments"] == list(range(8))
    assert cov["first"] == case.nch               # the zero-history tile of every row
    assert cov["near_start"] >= 8 and cov["near_end"] >= 8
    # every residue includes the cuts in a packet's last four samples and at both ends of its gap
    res = set(np.concatenate([r.residue[r.cut] for r in case.rows()]).tolist())
    assert {1876, 1877, 1878, 1879, 1880 % case.P, case.P - 1, 0} <= res
    # a tile behind the row's first that starts on a packet's sample 0, whole, with the tile before it
    # ending on the previous packet's last gap zero (its last sample at gap 0): the 9 history symbols
    # come from the previous packet
    assert any(((r.residue == 0) & r.cut & r.whole).any() for r in case.rows())
    if case.gap < 168:                            # P < tile: some tiles hold two packet starts
        assert cov["starts"].get(2, 0) > 0 and cov["starts"].get(1, 0) > 0
    else:
        assert cov["starts"].get(0, 0) > 0 and cov["starts"].get(1, 0) > 0


def test_gaps_that_hold_whole_tiles():
    """a full tile of 2,048 inside a gap needs gap >= 2,048; some of them lie in
    the gap that closes the call, where no packet follows"""
    cov = g.coverage(CASES["s16_gap2903"].rows())
    assert cov["whole_in_gap"] > 2000 and cov["whole_in_last_gap"] >= 8
    small = g.coverage(CASES["s16_gap903"].rows())
    assert small["whole_in_gap"] == 0             # what the suite had before: none
    deg = CASES["s16_gap168"]
    assert deg.P == g.TILE
    cov = g.coverage(deg.rows())
    assert cov["in_gap"] > 0 and cov["in_last_gap"] > 0 and not cov["every_residue"]


@pytest.mark.parametrize("name", ["calls41_gap903", "calls41_gap0", "mixed_gap903", "mixed_gap0"])
def test_split_calls_restart_the_grid_at_every_alignment(name):
    case = CASES[name]
    assert sum(case.calls) == 41 and case.nch == 8
    rows = case.rows()
    for c in range(8):
        mine = [r for r in rows if r.channel == c]
        assert [r.stream_start for r in mine] == [True] + [False] * (len(mine) - 1)
        assert all(r.lo[0] == 0 for r in mine)
        # P is odd at gap 903 and a multiple of 8 at gap 0, where the calls of a row share its class
        assert [r.a for r in mine] == [(mine[0].a + r.first_packet * case.P) % 8 for r in mine]
        # calls of 1, 2, 3, 5, 30 start 0, 1, 3, 6, 11 packets in: 11 = 3 mod 8
        want = 1 if case.gap == 0 else 8 if len(mine) == 41 else 4
        assert len({r.a for r in mine}) == want, (c, [r.a for r in mine])
    assert {r.a for r in rows} == set(range(8))
    assert g.coverage(rows)["first"] == 8


@pytest.mark.parametrize("name", ["launch2_s16", "launch2_alaw"])
def test_the_second_launch_holds_a_packet(name):
    case = CASES[name]
    assert case.n == 180_007_520
    row, = case.rows()
    assert row.lo.size == 87_895 > g.MAX_TILES_PER_LAUNCH
    t = row.tile_of(3 * case.P)
    assert 3 * case.P == 135_005_640 and t == 65_920 >= g.MAX_TILES_PER_LAUNCH
    assert g.coverage([row])["launches"] == 2
    assert "launch 1" in case.locate(0, 3 * case.P) and "tile 65920" in case.locate(0, 3 * case.P)
    # packet 3 is the only one behind the first launch's 65,535 tiles
    assert 2 * case.P + 1880 < g.MAX_TILES_PER_LAUNCH * g.TILE - 7 < 3 * case.P


@pytest.mark.parametrize("name,es", [("rows4g_s16", 2), ("rows4g_alaw", 1)])
def test_rows_start_past_4_and_8_gib(name, es):
    case = CASES[name]
    assert case.es == es and case.nch == 3
    assert case.ld * es > 2**32 and 2 * case.ld * es > 2**33
    assert case.ld % 2 == 1 and len({r.a for r in case.rows()}) == 3


def test_grid_x_cases_straddle_a_block_row():
    for nch in g.GRID_X_NCH:
        case = CASES[f"gridx_{nch}"]
        assert case.nch == nch and case.npk == 2 and case.ld % 2 == 1
        assert {r.a for r in case.rows()} == set(range(8))
    assert set(g.GRID_X_NCH) >= {127, 128, 129, 257}


def test_locate_names_the_tile_and_its_class():
    case = CASES["s16_gap2903"]
    row = case.rows(channels=[5])[0]
    t = int(np.flatnonzero(row.in_gap & row.whole)[0])
    msg = case.locate(5, int(row.lo[t]) + 7)
    assert f"channel 5 call 0" in msg and f"tile {t} " in msg and "in_gap" in msg and f"a = {row.a}" in msg
    split = CASES["mixed_gap903"]
    assert "call 2 (packets 3..5" in split.locate(0, 3 * split.P)
    assert "behind" in split.locate(0, split.n)
