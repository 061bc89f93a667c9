"""tests/tx_mask_geometry.py: what the cases of
tests/test_gpu_tx_mask_sweep.py reach.  Its coverage claims are conditions on
the inputs (addresses, masks, own indices), so they are asserted here, without
a GPU; the model itself is checked against a count per element."""
import numpy as np
import pytest

import tx_geometry as g
import tx_mask_geometry as mg
from tx_mask_geometry import CASES, Masked

SWEEPS = ["s16_gap903", "s16_gap0", "alaw_gap903"]


def test_the_sequence_is_de_bruijn():
    """B = 0000100110101111: its 16 cyclic windows of 4 are the 16 patterns"""
    B = mg.DE_BRUIJN
    assert "".join(map(str, B)) == "0000100110101111"
    wins = {tuple(B[(s + np.arange(4)) % 16]) for s in range(16)}
    assert len(wins) == 16
    # windows() of a row of the sweep mask is that window, slot k-1 first
    m = mg.sweep_mask(8, 40, 1)
    w = mg.windows(m)
    for k in range(1, 38):
        assert w[3, k] == int("".join(str(int(b != 0)) for b in m[3, k - 1:k + 3]), 2)
        assert tuple((m[3, k - 1:k + 3] != 0).astype(int)) == tuple(B[(k - 1 + np.arange(4)) % 16])
    assert set(np.unique(m)) == {0, 1, 2, 0x80, 0xFF}


@pytest.mark.parametrize("gap,es,addr16", [(0, 2, 2), (5, 2, 14), (903, 1, 3), (168, 2, 0)])
def test_pairs_equal_a_count_per_element(gap, es, addr16):
    """pair_coverage against address arithmetic alone: element e of the
    address space starts a tile where e is a multiple of 8 that is 2,048 k past
    the last multiple of 8 at or below the row's first element"""
    case = g.Case(19, 9, gap, addr16=addr16, es=es, tail=4)
    mask = mg.random_mask(3, case.nch, case.npk)
    P = case.P
    want = np.zeros((P, 16), bool)
    for c in range(case.nch):
        s = addr16 // es + c * case.ld
        for p in range(1, case.n):
            if (s + p - (s - s % 8)) % 2048 == 0 and 1 <= p // P <= case.npk - 3:
                k = p // P
                want[p % P, int("".join(str(int(b != 0)) for b in mask[c, k - 1:k + 3]), 2)] = True
    np.testing.assert_array_equal(mg.pair_coverage(case, mask), want)
    assert want.any()


@pytest.mark.parametrize("name", SWEEPS)
def test_the_sweeps_cut_every_residue_under_every_window(name):
    masked, pre = mg.sweep_case(name)
    case, mask = masked.case, masked.mask
    assert case.nch == 136 and case.splits is None and case.ld % 2 == 1 and case.ld > case.n
    assert case.npk == mg.packets_for_every_pair(case.gap) == {0: 259, 903: 290}[case.gap]
    assert case.addr16 == (2 if case.es == 2 else 3)
    assert set(np.unique(mask)) == {0, 1, 2, 0x80, 0xFF}
    seen = mg.pair_coverage(case, mask)
    assert seen.shape == (case.P, 16) and seen.all()
    # the named npk is the least: with one packet fewer some pair is missing
    less = g.Case(case.nch, case.npk - 1, case.gap, addr16=case.addr16, es=case.es)
    assert less.ld % 2 == 1
    short = mg.pair_coverage(less, mask[:, :-1])
    assert not short.all() and short.sum() < seen.sum()
    # the plain sweeps need two packets fewer: the window reaches two slots past the cut
    assert case.npk >= g.packets_for_every_residue(case.gap) + 2
    # alignments 0..7, 17 channels each, and a class is c = const mod 8: all 16 shifts in it
    a = np.array([g.alignment(case.addr16, case.es, c, case.ld) for c in range(case.nch)])
    assert sorted(set(a.tolist())) == list(range(8))
    win = mg.windows(mask)
    for cls in range(8):
        ch = np.flatnonzero(a == cls)
        assert ch.size == 17 and len(set((ch % 8).tolist())) == 1
        assert {int(c) // 8 % 16 for c in ch} == set(range(16))
        # the 16 channels one block loops over disagree about every slot: 16 different windows
        loop = win[ch[:16], 1:case.npk - 2]
        assert (np.sort(loop, axis=0) == np.arange(16)[:, None]).all()


@pytest.mark.parametrize("name", SWEEPS)
def test_the_preroll_spreads_the_own_indices(name):
    """own indices in front of the sweep: at least 5 different ones among the
    first 16 channels of every class, 0 among them; rows 0..8 of the carrier
    table, both signs, and the step from 8 to 9 at different slots"""
    masked, pre = mg.sweep_case(name)
    case = masked.case
    assert pre.shape == (136, mg.PREROLL) and mg.PREROLL == 12
    idx0 = masked.index[:, 0]
    np.testing.assert_array_equal(idx0, (pre != 0).sum(axis=1))
    np.testing.assert_array_equal(masked.index[:, -1], idx0 + (masked.mask != 0).sum(axis=1))
    a = np.array([g.alignment(case.addr16, case.es, c, case.ld) for c in range(case.nch)])
    for cls in range(8):
        mine = idx0[np.flatnonzero(a == cls)[:16]]
        assert len(set(mine.tolist())) >= 5 and 0 in mine, (cls, mine)
        # the slot of the sweep in which own index 9 is sent differs within the loop
        nine = {int(np.argmax(masked.index[c] == 9)) for c in np.flatnonzero(a == cls)[:16] if idx0[c] < 9}
        assert len(nine) >= 5 and 0 not in nine
    sent = masked.index[:, :-1][masked.mask != 0]            # the own index of every packet of the sweep
    assert set(range(13)) <= set(sent.tolist())
    assert (sent[sent > 8] % 2 == 0).any() and (sent[sent > 8] % 2 == 1).any()


@pytest.mark.parametrize("gap", [903, 0])
def test_joins_at_a_cut(gap):
    masked = mg.join_case(gap)
    case, mask = masked.case, masked.mask
    assert case.gap == gap and case.ld % 2 == 1 and case.ld > case.n and case.splits is None
    joins = mg.cut_joins(gap, case.npk)
    # all 50 residues occur, at 6 or 7 slots per alignment
    assert sorted(set(joins)) == list(range(8))
    assert {r for v in joins.values() for _, r in v} == set(range(mg.JOIN_SPAN))
    assert all(6 <= len(v) <= 7 for v in joins.values())
    assert case.nch == 8 * max(len(v) for v in joins.values())
    assert case.npk == mg.packets_for_every_join_residue(gap) + 1
    # with fewer packets than that some residue has no cut
    few = mg.cut_joins(gap, mg.packets_for_every_join_residue(gap) - 1)
    assert {r for v in few.values() for _, r in v} < set(range(mg.JOIN_SPAN))
    # a channel is idle in front of one slot and active from it on; the j-th of a class joins at its j-th cut slot
    act = mask != 0
    assert set(np.unique(mask)) == {0, 1, 2, 0x80, 0xFF}
    for c in range(case.nch):
        k0 = masked.first_slot(c)
        assert k0 is not None and not act[c, :k0].any() and act[c, k0:].all()
        mine = joins[g.alignment(case.addr16, case.es, c, case.ld)]
        if c // 8 < len(mine):
            assert k0 == mine[c // 8][0]
    # the condition: every cut residue below 50 in a row whose first packet ever lies in the cut's slot
    assert mg.joins_met(masked).all()
    # and it is a condition on the mask: with everyone active from slot 0 no cut meets a join
    assert not mg.joins_met(Masked(case, np.ones_like(mask))).any()
    # after the pre-roll and reset_channels the own indices are 0 again: the same condition
    assert not masked.index[:, 0].any()


@pytest.mark.parametrize("name", ["calls41_gap903", "calls41_gap0", "mixed_gap903", "mixed_gap0"])
def test_split_calls_carry_state_over_an_idle_tail(name):
    """a row whose last active slot of a call is not that call's last slot, and
    which sends again in a later call: its history comes from the saved word"""
    case = CASES[name]
    mask = mg.random_mask(50 + case.gap, case.nch, case.npk)
    act = mask != 0
    found = 0
    k = 0
    for n in case.calls[:-1]:
        tail_idle = ~act[:, k + n - 1]
        sent = act[:, :k + n - 1].any(axis=1)
        again = act[:, k + n:].any(axis=1)
        found += int((tail_idle & sent & again).sum())
        k += n
    assert found >= 8
    assert not act[1].any() and act[5].all()          # a row idle throughout and one always active


@pytest.mark.parametrize("name", ["launch2_s16", "launch2_alaw"])
def test_the_masked_second_launch(name):
    case = CASES[name]
    assert mg.LAUNCH2_MASK.tolist() == [[1, 0, 1, 1]]
    masked = Masked(case, mg.LAUNCH2_MASK)
    row, = case.rows()
    assert row.tile_of(3 * case.P) >= g.MAX_TILES_PER_LAUNCH > row.tile_of(2 * case.P + g.TX_PACKET)
    # the idle slot's 1880 samples lie in tiles of the first launch that hold periods and no packet
    t = row.tile_of(case.P)
    assert t < g.MAX_TILES_PER_LAUNCH and not row.in_gap[t] and row.starts[t] == 1
    assert (row.in_gap & row.whole).sum() > 80_000
    msg = masked.locate(0, case.P + 7)
    assert "slot 1 sample 7" in msg and "active 1011" in msg and "idle at own index 1" in msg
    msg = masked.locate(0, 3 * case.P)
    assert "launch 1" in msg and "active 11--" in msg and "sends its packet 2" in msg


def test_the_masked_rows_past_4_gib():
    assert mg.ROWS4G_MASK.tolist() == [[1, 1], [0, 1], [1, 0]]
    for name in ("rows4g_s16", "rows4g_alaw"):
        case = CASES[name]
        assert case is g.CASES[name] and case.nch == 3 and case.npk == 2
        masked = Masked(case, mg.ROWS4G_MASK)
        assert [masked.first_slot(c) for c in range(3)] == [0, 1, 0]
        assert masked.index[:, -1].tolist() == [2, 1, 1]


def test_the_other_cases():
    assert CASES["s16_gap168"].P == g.TILE and (CASES["s16_gap168"].nch, CASES["s16_gap168"].npk) == (8, 12)
    for nch in g.GRID_X_NCH:
        case = CASES[f"gridx_{nch}"]
        assert (case.nch, case.npk, case.gap) == (nch, 4, 903) and case.ld % 2 == 1
        assert {r.a for r in case.rows()} == set(range(8))
    assert set(g.GRID_X_NCH) == {8, 127, 128, 129, 257}
    for name in ("calls41_gap903", "calls41_gap0", "mixed_gap903", "mixed_gap0"):
        assert CASES[name] is g.CASES[name]


def test_locate_names_the_window_and_the_own_index():
    masked, _ = mg.sweep_case("s16_gap0")
    case = masked.case
    c, k = 21, 100
    msg = masked.locate(c, k * case.P + 44)
    assert case.locate(c, k * case.P + 44) in msg
    bits = "".join(str(int(b)) for b in mg.DE_BRUIJN[(k - 1 + c // 8 + np.arange(4)) % 16])
    assert f"slot {k} sample 44, slots {k - 1}..{k + 2} active {bits}" in msg
    own = int(masked.index[c, 0] + (masked.mask[c, :k] != 0).sum())
    assert msg.endswith(("sends its packet" if masked.mask[c, k] else "idle at own index") + f" {own}")
    assert masked.window(0, 0).startswith("-") and masked.window(0, case.npk - 1).endswith("--")
    assert "behind" in masked.locate(0, case.n)
    j = mg.join_case(903)
    k0 = j.first_slot(9)
    assert f"sends its packet 0" in j.locate(9, k0 * j.case.P) and "idle at own index 0" in j.locate(9, k0 * j.case.P - 1)
