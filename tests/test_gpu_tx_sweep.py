"""tx_batch_kernel (singlecarrier_amd/csrc/qpsk_tx.hip) at every tile cut and
past its launch limits.  The cases are tests/tx_geometry.py's CASES, whose
coverage tests/test_tx_geometry.py asserts on the CPU for exactly the
addresses used here; this file runs them and compares the whole destination
buffer (the guard in front, the rows, the row tails, the guard behind) with
the host twin sc.tx_batch_host, which tests/test_tx_batch.py pins to the
oracle and the reference over 2,049 packets.  Exact equality everywhere; a
failure names the tile of the first wrong element and its class.  The block,
the calls and the comparison are tests/tx_sweep_run.py's, shared with the
sweep of the general context (tests/test_gpu_tx_mask_sweep.py).  Run with
-m gpu."""
import numpy as np
import pytest

import singlecarrier_amd as sc
import tx_geometry as g
import tx_sweep_run as run
from tx_geometry import CASES
from tx_sweep_run import FMT, Block, expected, payload, send

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def run_case(name, enc, seed):
    run.run_case(name, CASES[name], enc, seed)


# ------------------------------------------------------------------ every cut
@pytest.mark.parametrize("name", ["s16_gap0", "s16_gap1", "s16_gap903"])
def test_every_cut_int16(name):
    """8 rows of the 8 alignments, one packet more than it takes for their cuts
    together to fall on every residue of the packet period"""
    run_case(name, sc.OUT_S16, 1)


def test_every_cut_over_the_channel_loop():
    """the gap 903 sweep with 136 channels: a block of the first 128 loops over
    16 rows of its alignment, so both LDS tiles and all 16 sign strings meet
    every cut; the last 8 channels are blocks of one row"""
    run_case("s16_gap903_136ch", sc.OUT_S16, 8)


@pytest.mark.parametrize("name", ["alaw_gap903", "ulaw_gap1"])
def test_every_cut_fused_codes(name):
    """the same kernel's 8-byte store pass, rows at all 8 byte offsets"""
    run_case(name, FMT[name.split("_")[0]], 2)


@pytest.mark.parametrize("name", ["s16_gap2903", "s16_gap168"])
def test_gaps_that_hold_whole_tiles(name):
    """tiles with no TX sample at all, some of them in the call's closing gap
    (at gap 2903 more than a sixth of all tiles are whole tiles of zeros), and
    the period that equals the tile"""
    cov = g.coverage(CASES[name].rows())
    assert cov["in_gap"] > 0 and cov["in_last_gap"] > 0
    run_case(name, sc.OUT_S16, 3)


# ------------------------------------------------------------------ calls that restart the grid
@pytest.mark.parametrize("gap", [903, 0])
@pytest.mark.parametrize("split", ["calls41", "mixed"])
def test_calls_restart_the_grid(split, gap):
    """41 packets in 41 calls of one, and in calls of 1, 2, 3, 5 and 30: the
    tile grid restarts at every call's out + k P (at gap 903 P is odd, so a
    row's calls take other alignments than the row), and every call but the
    first filters over the saved state.  Equal to the one-call result and the host
    twin; after a reset() mid-way the first call's block comes out again and
    the stream runs through from there."""
    case = CASES[f"{split}_gap{gap}"]
    one = g.Case(case.nch, case.npk, case.gap, addr16=case.addr16)
    assert one.ld == case.ld
    bits = payload(case, 4 + gap)
    want = expected(case, bits, sc.OUT_S16)
    d_bits = torch.from_numpy(bits).cuda()
    tx = sc.Transmitter(case.nch, gap=gap)
    try:
        whole = Block(one)
        send(tx, one, whole, d_bits, sc.OUT_S16)
        whole.expect(want)
        ref = whole.check(f"{split} gap {gap}: one call")
        tx.reset()
        block = Block(case)
        calls = list(case.calls)
        half = len(calls) // 2
        k = send(tx, case, block, d_bits, sc.OUT_S16, calls[:half])
        assert tx.packets() == k
        block.expect(want, 0, k)
        block.check(f"{split} gap {gap}: calls {calls[:half]}")
        tx.reset()
        assert tx.packets() == 0
        block.clear()
        k = send(tx, case, block, d_bits, sc.OUT_S16, calls[:1])
        block.expect(want, 0, k)
        block.check(f"{split} gap {gap}: the first call again after reset()")
        assert send(tx, case, block, d_bits, sc.OUT_S16, calls[1:], first=k) == case.npk
        assert tx.packets() == case.npk
        block.expect(want)
        got = block.check(f"{split} gap {gap}: calls {calls}")
        np.testing.assert_array_equal(got[block.start:block.start + block.body],
                                      ref[whole.start:whole.start + whole.body])
    finally:
        tx.close()


# ------------------------------------------------------------------ past the launch limits
@pytest.mark.parametrize("name", ["launch2_s16", "launch2_alaw"])
def test_more_than_65535_tiles(name):
    """one channel, 4 packets 45,000,000 zeros apart: 87,895 tiles, so the tile
    loop launches twice, and packet 3 lies in tile 65,920 of them"""
    case = CASES[name]
    row, = case.rows()
    assert row.lo.size > g.MAX_TILES_PER_LAUNCH and row.tile_of(3 * case.P) >= g.MAX_TILES_PER_LAUNCH
    run_case(name, FMT[name.split("_")[1]], 5)


@pytest.mark.parametrize("name", ["rows4g_s16", "rows4g_alaw"])
def test_row_offsets_past_2_to_32_bytes(name):
    """3 rows 2^31 + 1 int16 (2^32 + 1 codes) apart: row 1 starts past 4 GiB
    and row 2 past 8 GiB of the block.  The buffer is not filled: sentinels
    lie only around the three rows, each compared with its guards."""
    run.run_rows4g(name, CASES[name], FMT[name.split("_")[1]], 6)


@pytest.mark.parametrize("nch", g.GRID_X_NCH)
def test_grid_x_edges(nch):
    """a block row is 128 channels, 8 classes x 16 looped: one short of it,
    exactly it, one past it and one past two of them"""
    run_case(f"gridx_{nch}", sc.OUT_S16, 7)
