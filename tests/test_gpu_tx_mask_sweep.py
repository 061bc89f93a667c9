"""tx_plan_kernel and tx_mask_kernel (singlecarrier_amd/csrc/qpsk_tx.hip), the
transmitter of a general context, at every tile cut under every pattern of
active and idle slots around the cut, with channels that send their first
packet ever in a slot a tile cuts, over calls that restart the tile grid, and
past the launch limits.  The cases are tests/tx_mask_geometry.py's, whose
coverage tests/test_tx_mask_geometry.py asserts on the CPU for exactly the
addresses and masks used here; this file runs them and compares the whole
destination buffer (the guard in front, the rows, the row tails, the guard
behind) with the host twin qpsk_tx_batch_masked_host, which
tests/test_tx_mask_host.py pins to an independent restatement on these masks.
Exact equality everywhere; a failure names the tile of the first wrong
element, its class, the activity of the slots around it and the channel's own
index there.  Run with -m gpu."""
import numpy as np
import pytest

import singlecarrier_amd as sc
import tx_geometry as g
import tx_mask_geometry as mg
import tx_sweep_run as run
from g711 import compress
from tx_mask_cases import Restated, Twin, payload
from tx_mask_geometry import CASES, Masked
from tx_sweep_run import FMT, SENT, Block, expected, send

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def plain_call(tx, twin, bits, enc, mask=None):
    """one call in front of a case, on the context and the twin, into a block
    of its own with 5 sentinels behind every row; compared like the case"""
    nch, npk = bits.shape[:2]
    n = npk * (g.TX_PACKET + tx.gap)
    es = 2 if enc == sc.OUT_S16 else 1
    want = np.full((nch, n + 5), SENT[es], np.int16 if es == 2 else np.uint8)
    y = twin.call(bits, tx.gap, mask)
    want[:, :n] = y if enc == sc.OUT_S16 else compress(y, enc)
    out = torch.full((nch, n + 5), SENT[es], dtype=torch.int16 if es == 2 else torch.uint8, device="cuda")
    run.call(tx, torch.from_numpy(bits).cuda(), out, enc, None if mask is None else torch.from_numpy(mask).cuda())
    tx.sync()
    np.testing.assert_array_equal(out.cpu().numpy(), want)


# ------------------------------------------------------------------ every cut x every window
@pytest.mark.parametrize("name", ["s16_gap903", "s16_gap0", "alaw_gap903"])
def test_every_cut_under_every_window(name):
    """136 rows, 17 of each alignment, whose masks are the 16 shifts of the de
    Bruijn sequence B(2, 4): every residue of the packet period is cut under
    every pattern of the 4 slots around the cut, and the 16 channels of a block's
    loop disagree about every slot.  A masked call of 12 slots goes first, so
    own indices 0 .. 12 (carrier rows 0 .. 8, both signs, the crossing from 8
    to 9 at another slot in every channel) share each loop."""
    masked, pre = mg.sweep_case(name)
    case, enc, seed = masked.case, FMT[name.split("_")[0]], mg.SWEEP_SEED[name]
    twin, tx = Twin(case.nch), sc.Transmitter(case.nch, gap=case.gap)
    try:
        plain_call(tx, twin, payload(seed + 2, case.nch, mg.PREROLL), enc, pre)
        np.testing.assert_array_equal(tx.channel_packets(), masked.index[:, 0].astype(np.uint64))
        run.run_case(name, case, enc, seed + 3, masked.mask, tx, twin, masked.locate)
        np.testing.assert_array_equal(tx.channel_packets(), masked.index[:, -1].astype(np.uint64))
        assert tx.packets() == mg.PREROLL + case.npk
    finally:
        tx.close()


# ------------------------------------------------------------------ joins at a cut
@pytest.mark.parametrize("stale", [False, True], ids=["fresh", "after_reset"])
@pytest.mark.parametrize("gap", [903, 0])
def test_joins_at_a_cut(gap, stale):
    """Every cut within a slot's first 50 samples lies in a row that sends its
    first packet ever in that slot: the zero filter memory of a stream's first
    9 periods begins or ends inside a tile.  Once on a fresh context, once after
    3 slots sent by everyone and reset_channels on every channel: the state
    words under the joins are stale then and must not reach those samples."""
    masked = mg.join_case(gap)
    case = masked.case
    twin, tx = Twin(case.nch), sc.Transmitter(case.nch, gap=gap)
    try:
        if stale:
            plain_call(tx, twin, payload(31 + gap, case.nch, 3), sc.OUT_S16)
            np.testing.assert_array_equal(tx.channel_packets(), np.full(case.nch, 3, np.uint64))
            tx.reset_channels(0, case.nch)
            twin.reset(0, case.nch)
            assert not tx.channel_packets().any()
        want = run.run_case(f"joins gap {gap}", case, sc.OUT_S16, 32 + gap, masked.mask, tx, twin, masked.locate)
        np.testing.assert_array_equal(tx.channel_packets(), masked.index[:, -1].astype(np.uint64))
        # and the twin is the restatement here: each channel a fresh transmitter fed its own packets
        rest = Restated(case.nch).call(run.payload(case, 32 + gap), gap, masked.mask != 0)
        np.testing.assert_array_equal(want, rest)
    finally:
        tx.close()


# ------------------------------------------------------------------ P equal to the tile
def test_a_period_equal_to_the_tile():
    case = CASES["s16_gap168"]
    masked = Masked(case, mg.random_mask(41, case.nch, case.npk))
    run.run_case("s16_gap168", case, sc.OUT_S16, 42, masked.mask, locate=masked.locate)


# ------------------------------------------------------------------ calls that restart the grid
@pytest.mark.parametrize("gap", [903, 0])
@pytest.mark.parametrize("split", ["calls41", "mixed"])
def test_calls_restart_the_grid_on_a_general_context(split, gap):
    """41 slots under a random mask in 41 calls of one, and in calls of 1, 2,
    3, 5 and 30: every call's plan starts from the saved words and own indices
    (a row whose last active slot is not its call's last among them), and the
    tile grid restarts at out + k P.  Equal to the one-call result and the host
    twin; after reset() the context is uniform again and the plain first call
    comes out."""
    case = CASES[f"{split}_gap{gap}"]
    one = g.Case(case.nch, case.npk, case.gap, addr16=case.addr16)
    assert one.ld == case.ld
    masked = Masked(case, mg.random_mask(50 + gap, case.nch, case.npk))
    mask, sent = masked.mask, masked.index[:, -1].astype(np.uint64)
    bits = run.payload(case, 51 + gap)
    want = expected(case, bits, sc.OUT_S16, mask)
    d_bits, d_mask = torch.from_numpy(bits).cuda(), torch.from_numpy(mask).cuda()
    tx = sc.Transmitter(case.nch, gap=gap)
    try:
        whole = Block(one, Masked(one, mask).locate)
        send(tx, one, whole, d_bits, sc.OUT_S16, d_mask=d_mask)
        whole.expect(want)
        ref = whole.check(f"{split} gap {gap}: one call")
        np.testing.assert_array_equal(tx.channel_packets(), sent)
        tx.reset()
        block = Block(case, masked.locate)
        assert send(tx, case, block, d_bits, sc.OUT_S16, d_mask=d_mask) == case.npk
        assert tx.packets() == case.npk
        np.testing.assert_array_equal(tx.channel_packets(), sent)
        block.expect(want)
        got = block.check(f"{split} gap {gap}: calls {list(case.calls)}")
        np.testing.assert_array_equal(got[block.start:block.start + block.body],
                                      ref[whole.start:whole.start + whole.body])
        # uniform again: the plain first call, every channel a fresh stream
        tx.reset()
        assert tx.packets() == 0 and not tx.channel_packets().any()
        block.clear()
        k = send(tx, case, block, d_bits, sc.OUT_S16, case.calls[:1])
        block.expect(expected(case, bits, sc.OUT_S16), 0, k)
        block.check(f"{split} gap {gap}: the plain first call after reset()")
        np.testing.assert_array_equal(tx.channel_packets(), np.full(case.nch, k, np.uint64))
    finally:
        tx.close()


# ------------------------------------------------------------------ past the launch limits
@pytest.mark.parametrize("name", ["launch2_s16", "launch2_alaw"])
def test_more_than_65535_tiles_masked(name):
    """one channel, slots 45,000,000 zeros apart, active 1, 0, 1, 1: packet 3
    lies in the tile loop's second launch, the idle slot's 1880 samples are a
    tile with periods and no packet, and nearly every tile is all gap"""
    case = CASES[name]
    masked = Masked(case, mg.LAUNCH2_MASK)
    run.run_case(name, case, FMT[name.split("_")[1]], 5, masked.mask, locate=masked.locate)


@pytest.mark.parametrize("name", ["rows4g_s16", "rows4g_alaw"])
def test_row_offsets_past_2_to_32_bytes_masked(name):
    """3 rows 2^31 + 1 int16 (2^32 + 1 codes) apart, active [[1, 1], [0, 1],
    [1, 0]]: the rows past 4 and 8 GiB hold a join in the call's second slot
    and an idle last slot"""
    case = CASES[name]
    masked = Masked(case, mg.ROWS4G_MASK)
    run.run_rows4g(name, case, FMT[name.split("_")[1]], 6, masked.mask, masked.locate)


@pytest.mark.parametrize("nch", g.GRID_X_NCH)
def test_grid_x_edges_masked(nch):
    """a block row is 128 channels, 8 classes x 16 looped: one short of it,
    exactly it, one past it and one past two of them, 4 slots, random mask"""
    case = CASES[f"gridx_{nch}"]
    masked = Masked(case, mg.random_mask(60 + nch, nch, case.npk))
    run.run_case(f"gridx_{nch}", case, sc.OUT_S16, 7, masked.mask, locate=masked.locate)
