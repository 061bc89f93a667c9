"""tx_batch_kernel (singlecarrier_amd/csrc/qpsk_tx.hip) at every tile cut and
past its launch limits.  The cases are tests/tx_geometry.py's CASES, whose
coverage tests/test_tx_geometry.py asserts on the CPU for exactly the
addresses used here; this file runs them and compares the whole destination
buffer (the guard in front, the rows, the row tails, the guard behind) with
the host twin sc.tx_batch_host, which tests/test_tx_batch.py pins to the
oracle and the reference over 2,049 packets.  Exact equality everywhere; a
failure names the tile of the first wrong element and its class.  Run with
-m gpu."""
import numpy as np
import pytest

import singlecarrier_amd as sc
import tx_geometry as g
from g711 import CODES, compress
from tx_geometry import CASES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 64                                  # sentinel elements in front of and behind the block
SENT = {2: 0x5A5A, 1: 0xC3}
FMT = {"s16": sc.OUT_S16, "alaw": sc.OUT_ALAW, "ulaw": sc.OUT_ULAW}


def payload(case, seed):
    return np.random.default_rng(seed).integers(0, 2, (case.nch, case.npk, 8, 62), dtype=np.uint8)


def expected(case, bits, enc):
    """the host twin's samples [nch][n] as elements of the encoding"""
    host = sc.tx_batch_host(bits, gap=case.gap)
    assert host.shape == (case.nch, case.n)
    if enc == sc.OUT_S16:
        return host
    if case.gap < 100_000:
        return compress(host, enc)
    # nearly all gap: the code of 0 everywhere, the packets compressed one by one
    pk = host.reshape(case.nch, case.npk, case.P)
    assert not pk[:, :, g.TX_PACKET:].any()
    want = np.full(pk.shape, CODES[enc][32768], np.uint8)
    want[:, :, :g.TX_PACKET] = compress(pk[:, :, :g.TX_PACKET], enc)
    return want.reshape(case.nch, case.n)


class Block:
    """A case's destination inside a sentinel-filled device buffer, row 0 at
    case.addr16 bytes past a 16-byte boundary, and the host image of what the
    buffer is to hold."""

    def __init__(self, case):
        self.case, es = case, case.es
        self.dtype = torch.int16 if es == 2 else torch.uint8
        body = self.body = (case.nch - 1) * case.ld + case.n
        self.full = torch.full((GUARD + 16 + body + GUARD,), SENT[es], dtype=self.dtype, device="cuda")
        self.start = GUARD + ((case.addr16 - self.full.data_ptr() - GUARD * es) % 16) // es
        flat = self.full[self.start:self.start + body]
        self.rows = torch.as_strided(flat, (case.nch, case.n), (case.ld, 1), flat.storage_offset())
        # the addresses the CPU coverage test assumed
        assert self.rows.data_ptr() % 16 == case.addr16
        for c in (0, case.nch - 1):
            assert (self.rows[c].data_ptr() // es) % 8 == g.alignment(case.addr16, es, c, case.ld)
        self.image = np.full(self.full.numel(), SENT[es], np.int16 if es == 2 else np.uint8)

    def expect(self, want, first=0, last=None):
        """packets [first, last) of want [nch][n] into the image"""
        case = self.case
        lo, hi = first * case.P, (case.npk if last is None else last) * case.P
        for c in range(case.nch):
            s = self.start + c * case.ld
            self.image[s + lo:s + hi] = want[c, lo:hi]

    def clear(self):
        self.full.fill_(SENT[self.case.es])
        self.image[...] = SENT[self.case.es]

    def where(self, i):
        case = self.case
        e = i - self.start
        if e < 0:
            return f"{-e} elements in front of the block"
        c, p = divmod(e, case.ld)
        if c >= case.nch or (c == case.nch - 1 and p >= case.n):
            return f"{e - (case.nch - 1) * case.ld - case.n} elements behind the block"
        if p >= case.n:
            return f"channel {c}'s row tail, {p - case.n} elements behind its row"
        return case.locate(c, p)

    def check(self, what):
        torch.cuda.synchronize()
        got = self.full.cpu().numpy()
        bad = np.flatnonzero(got != self.image)
        if bad.size:
            i = int(bad[0])
            raise AssertionError(f"{what}: {bad.size} elements differ; the first, {int(got[i])} for {int(self.image[i])}, "
                                 f"at {self.where(i)}; the last at {self.where(int(bad[-1]))}")
        return got


def send(tx, case, block, d_bits, enc, calls=None, first=0):
    """the case's packets from `first` on in calls of `calls` packets, each at
    out + k * P"""
    k = first
    for n in (case.calls if calls is None else calls):
        part = d_bits[:, k:k + n].contiguous()
        out = block.rows[:, k * case.P:]
        if enc == sc.OUT_S16:
            tx.modulate_device(part, out)
        else:
            tx.modulate_device_fmt(part, out, enc | sc.OUT_PLANAR)
        k += n
    return k


def run_case(name, enc, seed):
    case = CASES[name]
    assert case.es == (2 if enc == sc.OUT_S16 else 1)
    bits = payload(case, seed)
    want = expected(case, bits, enc)
    block = Block(case)
    tx = sc.Transmitter(case.nch, gap=case.gap)
    try:
        assert send(tx, case, block, torch.from_numpy(bits).cuda(), enc) == case.npk
        tx.sync()
        assert tx.packets() == case.npk
        block.expect(want)
        block.check(name)
    finally:
        tx.close()


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
    case = CASES[name]
    enc, es = FMT[name.split("_")[1]], case.es
    count = GUARD + 16 + (case.nch - 1) * case.ld + case.n + GUARD
    if torch.cuda.mem_get_info()[0] < count * es + 6 * 2**30:
        pytest.skip(f"needs about {count * es / 1e9:.0f} GB of device memory")
    bits = payload(case, 6)
    want = expected(case, bits, enc)
    full = flat = rows = tx = None
    try:
        full = torch.empty(count, dtype=torch.int16 if es == 2 else torch.uint8, device="cuda")
        start = GUARD + ((case.addr16 - full.data_ptr() - GUARD * es) % 16) // es
        for c in range(case.nch):
            full[start + c * case.ld - GUARD:start + c * case.ld + case.n + GUARD] = SENT[es]
        flat = full[start:start + (case.nch - 1) * case.ld + case.n]
        rows = torch.as_strided(flat, (case.nch, case.n), (case.ld, 1), flat.storage_offset())
        assert rows.data_ptr() % 16 == case.addr16
        assert rows[1].data_ptr() - rows[0].data_ptr() > 2**32 and rows[2].data_ptr() - rows[0].data_ptr() > 2**33
        tx = sc.Transmitter(case.nch, gap=case.gap)
        d_bits = torch.from_numpy(bits).cuda()
        if enc == sc.OUT_S16:
            tx.modulate_device(d_bits, rows)
        else:
            tx.modulate_device_fmt(d_bits, rows, enc | sc.OUT_PLANAR)
        tx.sync()
        for c in range(case.nch):
            got = full[start + c * case.ld - GUARD:start + c * case.ld + case.n + GUARD].cpu().numpy()
            image = np.full(got.size, SENT[es], got.dtype)
            image[GUARD:GUARD + case.n] = want[c]
            bad = np.flatnonzero(got != image)
            assert bad.size == 0, (f"{name}: row {c}, {bad.size} elements differ, the first at "
                                   + (case.locate(c, int(bad[0]) - GUARD) if GUARD <= bad[0] < GUARD + case.n
                                      else f"guard element {int(bad[0]) - GUARD}"))
    finally:
        if tx is not None:
            tx.close()
        del full, flat, rows
        torch.cuda.empty_cache()


@pytest.mark.parametrize("nch", g.GRID_X_NCH)
def test_grid_x_edges(nch):
    """a block row is 128 channels, 8 classes x 16 looped: one short of it,
    exactly it, one past it and one past two of them"""
    run_case(f"gridx_{nch}", sc.OUT_S16, 7)
