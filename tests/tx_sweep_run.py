"""What the transmitter's sweeps (tests/test_gpu_tx_sweep.py on a uniform
context, tests/test_gpu_tx_mask_sweep.py on a general one) share: a case of
tests/tx_geometry.py as a destination block inside a sentinel-filled device
buffer, the calls that fill it, the host twin's samples as the elements of the
encoding, and the comparison of the whole buffer (the guard in front, the rows,
the row tails, the guard behind), exact, with the tile of the first wrong
element in the message.

Every helper takes an optional mask [nch][npk] (nonzero: the channel sends in
that slot; None: the plain call), and run_case a context and a host twin made
beforehand (tx_mask_cases.Twin), so that a case may follow other calls.

Plain module: torch is imported when a function is called, never at import.
"""
import numpy as np

import singlecarrier_amd as sc
import tx_geometry as g
from g711 import CODES, compress

GUARD = 64                                  # sentinel elements in front of and behind the block
SENT = {2: 0x5A5A, 1: 0xC3}
FMT = {"s16": sc.OUT_S16, "alaw": sc.OUT_ALAW, "ulaw": sc.OUT_ULAW}


def payload(case, seed):
    return np.random.default_rng(seed).integers(0, 2, (case.nch, case.npk, 8, 62), dtype=np.uint8)


def expected(case, bits, enc, mask=None, twin=None):
    """the host twin's samples [nch][n] as elements of the encoding; `twin`
    (tx_mask_cases.Twin) continues its own states, None starts every channel
    afresh"""
    host = sc.tx_batch_host(bits, gap=case.gap, active=mask) if twin is None else twin.call(bits, case.gap, mask)
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
    buffer is to hold.  `locate(c, p)` says where position p of channel c's row
    lies (default: the case's own)."""

    def __init__(self, case, locate=None):
        import torch
        self.case, es = case, case.es
        self.locate = locate or case.locate
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
        return self.locate(c, p)

    def check(self, what):
        import torch
        torch.cuda.synchronize()
        got = self.full.cpu().numpy()
        bad = np.flatnonzero(got != self.image)
        if bad.size:
            i = int(bad[0])
            raise AssertionError(f"{what}: {bad.size} elements differ; the first, {int(got[i])} for {int(self.image[i])}, "
                                 f"at {self.where(i)}; the last at {self.where(int(bad[-1]))}")
        return got


def call(tx, d_bits, out, enc, d_mask=None):
    """one device call of the planar encoding into the rows `out`"""
    if enc == sc.OUT_S16:
        tx.modulate_device(d_bits, out, active=d_mask)
    else:
        tx.modulate_device_fmt(d_bits, out, enc | sc.OUT_PLANAR, active=d_mask)


def send(tx, case, block, d_bits, enc, calls=None, first=0, d_mask=None):
    """the case's packets from `first` on in calls of `calls` packets, each at
    out + k * P, each with its columns of the mask"""
    k = first
    for n in (case.calls if calls is None else calls):
        part = d_bits[:, k:k + n].contiguous()
        call(tx, part, block.rows[:, k * case.P:], enc, None if d_mask is None else d_mask[:, k:k + n].contiguous())
        k += n
    return k


def run_case(name, case, enc, seed, mask=None, tx=None, twin=None, locate=None):
    """The case's packets into a Block and the comparison with the host twin.
    With `tx` (and the `twin` that took the same calls) the case follows what
    that context has sent and the context stays open; otherwise a fresh one.
    Returns the twin's rows."""
    import torch
    assert case.es == (2 if enc == sc.OUT_S16 else 1)
    assert (tx is None) == (twin is None)
    bits = payload(case, seed)
    want = expected(case, bits, enc, mask, twin)
    block = Block(case, locate)
    own = tx is None
    if own:
        tx = sc.Transmitter(case.nch, gap=case.gap)
    try:
        before = tx.packets()
        d_mask = None if mask is None else torch.from_numpy(mask).cuda()
        assert send(tx, case, block, torch.from_numpy(bits).cuda(), enc, d_mask=d_mask) == case.npk
        tx.sync()
        assert tx.packets() == before + case.npk
        block.expect(want)
        block.check(name)
    finally:
        if own:
            tx.close()
    return want


def run_rows4g(name, case, enc, seed, mask=None, locate=None):
    """3 rows 2^31 + 1 int16 (2^32 + 1 codes) apart.  The buffer is not
    filled: sentinels lie only around the three rows, each compared with its
    guards.  Skips where the device has not that much memory free; never
    shrunk."""
    import pytest
    import torch
    es = case.es
    locate = locate or case.locate
    count = GUARD + 16 + (case.nch - 1) * case.ld + case.n + GUARD
    if torch.cuda.mem_get_info()[0] < count * es + 6 * 2**30:
        pytest.skip(f"needs about {count * es / 1e9:.0f} GB of device memory")
    bits = payload(case, seed)
    want = expected(case, bits, enc, mask)
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
        call(tx, torch.from_numpy(bits).cuda(), rows, enc, None if mask is None else torch.from_numpy(mask).cuda())
        tx.sync()
        for c in range(case.nch):
            got = full[start + c * case.ld - GUARD:start + c * case.ld + case.n + GUARD].cpu().numpy()
            image = np.full(got.size, SENT[es], got.dtype)
            image[GUARD:GUARD + case.n] = want[c]
            bad = np.flatnonzero(got != image)
            assert bad.size == 0, (f"{name}: row {c}, {bad.size} elements differ, the first at "
                                   + (locate(c, int(bad[0]) - GUARD) if GUARD <= bad[0] < GUARD + case.n
                                      else f"guard element {int(bad[0]) - GUARD}"))
    finally:
        if tx is not None:
            tx.close()
        del full, flat, rows
        torch.cuda.empty_cache()
