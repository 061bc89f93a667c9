"""Where tx_batch_kernel cuts a row, from its documented contract
(singlecarrier_amd/csrc/qpsk_tx.hip, header comment): a channel's row of one
call is a flat stream of npackets * P elements, P = 1880 + gap; a block owns
TILE = 2048 elements of it, cut at addresses aligned to CHUNK = 8 elements
(16 bytes of int16, 8 bytes of G.711 codes), not at packet boundaries; row c
of a call that starts k packets into the block starts at element
out + c * ld + k * P, and its alignment a is that element index mod 8.

Plain module, integer arithmetic on numpy arrays; no GPU import and nothing of
the kernel's index arithmetic (tlo, thi, nper, LDS slots).  It answers two
questions:

  * which tile edges does a case reach (tests/test_tx_geometry.py asserts, on
    the CPU, that the cases below reach what tests/test_gpu_tx_sweep.py says
    they sweep: these are conditions on the inputs);
  * which tile, of which class, holds a given element (the GPU tests put that
    into the message of a failed comparison).

Case            what a GPU test sends: channels, packets, gap, the address of
                row 0's first element mod 16 bytes, the row stride, the element
                size and the packets of each call.
Case.rows()     one Row per (channel, call): its alignment and its tiles as
                arrays lo[], hi[] (positions of the call's row, clipped to it)
                with their classes.
coverage(rows)  what a list of rows reaches.
packets_for_every_residue(gap)
                the fewest packets of one call after which the cuts of 8 rows,
                one of each alignment, have fallen on every lo mod P (a row's
                start, tile 0, is no cut).
CASES           the sweeps of tests/test_gpu_tx_sweep.py by name.

At the end, what tests/test_tx_batch.py and tests/test_gpu_tx.py share: the
reference-made golden as a payload, and a payload as the reference's
transmitter calls (golden_payload, packet_calls, with_gaps).
"""
import functools
import os
from dataclasses import dataclass

import numpy as np

import oracle

TX_PACKET = 1880      # transmitted samples of a packet; the gap follows them
TILE = 2048           # elements of a row per block
CHUNK = 8             # elements of one aligned store
NEAR = 5              # "near" a packet's start or its sample 1880: within +-5 elements
MAX_TILES_PER_LAUNCH = 65535   # grid.y of one launch of the tile loop


def alignment(addr16, es, c, ld, start=0):
    """elements from the start of row c (ld apart, `start` elements into the
    block, the block addr16 bytes past a 16-byte boundary) back to a boundary
    of CHUNK elements"""
    assert addr16 % es == 0 and 0 <= addr16 < 16
    return (addr16 // es + c * ld + start) % CHUNK


def tile_edges(a, n):
    """(lo[], hi[]) of the tiles of a row of n elements with alignment a: tile
    t is [t * TILE - a, (t + 1) * TILE - a) clipped to [0, n)"""
    assert 0 <= a < CHUNK and n > 0
    ntile = (n + a + TILE - 1) // TILE
    t = np.arange(ntile, dtype=np.int64)
    lo = np.maximum(t * TILE - a, 0)
    hi = np.minimum((t + 1) * TILE - a, n)
    assert (hi > lo).all() and lo[0] == 0 and hi[-1] == n
    return lo, hi


def _near(e, P, what):
    """edge e within NEAR elements of a packet start (what = 0) or of a
    packet's sample 1880 (what = TX_PACKET)"""
    d = (e - what) % P
    return np.minimum(d, P - d) <= NEAR


class Row:
    """One channel's row of one call: its alignment a, its tiles lo[], hi[]
    (positions of the call's row) and, per tile, the classes below."""

    def __init__(self, channel, call, first_packet, npk, P, a, stream_start):
        self.channel, self.call, self.npk, self.P, self.a = channel, call, npk, P, a
        self.first_packet = first_packet      # packets of the block in front of this call
        self.stream_start = stream_start      # the call is the stream's first: no saved history
        lo, hi = self.lo, self.hi = tile_edges(a, npk * P)
        self.residue = lo % P
        # an edge the kernel cuts inside the row; tile 0 starts where the row does
        self.cut = lo > 0
        # packet starts k * P with lo <= k * P < hi
        self.starts = (hi + P - 1) // P - (lo + P - 1) // P
        self.in_gap = (self.residue >= TX_PACKET) & (hi <= (lo // P + 1) * P)
        self.near_start = _near(lo, P, 0) | _near(hi, P, 0)
        self.near_end = _near(lo, P, TX_PACKET) | _near(hi, P, TX_PACKET)
        self.first = ~self.cut & stream_start
        self.last = hi == npk * P
        self.ragged = self.last & (hi - lo < TILE)
        self.whole = hi - lo == TILE
        # a tile wholly inside the gap that closes the call
        self.in_last_gap = self.in_gap & (lo >= (npk - 1) * P)

    def tile_of(self, p):
        """index of the tile that holds position p of this call's row"""
        return int((p + self.a) // TILE)

    def describe(self, t):
        cls = [f"{int(self.starts[t])} packet starts"]
        for name in ("in_gap", "near_start", "near_end", "first", "last", "ragged"):
            if getattr(self, name)[t]:
                cls.append(name)
        return (f"channel {self.channel} call {self.call} (packets {self.first_packet}..{self.first_packet + self.npk - 1}"
                f", a = {self.a}) tile {t} = [{int(self.lo[t])}, {int(self.hi[t])}) launch {t // MAX_TILES_PER_LAUNCH}"
                f", lo mod P = {int(self.residue[t])}: " + ", ".join(cls))


@dataclass(frozen=True)
class Case:
    nch: int
    npk: int
    gap: int
    addr16: int = 0           # address of row 0's first element mod 16 bytes
    tail: int = 2             # ld = npk * P + tail, or one more where that is even: ld is odd
    es: int = 2               # bytes of an element: int16 samples or G.711 codes
    splits: tuple = None      # packets of each call; None = one call
    ld_fixed: int = None      # a row stride given outright (the 2^32-byte cases)

    @property
    def P(self):
        return TX_PACKET + self.gap

    @property
    def n(self):
        return self.npk * self.P

    @property
    def ld(self):
        if self.ld_fixed is not None:
            return self.ld_fixed
        return (self.n + self.tail) | 1

    @property
    def calls(self):
        s = self.splits or (self.npk,)
        assert sum(s) == self.npk and min(s) > 0
        return s

    def _calls_of(self, c):
        """channel c's Row of every call"""
        k = 0
        for j, n in enumerate(self.calls):
            yield Row(c, j, k, n, self.P, alignment(self.addr16, self.es, c, self.ld, k * self.P), j == 0)
            k += n

    def rows(self, channels=None):
        return [r for c in (range(self.nch) if channels is None else channels) for r in self._calls_of(c)]

    def locate(self, c, p):
        """the tile that holds position p of channel c's row of the block, said
        in words"""
        for row in self._calls_of(c):
            q = p - row.first_packet * self.P
            if q < row.npk * self.P:
                return f"position {p}: " + row.describe(row.tile_of(q))
        return f"position {p}: behind the row's {self.n} elements"


def coverage(rows):
    """what the tiles of `rows` (one gap) reach.  Residues count cuts only, the
    lower edges of tiles 1, 2, ...: tile 0 starts where its row does, at
    residue 0 whatever the alignment, and is counted under `first`."""
    P = rows[0].P
    cat = lambda name: np.concatenate([getattr(r, name) for r in rows])
    res, starts = cat("residue"), cat("starts")
    seen = np.zeros(P, bool)
    seen[res[cat("cut")]] = True
    return {
        "P": P,
        "tiles": int(res.size),
        "residues": int(seen.sum()),
        "every_residue": bool(seen.all()),
        "alignments": sorted({r.a for r in rows}),
        "starts": {int(s): int((starts == s).sum()) for s in np.unique(starts)},
        "in_gap": int(cat("in_gap").sum()),
        "in_last_gap": int(cat("in_last_gap").sum()),
        "whole_in_gap": int((cat("in_gap") & cat("whole")).sum()),
        "whole_in_last_gap": int((cat("in_last_gap") & cat("whole")).sum()),
        "near_start": int(cat("near_start").sum()),
        "near_end": int(cat("near_end").sum()),
        "first": int(cat("first").sum()),
        "ragged": int(cat("ragged").sum()),
        "whole_last": int((cat("last") & ~cat("ragged")).sum()),
        "launches": max((r.lo.size + MAX_TILES_PER_LAUNCH - 1) // MAX_TILES_PER_LAUNCH for r in rows),
    }


@functools.lru_cache(maxsize=None)
def packets_for_every_residue(gap):
    """the fewest packets of one call after which the cuts of 8 rows, one per
    alignment 0..7, have fallen on every residue 0..P-1 of the packet period;
    None where they never do.  Tile t > 0 of alignment a starts at t * TILE - a
    whatever the row's length, so the answer is the packet that holds the last
    residue's first cut.  Tile 0 is no cut: residue 0 counts only where a
    later tile starts on a packet's first sample."""
    P = TX_PACKET + gap
    # t * TILE mod P repeats after P / gcd tiles: looking further finds nothing new
    t = np.arange(1, P + 1, dtype=np.int64)
    first = np.full(P, np.iinfo(np.int64).max)
    for a in range(CHUNK):
        lo = t * TILE - a
        np.minimum.at(first, lo % P, lo)
    if (first == np.iinfo(np.int64).max).any():
        return None
    return int(first.max() // P + 1)


def _sweep(gap, **kw):
    return Case(8, packets_for_every_residue(gap) + 1, gap, **kw)


# 2^31 + 1 int16 and 2^32 + 1 codes: rows 1 and 2 start past 2^32 and 2^33 bytes
LD_S16_4G = 2**31 + 1
LD_CODE_4G = 2**32 + 1
CALLS_41 = (1,) * 41
CALLS_MIXED = (1, 2, 3, 5, 30)

# One row per alignment class unless said otherwise: 8 channels an odd ld apart.  The block
# of an int16 case starts 2 bytes past a 16-byte boundary and that of a code
# case 3 bytes past one, so no row of either is aligned by accident of the
# allocator; with odd ld the 8 rows still take every alignment 0..7.
CASES = {
    "s16_gap0": _sweep(0, addr16=2),
    "s16_gap1": _sweep(1, addr16=2),
    "s16_gap903": _sweep(903, addr16=2),
    "alaw_gap903": _sweep(903, addr16=3, es=1),
    "ulaw_gap1": _sweep(1, addr16=3, es=1),
    "s16_gap2903": _sweep(2903, addr16=2),
    # the gap 903 sweep over 136 channels: 17 rows per alignment, so the blocks of the
    # first 128 channels loop over 16 rows (both LDS tiles, 16 sign strings) at every cut
    "s16_gap903_136ch": Case(136, packets_for_every_residue(903) + 1, 903, addr16=2),
    "s16_gap168": Case(8, 12, 168, addr16=2),     # P == TILE: one residue per row, no coverage claim
    "calls41_gap903": Case(8, 41, 903, addr16=2, splits=CALLS_41),
    "calls41_gap0": Case(8, 41, 0, addr16=2, splits=CALLS_41),
    "mixed_gap903": Case(8, 41, 903, addr16=2, splits=CALLS_MIXED),
    "mixed_gap0": Case(8, 41, 0, addr16=2, splits=CALLS_MIXED),
    "launch2_s16": Case(1, 4, 45_000_000, addr16=2),
    "launch2_alaw": Case(1, 4, 45_000_000, addr16=3, es=1),
    "rows4g_s16": Case(3, 2, 903, addr16=2, ld_fixed=LD_S16_4G),
    "rows4g_alaw": Case(3, 2, 903, addr16=3, es=1, ld_fixed=LD_CODE_4G),
}
GRID_X_NCH = (8, 127, 128, 129, 257)   # a block row is 128 channels: 8 classes x 16 looped
for _nch in GRID_X_NCH:
    CASES[f"gridx_{_nch}"] = Case(_nch, 2, 903, addr16=2)


# ---------------------------------------------------------------- payloads and the reference's calls
def golden_payload(golden_dir):
    """tx_golden.npz (three packets back to back, 27 transmitter calls, no gap)
    as a payload [1][3][8][62] and its samples: I-bit = re < 0, Q-bit = im < 0,
    bits[2s] = Q, bits[2s+1] = I."""
    g = np.load(os.path.join(golden_dir, "tx_golden.npz"))
    assert list(g["lengths"]) == [128] + [31] * 8 + [128] + [31] * 8 + [128] + [31] * 8
    syms = np.split(g["symbols"], np.cumsum(g["lengths"])[:-1])
    bits = np.zeros((1, 3, 8, 62), np.uint8)
    for n, (s, pre) in enumerate(zip(syms, g["preamble"])):
        assert bool(pre) == (n % 9 == 0)
        if not pre:
            bits[0, n // 9, n % 9 - 1, 0::2] = s.imag < 0
            bits[0, n // 9, n % 9 - 1, 1::2] = s.real < 0
    return bits, g["samples"]


def packet_calls(bits):
    """One channel's payload [npackets][8][62] as the transmitter calls of the
    reference's main(): [(symbols, is_preamble), ...], 9 per packet."""
    pre = oracle.preamble().astype(np.float32)
    calls = []
    for pk in bits:
        calls.append((pre + 1j * pre, True))
        for fr in pk:
            i = np.where(fr[1::2] == 1, -1.0, 1.0)
            q = np.where(fr[0::2] == 1, -1.0, 1.0)
            calls.append(((i + 1j * q).astype(np.complex64), False))
    return calls


def with_gaps(calls_out, gap):
    """The samples of a list of per-call outputs with `gap` zeros after every
    9th call (the reference fwrites them, src/qpsk.c:410-412)."""
    parts = []
    for n, o in enumerate(calls_out):
        parts.append(o)
        if n % 9 == 8:
            parts.append(np.zeros(gap, np.int16))
    return np.concatenate(parts)
