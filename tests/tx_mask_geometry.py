"""Where tx_mask_kernel's tile cuts fall relative to slots whose activity
differs from their neighbours': tests/tx_geometry.py (the tiles of a row, from
the documented contract) together with a mask [nch][npk], nonzero where the
channel sends in that slot (include/qpsk_tx.h "Channels that come and go").

Plain module, integer arithmetic on numpy arrays; no GPU import and nothing of
the kernel's index arithmetic or of its plan words.  A channel's own index is
counted from the mask alone.

sweep_mask()      row c, slot k active where B[(k + c // 8) % 16], B the de
                  Bruijn sequence B(2, 4): its 16 cyclic windows of 4 are the
                  16 patterns of 4 slots.  Rows an odd ld apart take alignment
                  class c mod 8 (in some order), so the 17 channels of a class
                  in a 136-channel case carry all 16 shifts, and the 16
                  channels one block loops over carry 16 different windows at
                  every slot.
pair_coverage()   for every cut (lower edge lo > 0 of a tile) in slot
                  k = lo // P with 1 <= k <= npk - 3: the pair (lo mod P, the
                  activity of slots k-1, k, k+1, k+2), as a bool [P][16].
packets_for_every_pair(gap)
                  the least npk at which a 136-channel sweep reaches all
                  P x 16 pairs.
cut_joins(), join_case()
                  the (alignment, slot) pairs whose slot is cut within its
                  first JOIN_SPAN samples (the first 9 symbol periods, whose
                  filter memory is zero in a channel's first packet, and a
                  little past them), and the case in which a channel of that
                  alignment sends its first packet ever in exactly that slot.
Masked            a Case with its mask and the own indices in front of it:
                  names the tile of an element, the 4-slot window around it
                  and the channel's own index there.
"""
import functools

import numpy as np

import tx_geometry as g
from tx_geometry import CHUNK, TILE, TX_PACKET, Case

DE_BRUIJN = np.array([0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1], np.uint8)
VALUES = np.array([1, 2, 0x80, 0xFF], np.uint8)     # what an active byte may hold: any nonzero
JOIN_SPAN = 50                                      # 9 periods of 5 samples, and 5 more
SWEEP_NCH = 136                                     # 8 classes x 17: one block column of 16 and a ragged second
PREROLL = 12                                        # slots of the call in front of a sweep


def _values(active, seed):
    """the activity [nch][npk] (0/1) as mask bytes: nonzero values of VALUES"""
    vals = np.random.default_rng(seed).choice(VALUES, active.shape)
    return np.where(active != 0, vals, 0).astype(np.uint8)


def sweep_mask(nch, npk, seed):
    c = np.arange(nch)[:, None]
    k = np.arange(npk)[None, :]
    return _values(DE_BRUIJN[(k + c // 8) % 16], seed)


def windows(mask):
    """int [nch][npk]: the activity of slots k-1, k, k+1, k+2 as 4 bits, slot
    k-1 the highest; slots outside the call count as idle"""
    act = np.pad((mask != 0).astype(np.int64), ((0, 0), (1, 2)))
    n = mask.shape[1]
    return act[:, 0:n] * 8 + act[:, 1:n + 1] * 4 + act[:, 2:n + 2] * 2 + act[:, 3:n + 3]


def pair_coverage(case, mask):
    """bool [P][16]: the (residue, window) pairs the cuts of a case reach in
    slots 1 .. npk - 3 of the block, where all four slots of the window lie
    inside it"""
    assert mask.shape == (case.nch, case.npk)
    P, npk = case.P, case.npk
    win = windows(mask)
    seen = np.zeros((P, 16), bool)
    for row in case.rows():
        k = row.lo // P + row.first_packet
        ok = row.cut & (k >= 1) & (k <= npk - 3)
        seen[row.residue[ok], win[row.channel, k[ok]]] = True
    return seen


@functools.lru_cache(maxsize=None)
def packets_for_every_pair(gap):
    """The least npk at which the cuts of a sweep_mask case of 17 channels per
    alignment class reach every (residue, window) pair.  Each class then holds
    every window at every slot, so the pairs are reached when every residue has
    a cut in a slot k with 1 <= k <= npk - 3: the slot of the last residue's
    first cut behind slot 0, and the two slots its window reaches past it."""
    P = TX_PACKET + gap
    # t * TILE mod P repeats after at most P tiles, and at most two tiles start in slot 0
    t = np.arange(1, P + 3, dtype=np.int64)
    first = np.full(P, np.iinfo(np.int64).max)
    for a in range(CHUNK):
        lo = t * TILE - a
        lo = lo[lo >= P]
        np.minimum.at(first, lo % P, lo)
    if (first == np.iinfo(np.int64).max).any():
        return None
    return int(first.max() // P + 3)


def cut_joins(gap, npk):
    """{alignment: [(slot, residue), ...]} of the cuts of a row of npk packets
    that fall within a slot's first JOIN_SPAN samples, in slot order"""
    P = TX_PACKET + gap
    out = {}
    for a in range(CHUNK):
        lo = g.tile_edges(a, npk * P)[0][1:]
        sel = lo % P < JOIN_SPAN
        out[a] = [(int(e // P), int(e % P)) for e in lo[sel]]
    return out


@functools.lru_cache(maxsize=None)
def packets_for_every_join_residue(gap):
    """the fewest packets after which the cuts of the 8 alignments have fallen
    on each of a slot's first JOIN_SPAN samples"""
    P = TX_PACKET + gap
    t = np.arange(1, P + 1, dtype=np.int64)
    first = np.full(JOIN_SPAN, np.iinfo(np.int64).max)
    for a in range(CHUNK):
        lo = t * TILE - a
        lo = lo[lo % P < JOIN_SPAN]
        np.minimum.at(first, lo % P, lo)
    if (first == np.iinfo(np.int64).max).any():
        return None
    return int(first.max() // P + 1)


def own_indices(mask, index0=None):
    """int64 [nch][npk + 1]: a channel's own packet index in front of slot k
    (column npk: behind the call), from the indices in front of the call"""
    nch, npk = mask.shape
    idx = np.zeros((nch, npk + 1), np.int64)
    idx[:, 1:] = np.cumsum(mask != 0, axis=1)
    return idx + (0 if index0 is None else np.asarray(index0, np.int64)[:, None])


class Masked:
    """A Case, the mask of its npk slots (over all its calls) and the channels'
    own indices in front of the first call."""

    def __init__(self, case, mask, index0=None):
        assert mask.shape == (case.nch, case.npk) and mask.dtype == np.uint8
        self.case, self.mask = case, mask
        self.index = own_indices(mask, index0)

    def window(self, c, k):
        """slots k-1 .. k+2 of channel c as a string of 1, 0 and, outside the
        block, -"""
        m = self.mask[c]
        return "".join("-" if not 0 <= j < m.size else "1" if m[j] else "0" for j in range(k - 1, k + 3))

    def first_slot(self, c):
        """the slot of channel c's first packet ever, None where it has none here"""
        k = np.flatnonzero(self.mask[c])
        return int(k[0]) if k.size and self.index[c, 0] == 0 else None

    def locate(self, c, p):
        """Case.locate and, for a position of the row, the slot's window and
        the channel's own index there"""
        msg = self.case.locate(c, p)
        if p >= self.case.n:
            return msg
        k = p // self.case.P
        what = "sends its packet" if self.mask[c, k] else "idle at own index"
        return (f"{msg}; slot {k} sample {p % self.case.P}, slots {k - 1}..{k + 2} active {self.window(c, k)}, "
                f"{what} {int(self.index[c, k])}")


# ---------------------------------------------------------------- the cases of tests/test_gpu_tx_mask_sweep.py
def _sweep(gap, **kw):
    return Case(SWEEP_NCH, packets_for_every_pair(gap), gap, **kw)


# as in tx_geometry.CASES: an int16 block starts 2 bytes past a 16-byte
# boundary and a block of codes 3 bytes past one, and ld is odd
CASES = {
    "s16_gap903": _sweep(903, addr16=2),
    "s16_gap0": _sweep(0, addr16=2),
    "alaw_gap903": _sweep(903, addr16=3, es=1),
    "s16_gap168": g.CASES["s16_gap168"],
    "launch2_s16": g.CASES["launch2_s16"],
    "launch2_alaw": g.CASES["launch2_alaw"],
    "rows4g_s16": g.CASES["rows4g_s16"],
    "rows4g_alaw": g.CASES["rows4g_alaw"],
}
for _split in ("calls41", "mixed"):
    for _gap in (903, 0):
        CASES[f"{_split}_gap{_gap}"] = g.CASES[f"{_split}_gap{_gap}"]
for _nch in g.GRID_X_NCH:
    CASES[f"gridx_{_nch}"] = Case(_nch, 4, 903, addr16=2)

LAUNCH2_MASK = np.array([[1, 0, 1, 1]], np.uint8)
ROWS4G_MASK = np.array([[1, 1], [0, 1], [1, 0]], np.uint8)


def random_mask(seed, nch, npk):
    """tx_mask_cases.masks: a random half of the slots with the rows its
    docstring names (imported here, not above: that module loads the library)"""
    from tx_mask_cases import masks
    return masks(seed, nch, npk)


def preroll_mask(seed, nch=SWEEP_NCH):
    """The call in front of a sweep: tx_mask_cases.masks over PREROLL slots,
    with one channel of every alignment class idle throughout (row 1 is; rows
    8 and 10 .. 15 here), so that every class keeps a channel at own index 0
    whose first packet ever falls into the sweep."""
    m = random_mask(seed, nch, PREROLL)
    assert not m[1].any()
    m[8] = 0
    m[10:16] = 0
    return m


SWEEP_SEED = {"s16_gap903": 21, "s16_gap0": 23, "alaw_gap903": 25}


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    """(Masked of the sweep call, the pre-roll mask): own indices in front of
    the sweep are the pre-roll's counts"""
    case, seed = CASES[name], SWEEP_SEED[name]
    pre = preroll_mask(seed + 1, case.nch)
    return Masked(case, sweep_mask(case.nch, case.npk, seed), (pre != 0).sum(axis=1)), pre


@functools.lru_cache(maxsize=None)
def join_case(gap, seed=11, addr16=2):
    """Masked: 8 alignment classes x (the longest list of cut_joins) channels,
    one packet more than it takes to cut at every residue below JOIN_SPAN.
    The j-th channel of a class is idle in front of the j-th cut slot of its
    alignment and active from it on; a channel past its class's list joins at
    a seeded random slot."""
    npk = packets_for_every_join_residue(gap) + 1
    joins = cut_joins(gap, npk)
    per = max(len(v) for v in joins.values())
    case = Case(CHUNK * per, npk, gap, addr16=addr16)
    rng = np.random.default_rng(seed)
    first = np.empty(case.nch, np.int64)
    for c in range(case.nch):
        mine = joins[g.alignment(case.addr16, case.es, c, case.ld)]
        first[c] = mine[c // CHUNK][0] if c // CHUNK < len(mine) else rng.integers(0, npk)
    active = np.arange(npk)[None, :] >= first[:, None]
    return Masked(case, _values(active, seed + 1))


def joins_met(masked):
    """bool [JOIN_SPAN]: the residues below JOIN_SPAN at which a tile cuts the
    slot that holds the first packet ever of the row it cuts"""
    case = masked.case
    met = np.zeros(JOIN_SPAN, bool)
    for row in case.rows():
        k0 = masked.first_slot(row.channel)
        if k0 is None:
            continue
        k = row.lo // case.P + row.first_packet
        sel = row.cut & (row.residue < JOIN_SPAN) & (k == k0)
        met[row.residue[sel]] = True
    return met
