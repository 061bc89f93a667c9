"""What the tests of the transmitter's masked calls share, written from
include/qpsk_tx.h ("Channels that come and go") alone: nothing here knows how
the library keeps a channel's index or builds its plan.

Restated   the expected rows, restated independently of the host twin
           qpsk_tx_batch_masked_host: per channel, one channel at a time,
           sc.tx_batch_host on that channel's active packets only (gap 0, on a
           state carried per channel), each packet's 1880 samples placed at its
           slot and zeros everywhere else.
Twin       the host twin over explicit states: the yardstick of the GPU tests.
masks()    the mask rows the issue names, around a random mask of density 1/2.
snapshot fields, from the layout in the header.

Plain module: no GPU import.
"""
import numpy as np

import singlecarrier_amd as sc

PACKET = sc.TX_PACKET
MAGIC, VERSION, HEADER = 0x53585451, 1, 16


def payload(seed, nch, npk):
    return np.random.default_rng(seed).integers(0, 2, (nch, npk, 8, sc.NBITS), dtype=np.uint8)


class Restated:
    """nch channels, each a fresh run of the plain host transmitter fed its own
    packets; call() returns int16 [nch][npackets * (1880 + gap)]."""

    def __init__(self, nch):
        self.st = sc.tx_states(nch)
        self.sent = np.zeros(nch, np.uint64)

    def reset(self, c0, n):
        self.st[c0:c0 + n] = sc.tx_states(n)
        self.sent[c0:c0 + n] = 0

    def call(self, bits, gap, active=None):
        nch, npk = bits.shape[:2]
        P = PACKET + gap
        out = np.zeros((nch, npk, P), np.int16)
        for c in range(nch):
            k = np.arange(npk) if active is None else np.flatnonzero(active[c])
            if k.size:
                y = sc.tx_batch_host(bits[c:c + 1, k], gap=0, states=self.st[c:c + 1], threads=1)
                out[c, k, :PACKET] = y.reshape(k.size, PACKET)
                self.sent[c] += np.uint64(k.size)
        return out.reshape(nch, npk * P)


class Twin:
    """qpsk_tx_batch_masked_host over states of its own."""

    def __init__(self, nch):
        self.st = sc.tx_states(nch)

    def reset(self, c0, n):
        self.st[c0:c0 + n] = sc.tx_states(n)

    def call(self, bits, gap, active=None):
        return sc.tx_batch_host(bits, gap=gap, states=self.st, active=active)


def masks(seed, nch, npk):
    """uint8 [nch][npk]: a random half of the slots, with
       row 1   idle throughout
       row 2   its first packet in a later slot (npk // 2)
       row 3   its last active slot not the call's last (idle from npk - 3 on)
       row 4   an idle run longer than a tile at any gap (slots 1 .. npk - 2)
       row 5   every slot active
       row 6   idle first slot;  row 7  idle last slot
    and nonzero values other than 1 among the active ones."""
    assert nch >= 8 and npk >= 4
    rng = np.random.default_rng(seed)
    m = (rng.random((nch, npk)) < 0.5).astype(np.uint8)
    m[1] = 0
    m[2, :npk // 2], m[2, npk // 2] = 0, 1
    m[3, npk - 3:], m[3, npk - 4] = 0, 1
    m[4], m[4, 0], m[4, npk - 1] = 0, 1, 1
    m[5] = 1
    m[6, 0], m[6, 1] = 0, 1
    m[7, npk - 1], m[7, npk - 2] = 0, 1
    m *= rng.choice(np.array([1, 2, 0x80, 0xFF], np.uint8), m.shape)
    return m


def last_dibits(packet):
    """The state word of a channel whose latest packet is `packet` [8][62]:
    bit j = I sign (1: -1) of data symbol 239 + j, bit 16 + j its Q sign."""
    w = 0
    for j in range(9):
        d = 239 + j
        fr, s = divmod(d, 31)
        w |= int(packet[fr, 2 * s + 1] == 1) << j
        w |= int(packet[fr, 2 * s] == 1) << (16 + j)
    return w


def snapshot(indices, words):
    n = len(indices)
    return (np.array([MAGIC, VERSION, n, 0], "<u4").tobytes() + np.asarray(indices, "<u8").tobytes() +
            np.asarray(words, "<u4").tobytes())


def snapshot_fields(snap):
    """(n, indices uint64 [n], words uint32 [n]) of a snapshot, its header checked"""
    head = np.frombuffer(snap[:HEADER], "<u4")
    assert head[0] == MAGIC and head[1] == VERSION and head[3] == 0
    n = int(head[2])
    assert len(snap) == HEADER + 12 * n
    return n, np.frombuffer(snap[HEADER:HEADER + 8 * n], "<u8"), np.frombuffer(snap[HEADER + 8 * n:], "<u4")
