"""A deterministic corpus of short bursts at irregular spacing: every pair of
incoming rx_timing and preamble position the receive front can be in.

Plain module in the style of tests/timing.py: integer arithmetic plus
oracle.synth (the C generator, the same on every machine); no GPU import and
none of numpy's generators.  Arrays are made once and are read-only.

Why pairs.  Call n of the reference filters frame n - 1 and writes the upper
half of decimated_frame from it under the rx_timing the call starts with,
rt_in(n) (src/qpsk.c:157-162); call n + 1 hunts and equalizes in that half,
now the lower one (:172-188).  A frame's result so depends on two values: the
timing of the call before it and the max_index its own hunt finds.  With
r = rt_in(n), a preamble whose first sample is sample p of frame n - 1 is
found by call n + 1 at max_index m where

    p = 5 m + r - DELAY                                   (DELAY = 47),

and leaves rt_in(n + 2) = m + 128 behind.  The first two calls of a channel
see nothing but the zero-initialised buffers (the fresh rx_timing, 3, only
ever samples zeros), so max_index(0) = max_index(1) = 0 on every input, and
frame k's samples decide max_index(k + 2).

Burst.  bursts()[j] is the first BURST_LEN = 900 samples of packet j of
timing.base(): the preamble (640 samples), one block of 31 data symbols and
the transmit filter's tail.  A channel is a list of rows (start, burst, lo,
hi): the int32 sum of samples lo..hi-1 of the bursts named, the first of them
at sample `start` of the stream, clipped to int16.  Bursts may overlap.

The corpus is four groups of channels, NFRAMES = 12 frames each:

directed   NSTEP * 128 channels.  Channel (j, x) places one burst per frame so
           that max_index(k) = (x + STEPS[j][k]) % 128 for k = 2..11.  The
           differences of neighbouring entries of STEPS' rows hold every
           residue mod 128 (pair A below), and so do the differences of
           entries two apart (pair B); x = 0..127 then puts every value in
           the pairs' first place.  STEPS is built here, least used first.
random     NRANDOM channels of bursts whose start-to-start spacing an LCG
           draws from [SPACE_LO, SPACE_HI): bursts that fall anywhere in a
           frame, overlap, straddle frames and leave frames empty.  These
           bring the invalid frames, the match counts on both sides of the
           validity threshold and the hunts the filtered rule leaves
           undecided.
carried    NCUT * 128 channels.  For every r = 128..255 and every cut v:
           frames that are invalid without being silent and start with
           rx_timing r, each followed by a valid frame.  The invalid frame's
           window holds a burst cut inside its preamble, two bursts whose
           preambles overlap, or a burst that starts too late (CUTS[v]).
tails      NTAIL channels per piece of TAILS: the last samples of a burst
           alone in a window, a valid frame whose hunt the filtered rule
           leaves undecided, placed at a range of max_index.

pair_coverage(mode) says, from the oracle alone, what the corpus reaches;
tests/test_spacing_corpus.py asserts it.
"""
import functools
import hashlib

import numpy as np

import oracle
import timing
from rxcheck import frozen

FRAME = 1880
NFRAMES = 12
BURST_LEN = 900
NBURST = 5                      # packets of timing.base() the bursts are cut from
DELAY = 47                      # p = 5 m + r - DELAY, measured on the oracle
RT_INITIAL = timing.RT_INITIAL
BAD_PHASE = 31                  # see start()

NSTEP = 20
NRANDOM = 2048
SPACE_LO, SPACE_HI = 1240, 2520
LCG_A, LCG_C = 6364136223846793005, 1442695040888963407   # Knuth's MMIX, mod 2^64
# carried group, what makes a window invalid without being silent: (lo, lag,
# second).  Samples lo..899 of a burst, placed as if its sample 0 lay at that
# lag of the window (plus 0..6), and over it a second whole burst `second`
# samples later, or none.  lo > 0 cuts the burst inside its preamble, so the
# hunt meets the preamble's end where no lag fits; a second burst 40 to 165
# samples on overlaps the first one's preamble with its own; lag 140 starts
# the preamble past the last lag the hunt tries.  (Keeping only the head of a
# burst does not do it: the equalizer counts the zeros after it as matches.)
CUTS = ((300, 60, 0), (0, 60, 40), (200, 20, 0), (0, 40, 165), (0, 30, 85), (0, 140, 0))
NCUT = len(CUTS)
# tails group: (burst, lo, hi, shift, first and last max_index).  Samples lo..hi-1
# of the burst, the end of its data block and the filter's tail, alone in a
# window: some 30 non-zero symbols whose two largest correlations lie within
# 0.5 % of each other, so the filtered hunt commits to neither, while the
# equalizer counts the window's zeros as matches and the frame is valid.  Found
# by a scan of lo on the oracle; `shift` puts the winning lag at the target.
TAILS = ((3, 758, 900, 24, 19, 99), (0, 787, 900, 24, 9, 35), (1, 645, 900, -51, 27, 51))
NTAIL = 32


@functools.lru_cache(maxsize=None)
def bursts():
    """[NBURST][BURST_LEN] int32: the head of each of the base stream's packets."""
    b = timing.base(6)
    assert b.size >= (NBURST - 1) * timing.PERIOD + BURST_LEN
    out = np.stack([b[j * timing.PERIOD:j * timing.PERIOD + BURST_LEN] for j in range(NBURST)])
    return frozen(out.astype(np.int32))[0]


class _Lcg:
    def __init__(self, seed):
        self.s = seed & (2 ** 64 - 1)

    def below(self, n):
        self.s = (self.s * LCG_A + LCG_C) & (2 ** 64 - 1)
        return (self.s >> 33) % n


@functools.lru_cache(maxsize=None)
def steps():
    """STEPS [NSTEP][NFRAMES]: row j's entries 2..11 are offsets mod 128 whose
    differences d(k) = s[k] - s[k-1] (k = 3..11) and e(k) = s[k] - s[k-2]
    (k = 4..11) are chosen greedily: the least-used pair of residues, d
    among the differences of neighbours and e among those two apart, taken
    over all rows so far.  Every residue is so used by both about equally
    often, at varying frames k."""
    used_d, used_e = [0] * 128, [0] * 128
    rows = []
    for j in range(NSTEP):
        s = [0, 0, (37 * j) % 128]
        for k in range(3, NFRAMES):
            best = None
            for t in range(128):
                d = (t + 5 * j + 11 * k) % 128          # the scan's start moves with j and k
                cost = used_d[d] * 2
                if k >= 4:
                    cost += used_e[(s[k - 1] + d - s[k - 2]) % 128] * 2 + 1
                if best is None or cost < best[0]:
                    best = (cost, d)
            d = best[1]
            used_d[d] += 1
            if k >= 4:
                used_e[(s[k - 1] + d - s[k - 2]) % 128] += 1
            s.append((s[k - 1] + d) % 128)
        rows.append(s)
    return rows


def start(m, r):
    """The sample of its frame at which a burst starts for the call that reads
    it under rx_timing r to find it at max_index m.  One residue of p mod 40
    is avoided (1880 = 47 * 40, so it is the same samples of every frame, and
    the same phase of the receiver's mixer): measured on the oracle, a
    noiseless burst that starts there trains the equalizer to 79..83 matches
    of 128 in the dec752 mode and 79..117 in reference mode, under or near
    the validity threshold of 99, against 117 or more at every other residue.
    One sample later max_index is the same and the frame is valid."""
    p = 5 * m + r - DELAY
    return p + 1 if p % 40 == BAD_PHASE else p


def place(targets, which=0, piece=None):
    """Rows (start, burst, lo, hi) of one burst per frame, or of one piece
    (burst, lo, hi, shift) of TAILS per frame, so that the oracle finds
    max_index(k) = targets[k] for k = 2..len(targets) - 1 (targets[0] and [1]
    must be 0: the zero-initialised buffers)."""
    assert targets[0] == 0 and targets[1] == 0
    out = []
    for k in range(2, len(targets)):
        r = targets[k - 2] + 128                        # rt_in(k - 1): frame k - 2's max_index + 128
        p = (k - 2) * FRAME + start(targets[k], r)
        if piece:
            out.append((p + piece[3], piece[0], piece[1], piece[2]))
        else:
            out.append((p, (which + k) % NBURST, 0, BURST_LEN))
    return out


def render(rows, nframes=NFRAMES):
    """[len(rows)][nframes][1880] int16 from rows of (start, burst, lo, hi):
    samples lo..hi-1 of the burst, the first of them at sample `start`."""
    b = bursts()
    n = nframes * FRAME
    x = np.zeros((len(rows), n + BURST_LEN), np.int32)
    for c, row in enumerate(rows):
        for at, j, lo, hi in row:
            assert 0 <= at < n and 0 <= lo < hi <= BURST_LEN
            x[c, at:at + hi - lo] += b[j, lo:hi]
    np.clip(x, -32768, 32767, out=x)
    return x[:, :n].astype(np.int16).reshape(len(rows), nframes, FRAME)


def directed_rows():
    rows = []
    for j, s in enumerate(steps()):
        for x in range(128):
            rows.append(place([0, 0] + [(x + v) % 128 for v in s[2:]], which=j + x))
    return rows


def random_rows(n=NRANDOM, seed=1):
    rows = []
    for c in range(n):
        g = _Lcg(seed * 1000003 + c)
        for _ in range(4):
            g.below(2)
        t, row = g.below(SPACE_HI), []
        while t < NFRAMES * FRAME:
            row.append((t, g.below(NBURST), 0, BURST_LEN))
            t += SPACE_LO + g.below(SPACE_HI - SPACE_LO)
        rows.append(row)
    return rows


def carried_rows():
    """Per (r, v), three times: a burst in frame f that call f + 2 finds at
    max_index r - 128, so that call f + 3 starts with rx_timing r; CUTS[v]'s
    samples in frame f + 1, which are that call's window and leave it invalid
    (rx_timing stays r); a whole burst in frame f + 2, read under r, that call
    f + 4 finds valid.  The next f is three frames on, its burst read under
    the r the invalid frame kept."""
    rows = []
    for r in range(128, 256):
        for v, (lo, lag, second) in enumerate(CUTS):
            row = []
            m_read, m_bad, want = 0, 0, r - 128         # max_index of frames f and f + 1
            for f in (1, 4, 7):
                j = (r + v + f) % NBURST
                row.append((f * FRAME + start(want, m_read + 128), j, 0, BURST_LEN))
                bad = (f + 1) * FRAME + 5 * (lag + (r + f) % 7) + m_bad + 128 - DELAY + lo
                row.append((bad, (j + 1) % NBURST, lo, BURST_LEN))
                if second:
                    row.append((bad + second, (j + 2) % NBURST, 0, BURST_LEN))
                nxt = (r * 5 + v * 17 + f) % 128        # the valid frame after the invalid one
                row.append(((f + 2) * FRAME + start(nxt, r), (j + 3) % NBURST, 0, BURST_LEN))
                m_read, m_bad = want, nxt
            rows.append(row)
    return rows


def tail_rows():
    """Per piece of TAILS and channel c: one piece per frame, each alone in
    its window, at max_index values that step through the piece's range."""
    rows = []
    for burst, lo, hi, shift, m_lo, m_hi in TAILS:
        span = m_hi - m_lo + 1
        for c in range(NTAIL):
            t = [0, 0] + [m_lo + (c * 5 + k * 13 + (k & 1) * 40) % span for k in range(2, NFRAMES)]
            rows.append(place(t, piece=(burst, lo, hi, shift)))
    return rows


GROUPS = {"directed": directed_rows, "random": random_rows, "carried": carried_rows,
          "tails": tail_rows}


@functools.lru_cache(maxsize=None)
def group_slices():
    out, a = {}, 0
    for name, fn in GROUPS.items():
        n = len(fn())
        out[name] = slice(a, a + n)
        a += n
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    rows = [r for fn in GROUPS.values() for r in fn()]
    assert len(rows) <= 8192
    return frozen(render(rows))[0]


@functools.lru_cache(maxsize=None)
def expected(mode=0):
    """The oracle's (bits, valid, trace) over the corpus, computed once, read-only."""
    return frozen(*oracle.cpu_rx(corpus(), trace=True, mode=mode))


def pairs(valid, tr):
    """A and B [256][128] bool, and the incoming rx_timing values carried
    through an invalid frame into a valid one.
      A[rt_in(n), max_index(n)]      frame n valid;
      B[rt_in(n), max_index(n + 1)]  frames n and n + 1 valid;
      carried: rt_in(n) of invalid frames n followed by a valid frame n + 1."""
    vm = valid.astype(bool)
    rt = timing.rt_in(tr)
    mi = tr["max_index"]
    a = np.zeros((256, 128), bool)
    b = np.zeros((256, 128), bool)
    a[rt[vm], mi[vm]] = True
    both = vm[:, :-1] & vm[:, 1:]
    b[rt[:, :-1][both], mi[:, 1:][both]] = True
    inv = ~vm[:, :-1] & vm[:, 1:]
    return a, b, set(np.unique(rt[:, :-1][inv]).tolist())


def pair_coverage(mode=0, channels=None):
    """What the oracle's run over the corpus (or over corpus()[channels])
    reaches: the pair tables A and B, the rx_timing values carried through an
    invalid frame, and timing.coverage's counts."""
    exp = expected(mode)
    if channels is not None:
        exp = tuple(e[channels] for e in exp)
    _, valid, tr = exp
    a, b, carried = pairs(valid, tr)
    cv = timing.coverage(None, mode, exp)
    cv.update({"A": a, "B": b, "carried": carried})
    return cv


def digests(bits, valid, tr):
    """sha256 of each output over the whole corpus, little-endian bytes: bits,
    valid, max_index, matches and rx_timing as int32, and the soft symbols'
    bit patterns with those of invalid frames zeroed.  The reference's own are
    in tests/golden/spacing_ref.json (tests/golden/make_golden.py --spacing)."""
    vm = valid.astype(bool)
    soft = np.where(vm[..., None, None], tr["soft"].view(np.uint32), np.uint32(0))
    parts = {"bits": bits.astype(np.uint8), "valid": valid.astype(np.uint8), "soft": soft.astype("<u4")}
    for k in ("max_index", "matches", "rx_timing"):
        parts[k] = tr[k].astype("<i4")
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in parts.items()}
