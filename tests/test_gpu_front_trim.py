"""The reference-mode 4x2 kernel's trimmed front (run with -m gpu).

Its fronts prefetch frames n >= 2 of a call from one scalar base (the three
source frames are consecutive rows of the input: prefetch_rows; frames 0 and 1
read the carried history and keep the general path), and the split FIR derives
its per-lane LDS addresses from the wave-uniform rx_timing.  Every case forces
QPSK_SHAPE=4x2 and compares every output with the oracle's (oracle/cpu_ref.c)
by tests/rxcheck.py's comparison.

Which paths a corpus reaches is asserted on the oracle's trace first, so that
no case can pass on an input that never takes them.  On rx_timing: a fresh
channel's first window is all zero, so its frame 0 is valid whatever the input
and leaves rx_timing = max_index + 128; the initial rx_timing (3, below 128:
the only one at which the FIR reads the input's first item, M[0..127]) is
therefore the incoming rx_timing of a stream's first frame and of no other,
which is frame 0 of a context's first call, on the general path.
"""
import functools

import numpy as np
import pytest

import oracle
import rxcheck
import singlecarrier_amd as sc
import timing

pytestmark = pytest.mark.gpu

SPLIT_MI = 93        # qpsk_rx_front.h kSplitMi: the split FIR's tail runs from here on
NOISY = (23, 300, 6, 5.0)   # seed, channels (not a multiple of 32, 64 or 256), frames, Eb/N0


@functools.lru_cache(maxsize=None)
def _noisy():
    """The NOISY input and the oracle's (bits, valid, trace) for it, made once, read-only."""
    x = sc.synth(*NOISY)
    return rxcheck.frozen(x)[0], rxcheck.frozen(*oracle.cpu_rx(x, trace=True))


@pytest.fixture(autouse=True)
def _shape(monkeypatch):
    rxcheck.force_shape(monkeypatch, "4x2", None)


def _paths(tr, calls):
    """Per channel-frame masks from the oracle's trace: `rows`, the frame is
    the third or a later one of its call (one-base prefetch); `low`, its
    incoming rx_timing is below 128."""
    nch, nf = tr.shape
    n_in_call = np.concatenate([np.arange(f) for f in calls])
    assert n_in_call.size == nf
    rows = np.broadcast_to(n_in_call >= 2, (nch, nf))
    low = timing.rt_in(tr) < 128
    # both rx_timing regimes: the initial one in the stream's first frame only
    assert (low == (np.arange(nf) == 0)[None, :]).all()
    assert (timing.rt_in(tr)[low] == timing.RT_INITIAL).all()
    assert rows.any() and (~rows & ~low).any()
    return rows, low


def _run(x, exp, calls):
    rx = sc.Receiver(x.shape[0])
    out = rxcheck.demod_in_calls(rx, x, calls)
    assert rx.frames == x.shape[1]
    rx.close()
    rxcheck.assert_same(out, exp, f"calls {calls}")


@pytest.mark.parametrize("calls", [(6,), (1, 2, 3), (3, 1, 2)])
def test_noisy_300_channels(calls):
    """300 channels x 6 frames in one call, and in calls of 1, 2 and 3 frames
    chained on one context: a call's frames 0 and 1 read the history the calls
    before it left, its frame 2 takes the one-base path."""
    x, exp = _noisy()
    _paths(exp[2], calls)
    _run(x, exp, calls)


@pytest.mark.parametrize("calls", [(6,), (1, 2, 3)])
def test_sweep_every_rx_timing(calls):
    """tests/timing.py's sweep: every rx_timing 128..255 and every max_index
    on the one-base path, with and without the split FIR's tail."""
    x, exp = timing.corpus("sweep"), timing.expected("sweep", sc.MODE_REFERENCE)
    _, valid, tr = exp
    rows, _ = _paths(tr, calls)
    # the tail (max_index >= 93) and its absence, on both prefetch paths
    for m in (rows, ~rows):
        assert (m & (tr["max_index"] >= SPLIT_MI)).any() and (m & (tr["max_index"] < SPLIT_MI)).any()
    if calls == (6,):
        assert set(np.unique(timing.rt_in(tr)[rows]).tolist()) == set(range(128, 256))
        assert set(np.unique(tr["max_index"][valid.astype(bool) & rows]).tolist()) == set(range(128))
    _run(x, exp, calls)


@pytest.mark.parametrize("calls", [(4,), (3, 1)])
def test_impulses_exact_ties(calls):
    """Exact ties at the hunt's maximum, decided by the exact chain's
    first-lag rule.  The ties are in frame 3: on the one-base path, or a
    call's first frame."""
    x, exp = timing.corpus("impulses"), timing.expected("impulses", sc.MODE_REFERENCE)
    hc = timing.hunt_classes(x, sc.MODE_REFERENCE)
    tied = hc["split"] & ~hc["zero"]
    rows, _ = _paths(exp[2], calls)
    assert (tied & rows).any() if calls == (4,) else (tied & ~rows).any()
    _run(x, exp, calls)


def test_forced_exact(monkeypatch):
    """Every frame through the EXACT = true recomputation (QPSK_FORCE_EXACT)."""
    monkeypatch.setenv("QPSK_FORCE_EXACT", "1")
    _run(*_noisy(), (6,))
