"""Every pair of incoming rx_timing and preamble position, on every kernel
shape and receiver mode, across calls, through a checkpoint and through the
streaming pipeline (run with -m gpu).

The input is the corpus of tests/spacing.py: short bursts at irregular
spacing, 5,472 channels x 12 frames.  tests/test_spacing_corpus.py asserts, on
the oracle alone, what it reaches: all 16,384 pairs (rt_in(n), max_index(n))
on valid frames and all 16,384 pairs (rt_in(n), max_index(n + 1)) on
consecutive valid frames, in every mode; every rx_timing carried through an
invalid frame into a valid one; match counts on both sides of the validity
threshold; hunts the filtered rule leaves undecided, on valid frames.  The
pairs decide which LDS words the FIRs index, where the window store cuts,
whether the split FIR computes dec[255..289] and what the quad backs branch
on; the second kind of pair lives on the launch boundary and the carried
window, which the split calls and the checkpoint put between its two frames.

Every comparison with the oracle is tests/rxcheck.py's.  Expected values are
the oracle's (oracle/cpu_ref.c), computed once per mode, and the oracle is
pinned to the reference on this corpus.
"""
import functools

import numpy as np
import pytest

import rxcheck
import singlecarrier_amd as sc
import spacing
from rxcheck import KEYS
from timing import CALLS, DIRECT, MODES

pytestmark = pytest.mark.gpu

shapes = pytest.mark.parametrize("shape,width", rxcheck.ALL_SHAPES)
some_shapes = pytest.mark.parametrize("shape,width", [(None, None)] + rxcheck.ALL_SHAPES[:1])
CUT = 5                          # frames before the checkpoint
RANGE = slice(2304, 2816)        # the checkpoint's channels: directed and random ones


@functools.lru_cache(maxsize=None)
def _expected(mode):
    """spacing.expected as dense outputs, converted once per mode, read-only"""
    return rxcheck.frozen(rxcheck.dense(*spacing.expected(mode)))[0]


def _run(mode, calls=None):
    x = spacing.corpus()
    rx = sc.Receiver(x.shape[0], mode=mode)
    out = rxcheck.demod_in_calls(rx, x, calls or [x.shape[1]])
    assert rx.frames == x.shape[1]
    rx.close()
    rxcheck.assert_same(out, _expected(mode), f"mode {mode}")


@shapes
@pytest.mark.parametrize("mode", MODES)
def test_corpus_every_shape_and_mode(mode, shape, width, monkeypatch):
    rxcheck.force_shape(monkeypatch, shape, width)
    _run(mode)


@shapes
def test_corpus_head_prepass(shape, width, monkeypatch):
    """head_kernel's FIR heads (QPSK_HEADPASS=1, reference mode) at every pair."""
    monkeypatch.setenv("QPSK_HEADPASS", "1")
    rxcheck.force_shape(monkeypatch, shape, width)
    _run(sc.MODE_REFERENCE)


@some_shapes
@pytest.mark.parametrize("mode", DIRECT)
@pytest.mark.parametrize("calls", ["ones", "mixed"])
def test_corpus_across_calls(calls, mode, shape, width, monkeypatch):
    """One frame per call throughout, and calls of 1, 1, 2, 1 and the rest:
    the frames of every pair B fall on both sides of a launch boundary, with
    the window and its preamble position carried in the context between."""
    rxcheck.force_shape(monkeypatch, shape, width)
    nf = spacing.NFRAMES
    _run(mode, [1] * nf if calls == "ones" else list(CALLS) + [nf - sum(CALLS)])


@pytest.mark.parametrize("mode", DIRECT)
def test_checkpoint_in_the_middle(mode, monkeypatch):
    """state_save after frame 5 of channels RANGE in the whole corpus's context
    (default shape), state_load into a fresh 4x2 context of just those
    channels, then the other 7 frames: equal to the one-call result and to the
    oracle.  The oracle says the range still holds over 1,000 pairs B, and
    that in at least 256 of its channels the two frames of a pair B lie on
    either side of the cut."""
    exp = tuple(e[RANGE] for e in spacing.expected(mode))
    _, valid, tr = exp
    b = spacing.pairs(valid, tr)[1]
    vm = valid.astype(bool)
    on_cut = vm[:, CUT - 1] & vm[:, CUT]             # channels whose pair B straddles the cut
    print(mode, int(b[128:].sum()), int(on_cut.sum()))
    assert b[128:].sum() >= 1000
    assert on_cut.sum() >= 256

    x = spacing.corpus()
    n = RANGE.stop - RANGE.start
    a = sc.Receiver(x.shape[0], mode=mode)
    whole = sc.Receiver(x.shape[0], mode=mode).demod(x, trace=True, soft=True)
    head = a.demod(np.ascontiguousarray(x[:, :CUT]), trace=True, soft=True)
    snap = a.state_save(RANGE.start, n)
    a.close()
    rxcheck.force_shape(monkeypatch, "4x2", None)
    f = sc.Receiver(n, mode=mode)
    f.state_load(snap)
    assert f.frames == CUT
    rest = f.demod(np.ascontiguousarray(x[RANGE, CUT:]), trace=True, soft=True)
    f.close()
    got = {k: np.concatenate([head[k][RANGE], rest[k]], axis=1) for k in KEYS}
    for k in KEYS:
        np.testing.assert_array_equal(got[k], whole[k][RANGE], err_msg=k)
    rxcheck.assert_same(got, {k: v[RANGE] for k, v in _expected(mode).items()}, f"mode {mode}")


def test_corpus_through_the_stream():
    """sc.Stream, 3 slots, chunks of 2 frames, reference mode: bits and valid
    flags of the six chunks equal the oracle's."""
    x = spacing.corpus()
    fpc, nslot = 2, 3
    st = sc.Stream(x.shape[0], fpc, nslot=nslot)
    got_b, got_v = [], []
    for k in range(x.shape[1] // fpc):
        if st.pending == nslot:
            b, v = st.retrieve()
            got_b.append(b)
            got_v.append(v)
        st.acquire()[...] = x[:, k * fpc:(k + 1) * fpc]
        st.submit()
    while st.pending:
        b, v = st.retrieve()
        got_b.append(b)
        got_v.append(v)
    st.close()
    rxcheck.assert_same({"bits": np.concatenate(got_b, axis=1), "valid": np.concatenate(got_v, axis=1)},
                        _expected(sc.MODE_REFERENCE))


def test_corpus_forced_exact(monkeypatch):
    """Every frame and job through the EXACT = true recomputation."""
    monkeypatch.setenv("QPSK_FORCE_EXACT", "1")
    _run(sc.MODE_REFERENCE)
