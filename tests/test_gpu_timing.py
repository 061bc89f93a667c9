"""Every preamble position, every incoming rx_timing and exact ties at the
hunt's maximum, on every kernel shape and receiver mode (run with -m gpu).

The inputs are the corpora of tests/timing.py; tests/test_timing_corpus.py
asserts, on the oracle alone, what they reach:
- sweep: a valid frame at every max_index 0..127 and at every incoming
  rx_timing (3, 128..255), which the FIRs index LDS by and on which the window
  store, the split tail and the quad backs branch;
- sweep_noisy: match counts on both sides of the validity threshold, invalid
  frames at nearly every incoming rx_timing;
- impulses: non-zero hunt windows in which two lags hold exactly the maximum,
  all of them undecided by the filtered hunt, so that the exact chain's
  first-lag rule (and fft_hunt's) decides max_index, on valid frames.

Every comparison is tests/rxcheck.py's.  Expected values are the oracle's
(oracle/cpu_ref.c), computed once per corpus and mode.
"""
import functools

import numpy as np
import pytest

import rxcheck
import singlecarrier_amd as sc
import timing
from timing import CALLS, DIRECT, MODES

pytestmark = pytest.mark.gpu

assert MODES == [sc.MODE_REFERENCE, sc.MODE_DEC752, sc.MODE_FFT_HUNT, sc.MODE_DEC752 | sc.MODE_FFT_HUNT]

shapes = pytest.mark.parametrize("shape,width", rxcheck.ALL_SHAPES)
some_shapes = pytest.mark.parametrize("shape,width", [(None, None)] + rxcheck.ALL_SHAPES[:1])


@functools.lru_cache(maxsize=None)
def _expected(name, mode):
    """timing.expected as dense outputs, converted once per corpus and mode, read-only"""
    return rxcheck.frozen(rxcheck.dense(*timing.expected(name, mode)))[0]


def _run(name, mode, calls=None):
    x = timing.corpus(name)
    rx = sc.Receiver(x.shape[0], mode=mode)
    out = rxcheck.demod_in_calls(rx, x, calls or [x.shape[1]])
    assert rx.frames == x.shape[1]
    rx.close()
    rxcheck.assert_same(out, _expected(name, mode), f"{name}, mode {mode}")


@shapes
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["sweep", "sweep_noisy", "impulses"])
def test_corpus_every_shape_and_mode(name, mode, shape, width, monkeypatch):
    rxcheck.force_shape(monkeypatch, shape, width)
    _run(name, mode)


@shapes
def test_sweep_head_prepass(shape, width, monkeypatch):
    """head_kernel's FIR heads (QPSK_HEADPASS=1, reference mode) at every
    rx_timing and preamble position."""
    monkeypatch.setenv("QPSK_HEADPASS", "1")
    rxcheck.force_shape(monkeypatch, shape, width)
    _run("sweep", sc.MODE_REFERENCE)


@some_shapes
@pytest.mark.parametrize("mode", DIRECT)
@pytest.mark.parametrize("name", ["sweep", "impulses"])
def test_corpus_across_calls(name, mode, shape, width, monkeypatch):
    """Calls of 1, 1, 2, 1 and the remaining frames: ties and every rx_timing
    cross call boundaries and the carried history."""
    rxcheck.force_shape(monkeypatch, shape, width)
    nf = timing.corpus(name).shape[1]
    calls = [f for k, f in enumerate(CALLS) if sum(CALLS[:k + 1]) <= nf]
    if nf > sum(calls):
        calls.append(nf - sum(calls))
    assert len(calls) >= 3
    _run(name, mode, calls)


@pytest.mark.parametrize("mode", DIRECT)
@pytest.mark.parametrize("which", ["first16", "tied16"])
def test_impulses_tiny_host_calls(which, mode):
    """16 channels, one call per frame: at most 64 channel-frames a call, so
    the kernels read and write the pinned staging block itself.  The corpus's
    first 16 channels, and its first 16 that hold an exact tie."""
    ch = np.arange(16) if which == "first16" else timing.tied_channels(mode)
    x = np.ascontiguousarray(timing.impulses()[ch])
    rx = sc.Receiver(16, mode=mode)
    out = rxcheck.demod_in_calls(rx, x, [1] * x.shape[1])
    rx.close()
    rxcheck.assert_same(out, {k: v[ch] for k, v in _expected("impulses", mode).items()}, which)


def test_impulses_forced_exact(monkeypatch):
    """Every frame and job through the EXACT = true recomputation."""
    monkeypatch.setenv("QPSK_FORCE_EXACT", "1")
    _run("impulses", sc.MODE_REFERENCE)
