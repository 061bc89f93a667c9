"""The carried sample history (run with -m gpu).

Between calls a channel keeps the samples the next call's first frame reads:
x_{F-1}[0..hi) (hi = 1192, or 1704 in the dec752 mode) and the last 48 samples
of the call's last two frames.  The carry workgroups that lead the
rx_data_kernel launch write them into the context's history block,
[nch][2][1880] int16 (h0, h1), which qpsk_rx_state_save exports right after
its 64-byte header:
- h1 holds x_{F-1} on [0, hi) and on [1832, 1880);
- h0[1832..1880) holds x_{F-2}, or what h1 held there when the call had one
  frame;
- every other sample stays zero, as a fresh context has it.
These tests pin those bytes call by call on every kernel shape and both
modes, and the outputs of calls split so that one-frame calls (whose carry
reads the history it rewrites) follow each other, on device-staged and on
zero-copy pinned input.
"""
import functools

import numpy as np
import pytest

import oracle
import rxcheck
import singlecarrier_amd as sc

pytestmark = pytest.mark.gpu

FRAME = 1880
HDR = 64
TAIL = FRAME - 48

# (QPSK_SHAPE, QPSK_WIDTH): pick_shape's choice for a small batch, and each forced shape but W = 16
SHAPES = [(None, None)] + rxcheck.ALL_SHAPES[:4]
MODES = [sc.MODE_REFERENCE, sc.MODE_DEC752]
_ORACLE_MODE = {sc.MODE_REFERENCE: oracle.MODE_REF, sc.MODE_DEC752: oracle.MODE_DEC752}
_HEAD = {sc.MODE_REFERENCE: 1192, sc.MODE_DEC752: 1704}

shapes = pytest.mark.parametrize("shape,width", SHAPES)
modes = pytest.mark.parametrize("mode", MODES)


@functools.lru_cache(maxsize=None)
def _input(seed, nch, nf, ebn0):
    x = sc.synth(seed, nch, nf, ebn0)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _expected(seed, nch, nf, ebn0, mode):
    """The oracle's outputs over the whole stream, computed once per input and mode."""
    bits, valid, tr = oracle.cpu_rx(_input(seed, nch, nf, ebn0), trace=True, mode=_ORACLE_MODE[mode])
    return bits, valid, tr


def _history(rx, nch):
    snap = rx.state_save()
    return np.frombuffer(snap, np.int16, nch * 2 * FRAME, HDR).reshape(nch, 2, FRAME)


@shapes
@modes
@pytest.mark.parametrize("nch", [1, 65, 300])
def test_history_bytes(nch, mode, shape, width, monkeypatch):
    """After every call of F = [3] and of F = [1, 1, 1, 2] the snapshot's whole
    history block equals the one built here from the inputs: the carried
    ranges hold the call's last frames and every other sample is zero."""
    rxcheck.force_shape(monkeypatch, shape, width)
    _check_history_bytes(nch, mode)


@modes
def test_history_bytes_second_channel_pass(mode):
    """The same at 4,099 channels on the default shape.  The carry runs in
    min(256, ceil(nch / 16)) workgroups of 4 waves x 4 channels, so 4,099 is
    the smallest count at which a wave's channel loop runs a second time; on
    that pass 3 channels are left and the clamp min(c0 + k, nch - 1) of
    carry_block's loads is live."""
    _check_history_bytes(4099, mode)


def _check_history_bytes(nch, mode):
    hi = _HEAD[mode]
    for calls in ([3], [1, 1, 1, 2]):
        x = _input(300 + nch, nch, sum(calls), 6.0)
        rx = sc.Receiver(nch, mode=mode)
        want = np.zeros((nch, 2, FRAME), np.int16)
        np.testing.assert_array_equal(_history(rx, nch), want)
        a = 0
        for f in calls:
            rx.demod(np.ascontiguousarray(x[:, a:a + f]))
            a += f
            last = x[:, a - 1]
            prev = x[:, a - 2, TAIL:] if f >= 2 else want[:, 1, TAIL:].copy()
            want[:, 0, TAIL:] = prev
            want[:, 1, :hi] = last[:, :hi]
            want[:, 1, TAIL:] = last[:, TAIL:]
            np.testing.assert_array_equal(_history(rx, nch), want, err_msg=f"calls {calls}, after frame {a}")
        rx.close()


@shapes
@modes
def test_split_calls(mode, shape, width, monkeypatch):
    """130 channels x 10 frames as calls of 1, 1, 2, 1 and 5 frames: bits,
    valid flags, trace and soft symbols equal the oracle's over the 10 frames."""
    rxcheck.force_shape(monkeypatch, shape, width)
    x = _input(410, 130, 10, 6.0)
    rx = sc.Receiver(130, mode=mode)
    out = rxcheck.demod_in_calls(rx, x, [1, 1, 2, 1, 5])
    assert rx.frames == 10
    rxcheck.assert_same(out, _expected(410, 130, 10, 6.0, mode))
    rx.close()


@shapes
@modes
def test_pinned_small_calls(mode, shape, width, monkeypatch):
    """Host calls of at most 64 channel-frames read their input from the
    pinned staging block and write their outputs to it: 3 channels, five
    calls of 2 frames, equal to the oracle over the 10 frames."""
    rxcheck.force_shape(monkeypatch, shape, width)
    x = _input(420, 3, 10, 8.0)
    bits, valid, tr = _expected(420, 3, 10, 8.0, mode)
    assert valid.any() and not valid.all()   # data jobs ran, and not for every frame
    rx = sc.Receiver(3, mode=mode)
    out = rxcheck.demod_in_calls(rx, x, [2, 2, 2, 2, 2])
    rxcheck.assert_same(out, (bits, valid, tr))
    rx.close()
