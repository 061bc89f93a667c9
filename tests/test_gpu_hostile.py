"""Parity on hostile inputs (run with -m gpu): tests/hostile.py's streams drive
the reference's equalizer state out of fp32 range inside a frame, so valid
frames carry soft symbols of 1e36, inf and NaN, and the reference's C99 complex
products take gcc's Annex G recovery.  The expected values are the oracle's
(oracle/cpu_ref.c), pinned to the unmodified reference on this very corpus by
tests/test_oracle.py.

Comparison: tests/rxcheck.py's with nan_as_class=True: soft symbols of valid
frames bit for bit for finite values and infinities, NaN compared as NaN only
(the GPU's NaN payloads and signs need not be x86's).
"""
import os

import numpy as np
import pytest

import hostile
import oracle
import rxcheck
import singlecarrier_amd as sc

pytestmark = pytest.mark.gpu


def _demod(x, mode=sc.MODE_REFERENCE, cuts=None):
    """x through a fresh context, as calls that end at the frames `cuts` and at the last."""
    rx = sc.Receiver(x.shape[0], mode=mode)
    out = rxcheck.demod_in_calls(rx, x, np.diff([0] + (cuts or []) + [x.shape[1]]))
    rx.close()
    return out


def _run(name="wave", mode=sc.MODE_REFERENCE, cuts=None, what=""):
    rxcheck.assert_same(_demod(hostile.group(name), mode, cuts), hostile.expected(name, mode),
                        what or name, nan_as_class=True)


def test_device_product_equals_the_oracles():
    """The kernels' exact complex product (qpsk_cmul.h cmul_g, and cmulc_g as
    the product with the conjugate) against the oracle's qc_cmul, i.e. gcc's
    C99 product with the Annex G recovery, over every combination of
    {+-0, +-1, +-3e38, +-inf, NaN} in the four operands (6,561 of them: inf * 0,
    inf - inf, overflow from finite operands); NaN compared as a class."""
    import ctypes as C
    import itertools
    import subprocess
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernels")
    path = os.path.join(here, "libcmul_check.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-C", here], check=True)
    lib = C.CDLL(path)
    lib.cmul_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    vals = [0.0, -0.0, 1.0, -1.0, 3e38, -3e38, np.inf, -np.inf, np.nan]
    ops = np.array(list(itertools.product(vals, repeat=4)), np.float32)
    got = np.zeros((len(ops), 4), np.float32)
    assert lib.cmul_check(ops.ctypes.data, got.ctypes.data, len(ops)) == 0
    conj = ops * np.array([1, 1, 1, -1], np.float32)
    exp = np.concatenate([oracle.cmul(ops), oracle.cmul(conj)], axis=1)
    bad = rxcheck.same_soft(got, exp).any(1)
    assert not bad.any(), (int(bad.sum()), ops[bad][0], got[bad][0], exp[bad][0])
    assert np.isinf(exp).any() and np.isnan(exp).any()


def test_corpus_holds_non_finite_valid_frames():
    """What the other cases rest on, from the oracle's side: valid frames with
    inf or NaN soft symbols, and finite ones beyond 1e30."""
    _, valid, tr = hostile.expected("wave")
    soft = tr["soft"][valid.astype(bool)]
    nonfin = ~np.isfinite(soft).all((-1, -2))
    assert nonfin.sum() >= 8
    assert np.abs(soft[np.isfinite(soft)]).max() > 1e30


@pytest.mark.parametrize("shape", [None, "4x2", "2x4d", "1x8"])
def test_corpus_every_shape(shape, monkeypatch):
    """The 160 wave channels x 12 frames at the shape the batch size selects
    (one group per workgroup, quad backs) and with each rx_kernel shape forced."""
    rxcheck.force_shape(monkeypatch, shape, None)
    _run(what=f"shape {shape}")


@pytest.mark.parametrize("width", ["16", "32", "64"])
def test_corpus_group_widths(width, monkeypatch):
    """Quad backs (W = 16, 32) and lane backs (W = 64) of the dual-chain kernel."""
    rxcheck.force_shape(monkeypatch, None, width)
    _run(what=f"width {width}")


def test_corpus_forced_exact_path(monkeypatch):
    """Every frame and job through the EXACT = true recomputation."""
    monkeypatch.setenv("QPSK_FORCE_EXACT", "1")
    _run(what="force exact")


def test_corpus_head_prepass(monkeypatch):
    monkeypatch.setenv("QPSK_HEADPASS", "1")
    _run(what="headpass")


def test_corpus_across_call_splits():
    """Calls of 1, 1, 4 and the remaining frames: a frame's non-finite
    equalizer state reaches neither the next frame nor the next call (the
    reference resets it per frame, src/kalman.c:42-55)."""
    _run(cuts=[1, 2, 6], what="calls 1+1+4+6")


def test_tiny_host_call():
    """A host call of <= 64 channel-frames (the pinned staging block): the
    table's first 8 rows, sensitive inside their first 4 frames."""
    x = np.ascontiguousarray(hostile.group("wave")[:8, :4])
    exp = tuple(a[:8, :4] for a in hostile.expected("wave"))
    rxcheck.assert_same(_demod(x), exp, "tiny call", nan_as_class=True)


def test_rx_frame_surface_against_the_golden(golden_dir):
    """One sensitive channel frame by frame through qpsk_rx_frame(), against
    the reference-made golden (hostile_ref.npz).  The surface returns the
    valid flag and the bits only, and on this corpus the Annex G recovery has
    shown in `matches` alone: this case fails on a fault, on state leaking
    from a non-finite frame into the next call, or on a future difference in
    flags or bits, not on the product itself (test_corpus_* see that)."""
    g = np.load(os.path.join(golden_dir, "hostile_ref.npz"))
    gd = hostile.params()["golden"]
    nf = gd["frames"]
    gvalid = g["ref_valid"]
    c = int(np.argmax(gvalid[:gd["sensitive"]].sum(1)))   # the sensitive row with the most valid frames
    assert gvalid[c].any()
    gbits = np.unpackbits(g["ref_bits"][c], axis=-1)[:, :oracle.NBITS]
    sc.qpsk_rx_init()
    for n in range(nf):
        v, b = sc.qpsk_rx_frame(hostile.group("wave")[c, n])
        assert v == gvalid[c, n], n
        if v:
            np.testing.assert_array_equal(b, gbits[n], err_msg=f"frame {n}")


def test_stream_chunks():
    """The corpus through sc.Stream in chunks of 4 frames.  The stream returns
    bits and valid flags only, so, as with qpsk_rx_frame(), this case guards
    against faults and state leaking across chunks on non-finite frames; the
    product's effect (`matches`) is not visible here."""
    x = hostile.group("wave")
    bits, valid, _ = hostile.expected("wave")
    st = sc.Stream(x.shape[0], 4, nslot=3)
    got = []
    for k in range(3):
        st.acquire()[...] = x[:, 4 * k:4 * k + 4]
        st.submit()
    while st.pending:
        got.append(st.retrieve())
    st.close()
    rxcheck.assert_same({"bits": np.concatenate([b for b, _ in got], axis=1),
                         "valid": np.concatenate([v for _, v in got], axis=1)}, {"bits": bits, "valid": valid})


@pytest.mark.parametrize("mode", [sc.MODE_DEC752, sc.MODE_FFT_HUNT, sc.MODE_DEC752 | sc.MODE_FFT_HUNT])
def test_corpus_receiver_modes(mode):
    _run(mode=mode, what=f"mode {mode}")


@pytest.mark.parametrize("shape", [None, "4x2", "2x4d", "1x8"])
def test_impaired_group_every_shape(shape, monkeypatch):
    """The finite side: echoes, clipping gains, DC offsets and a level step on
    the modem's own signal (|soft| up to 1e10, match counts at the threshold)."""
    rxcheck.force_shape(monkeypatch, shape, None)
    _run("impaired", what=f"impaired, shape {shape}")
