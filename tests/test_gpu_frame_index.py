"""The context's global frame index g, far from zero (run with -m gpu).

Three things depend on g: the descrambler word (g mod 1057, the keystream
period of src/scramble.c's 15-bit LFSR in 62-bit frames), the mixer sign
(g & 1) and the parity of the double-buffered per-channel state.  Here g
crosses the keystream period on every back and shape, through the drop-in and
the stream; it is moved to 2^32 and beyond through a snapshot; one call holds
more than 2^32 samples; and the kernel-time accounting (qpsk_rx_timing_*) is
checked while its event pool folds.

Every comparison of a receive result is tests/rxcheck.py's, against the oracle
restatement (oracle/cpu_ref.c) of one continuous run from frame 0.
"""
import time

import numpy as np
import pytest

import oracle
import rxcheck
import singlecarrier_amd as sc

pytestmark = pytest.mark.gpu

KS_FRAMES = 1057            # keystream period in frames
G_PERIOD = 2 * KS_FRAMES    # period of everything the receive path takes from g


# ------------------------------------------------- A. the period on every back
@pytest.fixture(scope="module")
def long_stream():
    """130 clean channels x 1,070 frames and the oracle's outputs (read-only)."""
    x = oracle.synth(123, 130, 1070, 1000.0)
    bits, valid, tr = oracle.cpu_rx(x, trace=True)
    return rxcheck.frozen(x, bits, valid, tr)


@pytest.mark.parametrize("calls", [(1050, 20), (1056, 1, 1, 12)], ids=["1050+20", "1056+1+1+12"])
@pytest.mark.parametrize("shape,width", rxcheck.ALL_SHAPES)
def test_keystream_period_on_every_back(shape, width, calls, long_stream, monkeypatch):
    """The descrambler word is reduced mod 1057 once in the lane back (train:
    4x2, 2x4 dual, 1x8 W = 64) and once in the quad back (qtrain: W = 32, 16).
    Frame 1057 is crossed inside one persistent launch (1050 + 20), and calls
    start at g = 1056, 1057 and 1058 (1056 + 1 + 1 + 12)."""
    x, bits, valid, tr = long_stream
    assert valid[:, KS_FRAMES:].any(axis=1).sum() >= 100   # channels seen past the period
    rxcheck.force_shape(monkeypatch, shape, width)
    rx = sc.Receiver(x.shape[0])
    out = rxcheck.demod_in_calls(rx, x, calls)
    assert rx.frames == 1070
    rx.close()
    rxcheck.assert_same(out, (bits, valid, tr), f"{shape}/{width}, calls {calls}")


# ------------------------------------------- B. the drop-in and the stream
def test_drop_in_crosses_the_keystream_period():
    """qpsk_rx_frame() once per frame, 1,070 calls: the pinned tiny-call path
    (the job-counter parity calls & 1 alternating throughout) past g = 1057."""
    x1 = oracle.synth(124, 1, 1070, 1000.0)
    bits, valid, _ = oracle.cpu_rx(x1)
    assert valid[0, KS_FRAMES:].sum() >= 1
    sc.qpsk_rx_init()
    got_v = np.zeros(1070, np.uint8)
    got_b = np.zeros((1070, 62), np.uint8)
    for n in range(1070):
        got_v[n], got_b[n] = sc.qpsk_rx_frame(x1[0, n])
    np.testing.assert_array_equal(got_v, valid[0])
    vm = valid[0].astype(bool)
    np.testing.assert_array_equal(got_b[vm], bits[0][vm])


def test_stream_crosses_the_keystream_period(long_stream):
    """64 channels through a 3-slot qpsk_stream as 10 chunks of 107 frames."""
    nch, fpc, nchunk, nslot = 64, 107, 10, 3
    x, bits, valid, _ = long_stream
    assert valid[:nch, KS_FRAMES:].any()
    st = sc.Stream(nch, fpc, nslot=nslot)
    got_b, got_v = [], []
    for k in range(nchunk):
        buf = st.acquire()
        buf[...] = x[:nch, k * fpc:(k + 1) * fpc]
        st.submit()
        if st.pending == nslot:
            b, v = st.retrieve()
            got_b.append(b)
            got_v.append(v)
    while st.pending:
        b, v = st.retrieve()
        got_b.append(b)
        got_v.append(v)
    st.close()
    rxcheck.assert_same({"bits": np.concatenate(got_b, axis=1), "valid": np.concatenate(got_v, axis=1)},
                        {"bits": bits[:nch], "valid": valid[:nch]})


# ---------------------------------------- C. frame indices of 2^32 and beyond
def _frame_of(snap):
    return int(np.frombuffer(snap[24:32], "<u8")[0])


def _at_frame(snap, old, G):
    """The snapshot with StateHdr.frame (the little-endian uint64 at byte 24:
    after magic[8], version, hdr_bytes, mode and n) rewritten from `old` to G."""
    assert snap[:8] == b"QPSKSTA1" and len(snap) >= 64
    assert _frame_of(snap) == old, "StateHdr layout changed"
    return snap[:24] + np.array([G], "<u8").tobytes() + snap[32:]


@pytest.mark.parametrize("shape", [None, "4x2"], ids=["quad", "lane4x2"])
@pytest.mark.parametrize("seed,k,G", [(160, 1, 2**32 - 3), (161, 5, 2**32 + 1),
                                      (162, 3, 2114 * 2**31 + 3),
                                      (162, 3, 2114 * (2**63 // 2114) + 3)],
                         ids=["wrap-inside-call", "above-wrap", "far-above", "near-2^63"])
def test_frame_index_past_32_bits(seed, k, G, shape, monkeypatch):
    """The receive path depends on g only through g mod 2114 (1057-frame
    keystream x mixer sign), so channels really at frame k, declared to be at
    G = k + 2114 M by a snapshot header, must continue exactly as the oracle's
    plain run from 0 does: 8 more frames, with 2^32 inside the call, just below
    it and far below it.  qpsk_rx_frames() and the snapshots carry the full
    64-bit index.

    A kernel that saw only g mod 2^32 would descramble with word
    (g + 4 (g >> 32)) mod 1057 (2^32 mod 1057 = 4): wrong bits, everything else
    right.  It would still pass "far-above", whose G >> 32 is 1057 itself;
    "near-2^63" is the same input at an index where that does not cancel."""
    nch, more = 96, 8
    assert G % G_PERIOD == k and G + more < 2**64
    assert (4 * ((G + more) >> 32)) % KS_FRAMES != 0 or G == 2114 * 2**31 + 3
    x = oracle.synth(seed, nch, k + more, 1000.0)
    bits, valid, tr = oracle.cpu_rx(x, trace=True)
    assert valid[:, k:].sum(axis=0).min() >= 10   # every frame is observed through its bits
    rxcheck.force_shape(monkeypatch, shape, None)
    a = sc.Receiver(nch)
    a.demod(np.ascontiguousarray(x[:, :k]))
    snap = a.state_save()
    a.close()
    b = sc.Receiver(nch)
    b.state_load(_at_frame(snap, k, G))
    assert b.frames == G
    rest = b.demod(np.ascontiguousarray(x[:, k:]), trace=True, soft=True)
    assert b.frames == G + more
    snap2 = b.state_save()
    b.close()
    rxcheck.assert_same(rest, (bits[:, k:], valid[:, k:], tr[:, k:]), f"G = {G}")
    assert _frame_of(snap2) == G + more
    c = sc.Receiver(nch)
    c.state_load(snap2)
    assert c.frames == G + more
    c.close()


# --------------------------------------- D. one call of more than 2^32 samples
def test_call_of_more_than_2_to_32_samples():
    """70,001 channels x 33 frames = 4,342,862,040 samples in one call: element
    indices past 2^32 in the fronts' loads, carry_history and every output
    writer.  The input is 251 distinct channels (prime, so an index that wrapped
    by 2^32 elements cannot land on an identical channel at frame alignment)
    gathered on the device; outputs compare with the oracle's, gathered alike."""
    import torch
    nch, F, nu = 70001, 33, 251
    assert nch * F * sc.FRAME_SIZE == 4342862040 > 2**32
    first_above = -(-2**32 // (F * sc.FRAME_SIZE))
    assert first_above == 69230 and first_above * F * sc.FRAME_SIZE >= 2**32 > (first_above - 1) * F * sc.FRAME_SIZE
    if torch.cuda.mem_get_info()[0] < 16 * 2**30:
        pytest.skip("needs about 10 GB of device memory")
    u = oracle.synth(170, nu, F, 6.0)
    exp = rxcheck.expected(u)
    valid = exp["valid"]
    assert 0 < valid.sum() < valid.size
    idx = torch.arange(nch, device="cuda") % nu
    dx = torch.from_numpy(u).cuda()[idx]
    assert dx.is_contiguous() and dx.numel() > 2**32
    db = torch.zeros((nch, F, 62), dtype=torch.uint8, device="cuda")
    dv = torch.zeros((nch, F), dtype=torch.uint8, device="cuda")
    dt = torch.zeros((nch, F, 4), dtype=torch.int32, device="cuda")
    ds = torch.zeros((nch, F, 31, 2), dtype=torch.float32, device="cuda")
    rx = sc.Receiver(nch)
    rx.demod_device(dx, db, dv, dt, ds)
    rx.sync()
    assert rx.frames == F
    try:
        # 2.3 million channel-frames, compared where they are.  The rules are rxcheck.differences':
        # exp's soft symbols hold no NaN and are zero on invalid frames, so every bit is compared
        assert not np.isnan(exp["soft"]).any()
        for k, got in zip(rxcheck.KEYS, (db, dv, dt, ds.view(torch.int32))):
            want = torch.from_numpy(np.array(exp[k]).view(np.int32 if k == "soft" else exp[k].dtype)).cuda()[idx]
            assert got.shape == want.shape and got.dtype == want.dtype, k
            if not torch.equal(got, want):
                bad = (got != want).reshape(nch, F, -1).any(-1)
                raise AssertionError(f"{k} differs on {int(bad.sum())} channel-frames, "
                                     f"first at (channel, frame) {tuple(bad.nonzero()[0].tolist())}")
            del want
    finally:
        rx.close()
        del dx, db, dv, dt, ds, idx
        torch.cuda.empty_cache()


# ------------------------------------------------- E. kernel-time accounting
def test_kernel_time_accounting_folds_its_event_pool():
    """qpsk_rx_timing_*: 70 timed single-frame calls on one context overflow
    the 64-entry event pool, so pending spans fold into the running totals.
    The calls are serialised on one stream and every host call synchronises,
    so the summed kernel spans cannot exceed the host's span around them."""
    nch, timed, untimed = 64, 70, 3
    x = oracle.synth(171, nch, timed + untimed, 5.0)
    bits, valid, tr = oracle.cpu_rx(x, trace=True)
    rx = sc.Receiver(nch)
    rx.timing(True)
    parts = []
    t0 = time.perf_counter()
    for n in range(timed):   # written out: nothing but the calls inside the host's span
        parts.append(rx.demod(np.ascontiguousarray(x[:, n:n + 1]), trace=True, soft=True))
    host_ms = (time.perf_counter() - t0) * 1e3
    ms_rx, ms_data, frames = rx.collect_timing_split()
    print(f"rx_kernel {ms_rx:.3f} ms, rx_data_kernel {ms_data:.3f} ms, host {host_ms:.3f} ms")
    assert frames == timed
    assert ms_rx > 0 and ms_data > 0
    assert ms_rx + ms_data <= host_ms
    assert rx.collect_timing_split() == (0.0, 0.0, 0)
    rx.timing(False)
    parts.append(rxcheck.demod_in_calls(rx, x[:, timed:], [1] * untimed))
    assert rx.collect_timing_split() == (0.0, 0.0, 0)
    assert rx.collect_timing() == (0.0, 0)
    rx.close()
    out = {k: np.concatenate([p[k] for p in parts], axis=1) for k in rxcheck.KEYS}
    rxcheck.assert_same(out, (bits, valid, tr))
