"""Transmitter channels that come and go on the GPU (include/qpsk_tx.h
"Channels that come and go"; tx_plan_kernel and tx_mask_kernel of
singlecarrier_amd/csrc/qpsk_tx.hip) against the host twin
qpsk_tx_batch_masked_host, which tests/test_tx_mask_host.py pins to an
independent restatement.  Every comparison is exact equality of every element,
sentinels around the written block included.

The shape is 130 channels x 12 slots: 8 alignment classes x 16 looped channels
fill one block column and leave a ragged second one, and 12 slots cross the
carrier's transient at own index 8/9.  Gaps 903 (P odd), 0 (a tile spans two
packets, sometimes three) and 5."""
import functools

import numpy as np
import pytest

import gpu_delay
import singlecarrier_amd as sc
from tx_mask_cases import PACKET, Twin, last_dibits, masks, payload, snapshot, snapshot_fields

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NCH, NPK = 130, 12
GAPS = (903, 0, 5)
S16 = sc.OUT_S16 | sc.OUT_PLANAR
ALAW = sc.OUT_ALAW | sc.OUT_PLANAR                # through the modulator's fused store
ULAW_I = sc.OUT_ULAW | sc.OUT_INTERLEAVED         # int16 block and a conversion behind it
FMTS = (S16, ALAW, ULAW_I)
EINVAL = sc.QPSK_EINVAL


def _sentinel(fmt):
    return (0x5A5A, np.int16, torch.int16) if fmt & 0x0f == sc.OUT_S16 else (0x5A, np.uint8, torch.uint8)


def _block(fmt, nch, n):
    """(rows, ld) of a block with 5 foreign elements behind every row"""
    rows, least = (n, nch) if fmt & sc.OUT_INTERLEAVED else (nch, n)
    return rows, least + 5


def expected(y, fmt):
    """the int16 rows y [nch][n] as the block in format fmt, sentinel where no
    call may write: row tails, and foreign columns of an interleaved block"""
    nch, n = y.shape
    rows, ld = _block(fmt, nch, n)
    sent, dt, _ = _sentinel(fmt)
    exp = np.full((rows, ld), sent, dt)
    if fmt == S16:
        exp[:, :n] = y
    else:
        sc.output_convert_host(y, fmt, ld=ld, out=exp)
    return exp


def device_call(tx, bits, m, fmt, stream=None):
    """one call through the device entry points into a sentinel-filled block;
    the mask and the payload live in device memory"""
    nch, npk = bits.shape[:2]
    rows, ld = _block(fmt, nch, npk * (PACKET + tx.gap))
    sent, _, tdt = _sentinel(fmt)
    out = torch.full((rows, ld), sent, dtype=tdt, device="cuda")
    d_bits = torch.from_numpy(np.array(bits)).cuda()       # (a copy: the cached cases are read-only)
    d_m = None if m is None else torch.from_numpy(np.array(m)).cuda()
    if fmt == S16:
        tx.modulate_device(d_bits, out, stream=stream, active=d_m)
    else:
        tx.modulate_device_fmt(d_bits, out, fmt, stream=stream, active=d_m)
    tx.sync()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def mask_case(gap):
    """The masks test's inputs and the host twin's rows, once per gap: 12 masked
    slots, then 3 slots with every channel active, which filter over whatever
    dibits the first call left (row 3: its last active slot was not the last)."""
    twin = Twin(NCH)
    b0, m0, b1 = payload(10 + gap, NCH, NPK), masks(20 + gap, NCH, NPK), payload(30 + gap, NCH, 3)
    y0, y1 = twin.call(b0, gap, m0), twin.call(b1, gap)
    for a in (b0, m0, b1, y0, y1):
        a.setflags(write=False)
    return b0, m0, b1, y0, y1


@pytest.mark.parametrize("fmt", FMTS, ids=["s16", "alaw", "ulaw_i"])
@pytest.mark.parametrize("gap", GAPS)
def test_masks(gap, fmt):
    b0, m0, b1, y0, y1 = mask_case(gap)
    tx = sc.Transmitter(NCH, gap=gap)
    np.testing.assert_array_equal(device_call(tx, b0, m0, fmt), expected(y0, fmt))
    sent = (m0 != 0).sum(axis=1).astype(np.uint64)
    np.testing.assert_array_equal(tx.channel_packets(), sent)
    assert tx.packets() == NPK
    np.testing.assert_array_equal(device_call(tx, b1, None, fmt), expected(y1, fmt))
    np.testing.assert_array_equal(tx.channel_packets(), sent + np.uint64(3))
    assert tx.packets() == NPK + 3
    tx.close()


@pytest.mark.parametrize("fmt", FMTS, ids=["s16", "alaw", "ulaw_i"])
@pytest.mark.parametrize("gap", GAPS)
def test_mixed_indices_inside_one_channel_loop(gap, fmt):
    """9 slots on a uniform context, every third channel reset, 12 more slots:
    indices 0.. and 9.. side by side in every block, so both carrier signs, the
    transient rows and the stream-start periods share one 16-channel loop."""
    twin = Twin(NCH)
    tx = sc.Transmitter(NCH, gap=gap)
    b0, b1 = payload(40 + gap, NCH, 9), payload(50 + gap, NCH, NPK)
    np.testing.assert_array_equal(device_call(tx, b0, None, fmt), expected(twin.call(b0, gap), fmt))
    for c in range(0, NCH, 3):
        tx.reset_channels(c)
        twin.reset(c, 1)
    idx = np.where(np.arange(NCH) % 3 == 0, 0, 9).astype(np.uint64)
    np.testing.assert_array_equal(tx.channel_packets(), idx)
    m = masks(60 + gap, NCH, NPK)
    m[:16] = 1                                     # these cross 8/9 and 17/18 in step
    np.testing.assert_array_equal(device_call(tx, b1, m, fmt), expected(twin.call(b1, gap, m), fmt))
    np.testing.assert_array_equal(tx.channel_packets(), idx + (m != 0).sum(axis=1).astype(np.uint64))
    assert tx.packets() == 9 + NPK
    tx.close()


@pytest.mark.parametrize("fmt", FMTS, ids=["s16", "alaw", "ulaw_i"])
@pytest.mark.parametrize("gap", GAPS)
def test_equal_indices_on_a_general_context(gap, fmt):
    """A general context whose channels share one index, from the stream's
    start over the transient at 8/9: the general kernel where the uniform one
    would have done.  A masked call follows in which the indices drift apart
    slot by slot."""
    twin = Twin(NCH)
    tx = sc.Transmitter(NCH, gap=gap)
    tx.reset_channels(5, 2)                        # general, and still every channel at 0
    b0, b1 = payload(170 + gap, NCH, NPK), payload(171 + gap, NCH, 5)
    np.testing.assert_array_equal(device_call(tx, b0, None, fmt), expected(twin.call(b0, gap), fmt))
    np.testing.assert_array_equal(tx.channel_packets(), np.full(NCH, NPK, np.uint64))
    m = masks(172 + gap, NCH, 5)
    np.testing.assert_array_equal(device_call(tx, b1, m, fmt), expected(twin.call(b1, gap, m), fmt))
    tx.close()


@pytest.mark.parametrize("gap", GAPS)
def test_call_sequences_are_equivalent(gap):
    """1 + 3 + 1 slots equal one call of 5 with the same mask rows, and masked,
    plain and format calls alternate on one context, host and device forms."""
    bits, m = payload(70 + gap, NCH, 5), masks(71 + gap, NCH, 5)
    P = PACKET + gap
    whole = Twin(NCH).call(bits, gap, m)
    one = sc.Transmitter(NCH, gap=gap)
    np.testing.assert_array_equal(one.modulate(bits, active=m), whole)
    tx = sc.Transmitter(NCH, gap=gap)
    parts = [tx.modulate(bits[:, lo:hi], active=m[:, lo:hi]) for lo, hi in ((0, 1), (1, 4), (4, 5))]
    np.testing.assert_array_equal(np.concatenate(parts, axis=1), whole)
    # both go on: plain host call, masked interleaved mu-law, plain A-law, masked device call
    twin = Twin(NCH)
    twin.call(bits, gap, m)
    for step, (fmt, masked) in enumerate(((S16, False), (ULAW_I, True), (ALAW, False), (S16, True))):
        b = payload(80 + step, NCH, 2)
        mm = masks(90 + step, NCH, 5)[:, :2].copy() if masked else None
        y = twin.call(b, gap, mm)
        if step == 0:
            np.testing.assert_array_equal(one.modulate(b), y)
            np.testing.assert_array_equal(tx.modulate(b), y)
        elif step < 3:
            rows, ld = _block(fmt, NCH, 2 * P)
            sent, dt, _ = _sentinel(fmt)
            for t in (one, tx):
                got = t.modulate_fmt(b, fmt, ld=ld, out=np.full((rows, ld), sent, dt), active=mm)
                np.testing.assert_array_equal(got, expected(y, fmt))
        else:
            for t in (one, tx):
                np.testing.assert_array_equal(device_call(t, b, mm, fmt), expected(y, fmt))
    np.testing.assert_array_equal(one.channel_packets(), tx.channel_packets())
    assert one.state_save() == tx.state_save()
    assert one.packets() == tx.packets() == 13
    one.close()
    tx.close()


def test_migration_to_a_context_of_another_gap():
    """Channels 100..129 of a 130-channel context move to channels 3..32 of a
    40-channel context of another gap and another packet count; both contexts
    continue as the host twin does, and equal states give equal bytes."""
    ga, gb, n = 903, 0, 30
    ta, tb = Twin(NCH), Twin(40)
    A, B = sc.Transmitter(NCH, gap=ga), sc.Transmitter(40, gap=gb)
    ba, ma = payload(100, NCH, 10), masks(101, NCH, 10)
    np.testing.assert_array_equal(A.modulate(ba, active=ma), ta.call(ba, ga, ma))
    bb = payload(102, 40, 3)
    np.testing.assert_array_equal(B.modulate(bb), tb.call(bb, gb))      # B is uniform, at 3
    snap = A.state_save(100, n)
    cnt, idx, words = snapshot_fields(snap)
    assert cnt == n
    np.testing.assert_array_equal(idx, (ma[100:] != 0).sum(axis=1))
    for i in range(n):
        k = np.flatnonzero(ma[100 + i])
        assert words[i] == (last_dibits(ba[100 + i, k[-1]]) if k.size else 0)
    B.state_load(snap, 3)
    tb.st[3:3 + n] = ta.st[100:]
    assert B.state_save(3, n) == snap                                   # equal states, equal bytes
    np.testing.assert_array_equal(B.channel_packets(), np.concatenate([[3] * 3, idx, [3] * 7]).astype(np.uint64))
    assert B.packets() == 3 and A.packets() == 10
    # the part of the snapshot that is the whole of a smaller one
    assert snapshot(idx[:4], words[:4]) == A.state_save(100, 4)
    for step in range(2):
        ba, ma = payload(110 + step, NCH, 4), masks(111 + step, NCH, 5)[:, :4].copy()
        bb, mb = payload(120 + step, 40, 4), masks(121 + step, 40, 5)[:, :4].copy()
        np.testing.assert_array_equal(A.modulate(ba, active=ma), ta.call(ba, ga, ma))
        np.testing.assert_array_equal(B.modulate(bb, active=mb), tb.call(bb, gb, mb))
    # a plain reset makes B uniform again: every channel a fresh stream
    B.reset()
    assert B.packets() == 0 and not B.channel_packets().any()
    np.testing.assert_array_equal(B.modulate(bb), sc.tx_batch_host(bb, gap=gb))
    A.close()
    B.close()


def test_snapshots_that_are_refused_change_nothing():
    nch, gap = 8, 5
    tx = sc.Transmitter(nch, gap=gap)
    bits = payload(130, nch, 2)
    y = sc.tx_batch_host(bits, gap=gap)
    np.testing.assert_array_equal(tx.modulate(bits[:, :1]), y[:, :PACKET + gap])
    good = tx.state_save(2, 3)
    L, h = sc.lib(), tx._h

    def load(snap, c0=2, n=3, size=None):
        buf = np.frombuffer(snap, np.uint8).copy()
        return L.qpsk_tx_state_load(h, c0, n, sc._ptr(buf), buf.size if size is None else size)

    n, idx, words = snapshot_fields(good)
    head = lambda *w: np.array(w, "<u4").tobytes() + good[16:]
    assert load(good[:-1]) == EINVAL                                     # short
    assert load(good, size=15) == EINVAL
    assert load(b"QPSKSTA1" + good[8:]) == EINVAL                        # foreign: the receive side's magic
    assert load(head(0x53585451, 2, 3, 0)) == EINVAL                     # another version
    assert load(head(0x53585451, 1, 4, 0)) == EINVAL                     # another n
    assert load(head(0x53585451, 1, 3, 1)) == EINVAL
    assert load(snapshot(idx, words | np.uint32(1 << 9))) == EINVAL      # a bit outside the 9 dibits
    assert load(snapshot([0, 1, 1], words)) == EINVAL                    # dibits at index 0
    assert load(good, c0=6) == EINVAL and load(good, c0=-1) == EINVAL    # a range outside the context
    assert L.qpsk_tx_state_load(h, 2, 3, None, len(good)) == EINVAL
    buf = np.zeros(len(good), np.uint8)
    assert L.qpsk_tx_state_save(h, 2, 3, sc._ptr(buf), len(good) - 1) == EINVAL
    assert L.qpsk_tx_state_save(h, 2, 0, sc._ptr(buf), len(good)) == EINVAL
    assert L.qpsk_tx_state_save(h, 6, 3, sc._ptr(buf), len(good)) == EINVAL
    assert not buf.any()
    out = np.zeros(nch, np.uint64)
    assert L.qpsk_tx_channel_packets(h, 0, nch + 1, sc._ptr(out)) == EINVAL
    assert L.qpsk_tx_channel_packets(h, 0, 1, None) == EINVAL
    assert L.qpsk_tx_channel_packets(h, nch, 0, None) == 0               # an empty range is a no-op
    for c0, k in ((-1, 1), (0, -1), (nch, 1), (1, nch), (0, 2**31 - 1)):
        assert L.qpsk_tx_reset_channels(h, c0, k) == EINVAL
    assert L.qpsk_tx_reset_channels(h, nch, 0) == 0
    # nothing of that moved the context: it is still the uniform one it was
    assert tx.state_save(2, 3) == good
    np.testing.assert_array_equal(tx.modulate(bits[:, 1:]), y[:, PACKET + gap:])
    assert load(good) == 0
    tx.close()


def test_an_index_past_2_to_the_32():
    """A snapshot edited to own index 2^33 + 9 with the dibits of a host run to
    index 9: odd and past the transient like 9, so the samples are those of the
    host twin continued from index 9."""
    nch, gap = 8, 5
    twin = Twin(nch)
    b0, b1 = payload(140, nch, 9), payload(141, nch, 4)
    twin.call(b0, gap)
    big = 2**33 + 9
    tx = sc.Transmitter(nch, gap=gap)
    tx.state_load(snapshot([big] * nch, [last_dibits(b0[c, 8]) for c in range(nch)]))
    m = masks(142, nch, 5)[:, :4].copy()
    np.testing.assert_array_equal(device_call(tx, b1, m, S16), expected(twin.call(b1, gap, m), S16))
    np.testing.assert_array_equal(tx.channel_packets(), np.uint64(big) + (m != 0).sum(axis=1).astype(np.uint64))
    _, idx, _ = snapshot_fields(tx.state_save())
    assert idx.dtype.itemsize == 8 and int(idx[5]) == big + 4
    tx.close()


def test_stream_order():
    """The masked device call reads mask and payload in stream order and waits
    for nothing: both arrive late on the stream, behind a delay, and are
    overwritten behind the call.  channel_packets, state_save and
    reset_channels wait for the call in flight."""
    nch, npk, gap, ms = NCH, 4, 5, 100.0
    P = PACKET + gap
    twin = Twin(nch)
    tx = sc.Transmitter(nch, gap=gap)
    S = torch.cuda.Stream()
    gpu_delay.put(S, 1.0).ms()                     # loads the delay kernel
    w_b, w_m = payload(150, nch, npk), masks(151, nch, npk)
    np.testing.assert_array_equal(device_call(tx, w_b, w_m, S16, stream=S)[:, :npk * P], twin.call(w_b, gap, w_m))
    sent = (w_m != 0).sum(axis=1).astype(np.uint64)

    def late_call(seed):
        """a masked call on S behind a delay; returns (the delay, was it running
        when the enqueue sequence ended, the clone of the call's rows, the mask)"""
        b, m = payload(seed, nch, npk), masks(seed + 1, nch, npk)
        pin_b, pin_m = torch.from_numpy(b).pin_memory(), torch.from_numpy(m).pin_memory()
        d_b = torch.from_numpy(1 - b).cuda()                             # decoys until the copies run
        d_m = torch.from_numpy((m == 0).astype(np.uint8)).cuda()
        out = torch.zeros((nch, npk * P), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        delay = gpu_delay.put(S, ms)
        with torch.cuda.stream(S):
            d_b.copy_(pin_b, non_blocking=True)
            d_m.copy_(pin_m, non_blocking=True)
        tx.modulate_device(d_b, out, stream=S, active=d_m)
        with torch.cuda.stream(S):
            keep = out.clone()
            d_b.zero_()
            d_m.fill_(1)
            out.fill_(0x5A5A)
        return delay, delay.running(), keep, b, m

    delay, running, keep, b, m = late_call(152)
    idx = tx.channel_packets()                                           # waits for the call
    assert not delay.running()
    sent += (m != 0).sum(axis=1).astype(np.uint64)
    np.testing.assert_array_equal(idx, sent)
    assert running, "the delay had ended when the enqueue sequence returned: the call waited"
    assert delay.ms() >= 0.9 * ms
    np.testing.assert_array_equal(keep.cpu().numpy(), twin.call(b, gap, m))

    delay, running, keep, b, m = late_call(154)
    snap = tx.state_save()                                               # waits for the call
    assert not delay.running() and running
    sent += (m != 0).sum(axis=1).astype(np.uint64)
    np.testing.assert_array_equal(snapshot_fields(snap)[1], sent)
    np.testing.assert_array_equal(keep.cpu().numpy(), twin.call(b, gap, m))

    delay, running, keep, b, m = late_call(156)
    tx.reset_channels(0, 16)                                             # waits: the call still sends from the old state
    assert not delay.running() and running
    np.testing.assert_array_equal(keep.cpu().numpy(), twin.call(b, gap, m))
    sent += (m != 0).sum(axis=1).astype(np.uint64)
    sent[:16] = 0
    np.testing.assert_array_equal(tx.channel_packets(), sent)
    twin.reset(0, 16)
    b = payload(158, nch, 2)
    np.testing.assert_array_equal(tx.modulate(b), twin.call(b, gap))
    tx.close()


def test_an_untouched_context_is_as_before():
    """No new call, or only their NULL-mask forms and the two reads: the
    context stays uniform and gives the plain calls' results over any calls."""
    nch, gap = NCH, 903
    bits = payload(160, nch, 11)
    y = sc.tx_batch_host(bits, gap=gap)
    P = PACKET + gap
    plain, nulls = sc.Transmitter(nch, gap=gap), sc.Transmitter(nch, gap=gap)
    a = np.concatenate([plain.modulate(bits[:, lo:hi]) for lo, hi in ((0, 2), (2, 9), (9, 11))], axis=1)
    np.testing.assert_array_equal(a, y)
    parts = []
    for lo, hi in ((0, 2), (2, 9), (9, 11)):
        parts.append(nulls.modulate(bits[:, lo:hi], active=None))
        np.testing.assert_array_equal(nulls.channel_packets(), np.full(nch, hi, np.uint64))
        assert nulls.state_save() == snapshot([hi] * nch, [last_dibits(bits[c, hi - 1]) for c in range(nch)])
    np.testing.assert_array_equal(np.concatenate(parts, axis=1), y)
    assert plain.packets() == nulls.packets() == 11
    assert plain.state_save() == nulls.state_save()
    assert y.shape == (nch, 11 * P)
    plain.close()
    nulls.close()
