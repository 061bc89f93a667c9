"""Channels that come and go: qpsk_rx_reset_channels, qpsk_rx_channel_frames
and qpsk_rx_state_join (run with -m gpu).

Every channel of a context has a frame index of its own.  A channel reset or
joined on its own keeps the context's mixer sign and state parity; only its
descrambler word is moved, in rx_data_kernel (koff).  That is exact because the
receiver is even in its input (tests/test_channel_index.py pins that on the
CPU); here the kernels themselves are checked at odd and at even distances
between a channel's index and its context's, on the quad and the lane backs, the
pinned tiny-call path and a stream.

Every expected value is the oracle's (oracle.cpu_rx) on the channel's own
sub-stream from its latest start; every comparison is tests/rxcheck.py's.
"""
import numpy as np
import pytest

import oracle
import rxcheck
import singlecarrier_amd as sc
from traffic import at_frame as _at_frame, frame_of as _frame_of, keywords as _keywords

pytestmark = pytest.mark.gpu

MODES = [sc.MODE_REFERENCE, sc.MODE_DEC752]
MODE_IDS = ["reference", "dec752"]


def _sub(out, chans, frames=slice(None)):
    return {k: v[chans][:, frames] for k, v in out.items()}


def _clip(ranges, nch):
    """Channel ranges [a, b) clipped to a context of nch channels (a < 0: from the end)."""
    out = []
    for a, b in ranges:
        a, b = (nch + a, nch + b) if a < 0 else (a, b)
        out.append((a, min(b, nch)))
    return out


def _come_and_go(nch, mode, calls, resets, seed):
    """calls: frames per call; resets[i]: channel ranges reset after call i.
    Feeds noiseless synth through one Receiver and checks every channel against
    the oracle on its sub-streams; returns nothing."""
    nf = sum(calls)
    x = oracle.synth(seed, nch, nf, 1000.0)
    edges = np.concatenate([[0], np.cumsum(calls)])
    # per channel: the frames at which it (re)starts
    starts = [[0] for _ in range(nch)]
    for i, ranges in enumerate(resets):
        for a, b in _clip(ranges, nch):
            assert 0 <= a < b <= nch
            for c in range(a, b):
                if starts[c][-1] != edges[i + 1]:
                    starts[c].append(int(edges[i + 1]))
    rx = sc.Receiver(nch, mode=mode)
    parts = []
    for i, n in enumerate(calls):
        parts.append(rx.demod(np.ascontiguousarray(x[:, edges[i]:edges[i + 1]]), trace=True, soft=True))
        assert rx.frames == edges[i + 1]
        if i < len(resets):
            for a, b in _clip(resets[i], nch):
                rx.reset_channels(a, b - a)
            own = rx.channel_frames()
            want = [int(edges[i + 1]) - max(s for s in starts[c] if s <= edges[i + 1]) for c in range(nch)]
            np.testing.assert_array_equal(own, np.asarray(want, np.uint64))
    rx.close()
    got = {k: np.concatenate([p[k] for p in parts], axis=1) for k in rxcheck.KEYS}
    # channels with the same starts share an oracle run per segment
    groups = {}
    for c in range(nch):
        groups.setdefault(tuple(starts[c]), []).append(c)
    assert (0,) in groups, "no untouched channel"
    for st, chans in groups.items():
        seg = list(st) + [nf]
        for a, b in zip(seg[:-1], seg[1:]):
            exp = rxcheck.expected(x[chans, a:b], mode)
            # each (range, segment) must be observed through a valid frame
            for ra, rb in ([(0, nch)] if st == (0,) else
                           [r for rs in resets for r in _clip(rs, nch)]):
                inr = [k for k, c in enumerate(chans) if ra <= c < rb]
                if inr:
                    assert exp["valid"][inr].any(), f"no valid frame: channels [{ra}, {rb}) frames [{a}, {b})"
            rxcheck.assert_same(_sub(got, chans, slice(a, b)), exp, f"starts {st}, frames [{a}, {b})")


# ------------------------------------------------------------- A. come and go
# [1, 2): inside the first quad group; [61, 131): across a wave of 64 and the
# end of a 130-channel context; (-1, 0): the last channel
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("nch,shape", [(130, None), (4500, "4x2")], ids=["quad130", "lane4500"])
def test_channels_come_and_go(nch, shape, mode, monkeypatch):
    """3 frames, reset [61, 131) at context frame 3 (odd), 5 frames, reset
    [1, 2) and the last channel at context frame 8 (even), 4 frames.  130
    channels run the quad backs; 4,500 would too (lane backs start above 8,192
    channels), so that case forces the 4x2 shape, whose backs are lane backs."""
    rxcheck.force_shape(monkeypatch, shape, None)
    _come_and_go(nch, mode, (3, 5, 4), [[(61, 131)], [(1, 2), (-1, 0)]], seed=11)


# --------------------------------------------------------------- B. tiny call
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("F", [3, 5])
def test_tiny_calls_reset_one_channel(F, mode):
    """2 channels x F frames is at most 64 channel-frames: the kernels run on
    the pinned staging block (F is no power of two: channel = cf / F).  Channel
    1 restarts at context frames F and 2 F."""
    _come_and_go(2, mode, (F, F, F), [[(1, 2)], [(1, 2)]], seed=11)


# ---------------------------------------------------------- C. keystream wrap
def test_keystream_wraps_inside_a_call():
    """A context at index 1055 (a fresh snapshot with an edited header), 64
    channels joined at own indices 0, 1, 1056, 2113 and 2^32 + 5 after two real
    frames, then 4 frames: the call's word runs 1055, 1056, 0, 1 and every
    channel's own word passes 1057 or starts past it.  Expected: the oracle's
    6-frame run, its bits moved from the keystream words of frames 2.. to the
    channel's own (tests/test_channel_index.py: a start at another index
    changes nothing else)."""
    nch, k, more = 64, 2, 4
    owns = [0, 1, 1056, 2113, 2**32 + 5]
    cut = [0, 13, 26, 39, 52, 64]
    x = oracle.synth(31, nch, k + more, 1000.0)
    exp = rxcheck.expected(x, sc.MODE_REFERENCE)
    src = sc.Receiver(nch)
    src.demod(np.ascontiguousarray(x[:, :k]))
    snaps = [src.state_save(cut[i], cut[i + 1] - cut[i]) for i in range(len(owns))]
    src.close()
    rx = sc.Receiver(nch)
    rx.state_load(_at_frame(rx.state_save(), 0, 1055))
    assert rx.frames == 1055
    for i, G in enumerate(owns):
        rx.state_join(_at_frame(snaps[i], k, G), cut[i])
    want = np.concatenate([np.full(cut[i + 1] - cut[i], G, np.uint64) for i, G in enumerate(owns)])
    np.testing.assert_array_equal(rx.channel_frames(), want)
    got = rx.demod(np.ascontiguousarray(x[:, k:]), trace=True, soft=True)
    assert rx.frames == 1055 + more
    np.testing.assert_array_equal(rx.channel_frames(), want + np.uint64(more))
    for i, G in enumerate(owns):
        ch = slice(cut[i], cut[i + 1])
        e = _sub(exp, ch, slice(k, None))
        vm = e["valid"].astype(bool)
        assert vm.any(axis=0).all(), "a frame of the call is not observed in this group"
        e["bits"] = np.where(vm[..., None], e["bits"] ^ _keywords(k, more)[None] ^ _keywords(G, more)[None], 0)
        rxcheck.assert_same(_sub(got, ch), e, f"own index {G}")
        # a snapshot carries the exact 64-bit index
        assert _frame_of(rx.state_save(cut[i], cut[i + 1] - cut[i])) == G + more
    rx.close()


# ------------------------------------------------- D. migration and snapshots
@pytest.fixture(scope="module")
def migration():
    """Context A: 130 channels, 7 frames, channels 10..49 saved.  Context B: 64
    channels at frame 4; the snapshot joins its channels 3..42 (own index 7,
    context index 4: an odd distance) and B receives 9 more frames.  Returns
    what the tests compare (read-only)."""
    xa = oracle.synth(41, 130, 18, 1000.0)
    xb = oracle.synth(42, 64, 13, 1000.0)
    a = sc.Receiver(130)
    a.demod(np.ascontiguousarray(xa[:, :7]))
    snap = a.state_save(10, 40)
    a.close()
    b = sc.Receiver(64)
    first = b.demod(np.ascontiguousarray(xb[:, :4]), trace=True, soft=True)
    b.state_join(snap, 3)
    own = b.channel_frames()
    xin = xb[:, 4:].copy()
    xin[3:43] = xa[10:50, 7:16]
    rest = b.demod(xin, trace=True, soft=True)
    res = {"xa": xa, "xb": xb, "snap": snap, "first": first, "rest": rest, "own": own,
           "own_after": b.channel_frames(), "frames": b.frames,
           "snap_joined": b.state_save(3, 40), "snap_other": b.state_save(43, 21)}
    with pytest.raises(sc.QpskError) as ei:
        b.state_save(0, 64)
    res["mixed_code"] = ei.value.code
    with pytest.raises(sc.QpskError) as ei:
        b.state_save(2, 2)
    res["mixed_edge_code"] = ei.value.code
    b.close()
    return res


def test_migration_continues_the_channels_stream(migration):
    m = migration
    assert _frame_of(m["snap"]) == 7 and m["frames"] == 13
    want = np.full(64, 4, np.uint64)
    want[3:43] = 7
    np.testing.assert_array_equal(m["own"], want)
    np.testing.assert_array_equal(m["own_after"], want + np.uint64(9))
    ea = rxcheck.expected(m["xa"][10:50, :16], sc.MODE_REFERENCE)
    assert ea["valid"][:, 7:].any(axis=1).sum() >= 30 and ea["valid"][:, 7:].any(axis=0).all()
    rxcheck.assert_same(_sub(m["rest"], slice(3, 43)), _sub(ea, slice(None), slice(7, 16)), "joined channels")
    eb = rxcheck.expected(m["xb"], sc.MODE_REFERENCE)
    others = np.r_[0:3, 43:64]
    assert eb["valid"][others, 4:].any()
    rxcheck.assert_same(m["first"], _sub(eb, slice(None), slice(0, 4)), "B before the join")
    rxcheck.assert_same(_sub(m["rest"], others), _sub(eb, others, slice(4, 13)), "B's own channels")


def test_snapshots_of_joined_ranges(migration):
    """A range with two indices has no snapshot (QPSK_EINVAL).  A joined range's
    snapshot is, byte for byte, the one of a context that received the same 16
    frames with no join; qpsk_rx_state_load takes it under its old rules."""
    m = migration
    assert m["mixed_code"] == sc.QPSK_EINVAL and m["mixed_edge_code"] == sc.QPSK_EINVAL
    assert _frame_of(m["snap_joined"]) == 16 and _frame_of(m["snap_other"]) == 13
    xa = m["xa"]
    c = sc.Receiver(40)
    c.demod(np.ascontiguousarray(xa[10:50, :16]))
    plain = c.state_save()
    assert m["snap_joined"] == plain
    with pytest.raises(sc.QpskError) as ei:   # the old rule: one index per context
        c.state_load(m["snap"])
    assert ei.value.code == sc.QPSK_EINVAL
    c.close()
    d = sc.Receiver(40)
    d.state_load(m["snap_joined"])
    assert d.frames == 16 and (d.channel_frames() == 16).all()
    got = d.demod(np.ascontiguousarray(xa[10:50, 16:]), trace=True, soft=True)
    d.close()
    e = rxcheck.expected(xa[10:50], sc.MODE_REFERENCE)
    assert e["valid"][:, 16:].any()
    rxcheck.assert_same(got, _sub(e, slice(None), slice(16, 18)), "loaded from a joined range's snapshot")


def test_snapshot_of_a_reset_range_and_load_after_it():
    """A range reset on its own at an odd context frame gives the bytes of a
    fresh context fed the same frames; qpsk_rx_state_load puts a range back on
    the context's index."""
    x = oracle.synth(43, 8, 8, 1000.0)
    rx = sc.Receiver(8)
    rx.demod(np.ascontiguousarray(x[:, :3]))
    keep = rx.state_save(2, 3)
    rx.reset_channels(2, 3)
    assert rx.state_save(2, 3) == sc.Receiver(3).state_save()
    rx.demod(np.ascontiguousarray(x[:, 3:]))
    f = sc.Receiver(3)
    f.demod(np.ascontiguousarray(x[2:5, 3:]))
    assert rx.state_save(2, 3) == f.state_save()
    f.close()
    np.testing.assert_array_equal(rx.channel_frames(), np.asarray([8, 8, 5, 5, 5, 8, 8, 8], np.uint64))
    # the context's own index is 8: a snapshot at 3 is refused, one at 8 loads
    with pytest.raises(sc.QpskError) as ei:
        rx.state_load(keep, 2)
    assert ei.value.code == sc.QPSK_EINVAL
    rx.state_load(rx.state_save(5, 3), 2)
    assert (rx.channel_frames() == 8).all()
    rx.state_save()   # one index again
    rx.close()


def test_argument_and_assembly_errors():
    L = sc.lib()
    rx = sc.Receiver(8)
    out = np.zeros(8, np.uint64)
    for c0, n in ((-1, 1), (0, 0), (0, 9), (8, 1), (5, 4)):
        assert L.qpsk_rx_reset_channels(rx._h, c0, n) == sc.QPSK_EINVAL
        assert L.qpsk_rx_channel_frames(rx._h, c0, n, out.ctypes.data) == sc.QPSK_EINVAL
    assert L.qpsk_rx_reset_channels(None, 0, 1) == sc.QPSK_EINVAL
    assert L.qpsk_rx_channel_frames(rx._h, 0, 8, None) == sc.QPSK_EINVAL
    # a partial load at G != 0 into a fresh context: channels still to be loaded
    snap = _at_frame(rx.state_save(0, 4), 0, 6)
    rx.state_load(snap, 0)
    for call in (lambda: rx.reset_channels(0, 1), lambda: rx.state_join(snap, 4)):
        with pytest.raises(sc.QpskError) as ei:
            call()
        assert ei.value.code == sc.QPSK_EINVAL
    rx.state_load(snap, 4)
    rx.reset_channels(0, 1)
    np.testing.assert_array_equal(rx.channel_frames(), np.asarray([0] + [6] * 7, np.uint64))
    # a snapshot of another mode or size is refused by the join as by the load
    with pytest.raises(sc.QpskError) as ei:
        rx.state_join(snap, 0, 3)
    assert ei.value.code == sc.QPSK_EINVAL
    rx.reset()
    assert (rx.channel_frames() == 0).all() and rx.frames == 0
    rx.close()


# ------------------------------------------------------------------ E. streams
def test_stream_context_resets_channels_between_chunks():
    """qpsk_rx_reset_channels on a stream's context: QPSK_EBUSY with a chunk
    pending; after the drain it succeeds and the next chunk follows the oracle
    (channels 5..14 from a fresh start, the others continuing)."""
    nch, fpc = 64, 3
    x = oracle.synth(51, nch, 2 * fpc, 1000.0)
    st = sc.Stream(nch, fpc, nslot=2)
    L = sc.lib()
    ctx = L.qpsk_stream_ctx(st._h)
    st.acquire()[...] = x[:, :fpc]
    st.submit()
    assert L.qpsk_rx_reset_channels(ctx, 5, 10) == sc.QPSK_EBUSY
    b0, v0 = st.retrieve()
    assert st.pending == 0
    assert L.qpsk_rx_reset_channels(ctx, 5, 10) == 0
    st.acquire()[...] = x[:, fpc:]
    st.submit()
    b1, v1 = st.retrieve()
    st.close()
    e = rxcheck.expected(x, sc.MODE_REFERENCE)
    rxcheck.assert_same({"bits": b0, "valid": v0}, _sub(e, slice(None), slice(0, fpc)))
    others = np.r_[0:5, 15:nch]
    assert e["valid"][others, fpc:].any()
    rxcheck.assert_same({"bits": b1[others], "valid": v1[others]}, _sub(e, others, slice(fpc, None)))
    fresh = rxcheck.expected(x[5:15, fpc:], sc.MODE_REFERENCE)
    assert fresh["valid"].any()
    rxcheck.assert_same({"bits": b1[5:15], "valid": v1[5:15]}, fresh)


# ---------------------------------------------------------- F. stalled context
def test_stalled_context_refuses_a_channel_reset(monkeypatch):
    """After a stall every channel's state is undefined and the context's epoch
    stays open: qpsk_rx_reset_channels returns QPSK_ESTALL until qpsk_rx_reset."""
    x = oracle.synth(52, 96, 2, 1000.0)
    monkeypatch.setenv("QPSK_DEBUG_STALL", "first")
    rx = sc.Receiver(96)   # a dual-chain shape: it has the progress waits
    monkeypatch.delenv("QPSK_DEBUG_STALL")
    with pytest.raises(sc.QpskError) as ei:
        rx.demod(x)
    assert ei.value.code == sc.QPSK_ESTALL
    with pytest.raises(sc.QpskError) as ei:
        rx.reset_channels(0, 4)
    assert ei.value.code == sc.QPSK_ESTALL
    rx.reset()
    rx.reset_channels(0, 4)
    got = rx.demod(x, trace=True, soft=True)
    rx.close()
    rxcheck.assert_same(got, rxcheck.expected(x, sc.MODE_REFERENCE))
