"""Records behind the receive (include/qpsk_compact.h): the context-bound calls,
the record stream and the C example against the host compaction of the dense
outputs that the plain calls give on the same input.  Run with -m gpu."""
import gc
import os
import subprocess

import numpy as np
import pytest

import singlecarrier_amd as sc
from g711 import compress
from rxcheck import live_handles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = [sc.REC_BY_CHANNEL, sc.REC_BY_FRAME]
# 300 channels take the quad backs, 4,500 the lane backs
SHAPES = [(300, 12), (4500, 6)]
EBN0 = 5.0


@pytest.fixture(scope="module")
def cases():
    """(nch, nf) -> (input, the dense outputs of a fresh receiver); made once, never changed"""
    out = {}
    for nch, nf in SHAPES:
        x = sc.synth_device(41, nch, nf, EBN0).cpu().numpy()
        rx = sc.Receiver(nch)
        out[nch, nf] = (x, rx.demod(x, trace=True, soft=True))
        rx.close()
        n = int(out[nch, nf][1]["valid"].sum())
        assert 0 < n < nch * nf   # neither an empty list nor a full one
    return out


def _expect(d, order, cap=None, rows=True):
    return sc.compact_host(d["bits"], d["valid"], d["trace"] if rows else None, d["soft"] if rows else None,
                           order=order, cap=cap)


def _same(got, exp, rows=True):
    assert got["count"] == exp["count"]
    np.testing.assert_array_equal(got["groups"], exp["groups"])
    assert got["rec"].tobytes() == exp["rec"].tobytes()
    if rows:
        np.testing.assert_array_equal(got["trace"], exp["trace"])
        assert got["soft"].tobytes() == exp["soft"].tobytes()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", SHAPES)
def test_demod_records_equals_compaction_of_demod(cases, shape, order):
    x, d = cases[shape]
    rx = sc.Receiver(shape[0])
    got = rx.demod_records(x, order=order, trace=True, soft=True)
    rx.close()
    exp = _expect(d, order)
    assert 0 < got["count"] < shape[0] * shape[1]
    assert len(got["rec"]) == got["count"]
    _same(got, exp)


@pytest.mark.parametrize("order", ORDERS)
def test_cap_and_plain_records(cases, order):
    """cap below the count: the full count, cap rows; without trace / soft"""
    x, d = cases[SHAPES[0]]
    full = _expect(d, order, rows=False)
    cap = full["count"] // 2
    rx = sc.Receiver(SHAPES[0][0])
    got = rx.demod_records(x, order=order, cap=cap)
    rx.close()
    assert got["count"] == full["count"] and len(got["rec"]) == cap
    _same(got, _expect(d, order, cap=cap, rows=False), rows=False)
    rx = sc.Receiver(SHAPES[0][0])
    got = rx.demod_records(x, order=order, cap=0)   # a pure count
    rx.close()
    assert got["count"] == full["count"] and len(got["rec"]) == 0
    np.testing.assert_array_equal(got["groups"], full["groups"])


@pytest.mark.parametrize("order", ORDERS)
def test_split_calls_concatenate(cases, order):
    """5 + 7 frames: the two lists, the second with its frames moved on by 5,
    are the 12-frame list (merged by frame for by-channel order)."""
    x, d = cases[SHAPES[0]]
    exp = _expect(d, order)
    rx = sc.Receiver(SHAPES[0][0])
    a = rx.demod_records(np.ascontiguousarray(x[:, :5]), order=order, trace=True, soft=True)
    assert rx.frames == 5
    b = rx.demod_records(np.ascontiguousarray(x[:, 5:]), order=order, trace=True, soft=True)
    rx.close()
    rb = b["rec"].copy()
    rb["frame"] += 5
    rec = np.concatenate([a["rec"], rb])
    tr, so = np.concatenate([a["trace"], b["trace"]]), np.concatenate([a["soft"], b["soft"]])
    if order == sc.REC_BY_CHANNEL:   # a channel's frames of both calls side by side
        k = np.lexsort((rec["frame"], rec["channel"]))
        rec, tr, so = rec[k], tr[k], so[k]
    assert a["count"] + b["count"] == exp["count"]
    assert rec.tobytes() == exp["rec"].tobytes()
    np.testing.assert_array_equal(tr, exp["trace"])
    assert so.tobytes() == exp["soft"].tobytes()


@pytest.mark.parametrize("order", ORDERS)
def test_format_call_on_interleaved_alaw(order):
    nch, nf = 130, 6
    x = sc.synth_device(43, nch, nf, EBN0).cpu().numpy()
    fmt = sc.IN_ALAW | sc.IN_INTERLEAVED
    codes = np.ascontiguousarray(compress(x.reshape(nch, -1), sc.OUT_ALAW).T)
    rx = sc.Receiver(nch)
    d = rx.demod_fmt(codes, fmt, trace=True, soft=True)
    rx.close()
    assert 0 < d["valid"].sum() < nch * nf
    rx = sc.Receiver(nch)
    got = rx.demod_records_fmt(codes, fmt, order=order, trace=True, soft=True)
    rx.close()
    _same(got, _expect(d, order))


@pytest.mark.parametrize("order", ORDERS)
def test_device_call_on_a_side_stream(cases, order):
    import torch
    x, d = cases[SHAPES[0]]
    nch, nf = SHAPES[0]
    exp = _expect(d, order)
    dx = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    rx = sc.Receiver(nch)
    o = rx.demod_records_device(dx, order=order, trace=True, soft=True, stream=side)
    rx.sync()
    side.synchronize()
    count = int(o["count"].cpu().numpy().view(np.uint32)[0])
    got = {"count": count, "groups": o["groups"].cpu().numpy().view(np.uint32),
           "rec": sc.rec_from_tensor(o["rec"], count), "trace": o["trace"][:count].cpu().numpy(),
           "soft": o["soft"][:count].cpu().numpy()}
    rx.close()
    _same(got, exp)


def test_stalled_context_reports_estall(monkeypatch):
    import oracle
    x = oracle.synth(162, 96, 6, 4.0)
    monkeypatch.setenv("QPSK_DEBUG_STALL", "first")
    rx = sc.Receiver(96)   # 96 channels: a dual-chain shape
    monkeypatch.delenv("QPSK_DEBUG_STALL")
    with pytest.raises(sc.QpskError) as ei:
        rx.demod_records(x)
    assert ei.value.code == sc.QPSK_ESTALL
    rx.reset()
    got = rx.demod_records(x)   # the knob stalls the first launch only
    rx.close()
    rx = sc.Receiver(96)
    d = rx.demod(x)
    rx.close()
    assert got["rec"].tobytes() == sc.compact_host(d["bits"], d["valid"])["rec"].tobytes()


def _feed(st, x, fpc, nchunk, take):
    got = []
    for k in range(nchunk):
        st.acquire()[...] = x[:, k * fpc:(k + 1) * fpc]
        st.submit()
        if st.pending == st.nslot:
            got.append(take())
    while st.pending:
        got.append(take())
    return got


@pytest.mark.parametrize("order", ORDERS)
def test_record_stream_equals_plain_stream(order):
    nch, fpc, nchunk = 130, 4, 5
    x = sc.synth_device(44, nch, fpc * nchunk, EBN0).cpu().numpy()
    gc.collect()
    live = live_handles()
    plain = sc.Stream(nch, fpc, nslot=3)
    dense = _feed(plain, x, fpc, nchunk, plain.retrieve)
    with pytest.raises(sc.QpskError) as ei:   # a record retrieve on a plain stream
        plain.acquire()
        plain.submit()
        plain.retrieve_records()
    assert ei.value.code == sc.QPSK_EINVAL
    plain.retrieve()
    plain.close()
    st = sc.Stream(nch, fpc, nslot=3, records=True, order=order)
    recs = _feed(st, x, fpc, nchunk, st.retrieve_records)
    st.acquire()[...] = x[:, :fpc]
    st.submit()
    with pytest.raises(sc.QpskError) as ei:   # a plain retrieve on a record stream
        st.retrieve()
    assert ei.value.code == sc.QPSK_EINVAL
    assert st.pending == 1
    st.retrieve_records()
    st.close()
    assert live_handles() == live
    assert len(recs) == len(dense) == nchunk
    total = 0
    for (b, v), r in zip(dense, recs):
        exp = sc.compact_host(b, v, order=order)
        assert r["count"] == exp["count"]
        assert r["rec"].tobytes() == exp["rec"].tobytes()
        np.testing.assert_array_equal(r["groups"], exp["groups"])
        total += r["count"]
    assert 0 < total < nch * fpc * nchunk


def test_record_stream_with_a_small_cap():
    nch, fpc, nchunk = 130, 4, 5
    x = sc.synth_device(44, nch, fpc * nchunk, EBN0).cpu().numpy()
    plain = sc.Stream(nch, fpc, nslot=2)
    dense = _feed(plain, x, fpc, nchunk, plain.retrieve)
    plain.close()
    cap = 7
    assert max(int(v.sum()) for _, v in dense) > cap
    st = sc.Stream(nch, fpc, nslot=2, records=True, order=sc.REC_BY_FRAME, cap=cap)
    recs = _feed(st, x, fpc, nchunk, st.retrieve_records)
    st.close()
    for (b, v), r in zip(dense, recs):
        exp = sc.compact_host(b, v, order=sc.REC_BY_FRAME, cap=cap)
        assert r["count"] == exp["count"] == int(v.sum())
        assert len(r["rec"]) == min(cap, r["count"])
        assert r["rec"].tobytes() == exp["rec"].tobytes()
        np.testing.assert_array_equal(r["groups"], exp["groups"])


def test_record_stream_reports_a_stalled_chunk(monkeypatch):
    import oracle
    nch, fpc = 96, 3
    x = oracle.synth(18, nch, 2 * fpc, 6.0)
    monkeypatch.setenv("QPSK_DEBUG_STALL", "1")
    st = sc.Stream(nch, fpc, nslot=2, records=True)
    monkeypatch.delenv("QPSK_DEBUG_STALL")
    for k in range(2):
        st.acquire()[...] = x[:, k * fpc:(k + 1) * fpc]
        st.submit()
    for _ in range(2):
        with pytest.raises(sc.QpskError) as ei:
            st.retrieve_records()
        assert ei.value.code == sc.QPSK_ESTALL
    assert st.pending == 0   # the chunks count as retrieved either way
    st.close()


def test_example_packed_file(tmp_path):
    """examples/qpsk_rx_stream -p: one file of 16-byte records in time order ==
    the by-frame records of the same channel files through Python, for chunk
    sizes that do and do not divide the stream."""
    exe = os.path.join(ROOT, "examples", "qpsk_rx_stream")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.dirname(exe)], check=True)
    nch, nf = 5, 14
    x = sc.synth_device(45, nch, nf, 8.0).cpu().numpy()
    paths = []
    for i in range(nch):
        x[i].tofile(tmp_path / f"ch{i}.raw")
        paths.append(str(tmp_path / f"ch{i}.raw"))
    rx = sc.Receiver(nch)
    exp = rx.demod_records(x, order=sc.REC_BY_FRAME)
    rx.close()
    assert 0 < exp["count"]
    for fpc in (4, 7, 20):
        out = tmp_path / f"p{fpc}.rec"
        r = subprocess.run([exe, "-f", str(fpc), *paths, "-p", str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == exp["rec"].tobytes(), fpc
        assert not os.path.exists(f"{out}0.bin")   # no per-channel files
