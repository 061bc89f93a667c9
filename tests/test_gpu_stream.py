"""Streaming ingest (include/qpsk_stream.h): chunks pushed through pinned slots
and three HIP streams give exactly the outputs of one batched call over the
concatenated frames -- and so the reference's, via the oracle."""
import numpy as np
import pytest

import oracle
import rxcheck
import singlecarrier_amd as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nslot", [1, 2, 3])
def test_stream_equals_one_batch(nslot):
    nch, fpc, nchunk = 150, 4, 5
    x = oracle.synth(17, nch, fpc * nchunk, 7.0)
    eb, ev, _ = oracle.cpu_rx(x)
    st = sc.Stream(nch, fpc, nslot=nslot)
    got_b, got_v = [], []
    for k in range(nchunk):
        buf = st.acquire()
        buf[...] = x[:, k * fpc:(k + 1) * fpc]
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
                        {"bits": eb, "valid": ev})
    assert ev.any()


def test_stream_reports_a_stalled_chunk(monkeypatch):
    """A progress wait that runs out in a chunk's receive must come back from
    qpsk_stream_retrieve() as QPSK_ESTALL for THAT chunk, never as bits with
    QPSK_OK.  QPSK_DEBUG_STALL (read at creation) makes one wait of every call
    unending on 96 channels (a dual-chain shape); the timeout is sticky per
    workgroup, so the call ends after one bound.  A stream made without the
    knob delivers the oracle's bits."""
    nch, fpc = 96, 3
    x = oracle.synth(18, nch, 2 * fpc, 6.0)
    monkeypatch.setenv("QPSK_DEBUG_STALL", "1")
    st = sc.Stream(nch, fpc, nslot=2)
    monkeypatch.delenv("QPSK_DEBUG_STALL")
    for k in range(2):
        st.acquire()[...] = x[:, k * fpc:(k + 1) * fpc]
        st.submit()
    for _ in range(2):
        with pytest.raises(sc.QpskError) as ei:
            st.retrieve()
        assert ei.value.code == sc.QPSK_ESTALL
    assert st.pending == 0
    st.close()
    st = sc.Stream(nch, fpc, nslot=2)
    got = []
    for k in range(2):
        st.acquire()[...] = x[:, k * fpc:(k + 1) * fpc]
        st.submit()
    while st.pending:
        got.append(st.retrieve()[0])
    st.close()
    assert (np.concatenate(got, axis=1) == oracle.cpu_rx(x)[0]).all()


def test_stream_stall_is_sticky_until_reset(monkeypatch):
    """A stall in the FIRST chunk only (QPSK_DEBUG_STALL=first) leaves every
    channel's carried state undefined: the clean chunks after it must come
    back QPSK_ESTALL too, the stream context's qpsk_rx_sync() must see the
    stall, and after qpsk_rx_reset() the stream must deliver the oracle's bits
    again."""
    nch, fpc = 96, 3
    x = oracle.synth(18, nch, 2 * fpc, 6.0)
    monkeypatch.setenv("QPSK_DEBUG_STALL", "first")
    st = sc.Stream(nch, fpc, nslot=3)
    monkeypatch.delenv("QPSK_DEBUG_STALL")
    for k in range(3):
        st.acquire()[...] = x[:, (k % 2) * fpc:(k % 2 + 1) * fpc]
        st.submit()
    for _ in range(3):
        with pytest.raises(sc.QpskError) as ei:
            st.retrieve()
        assert ei.value.code == sc.QPSK_ESTALL
    ctx = sc.lib().qpsk_stream_ctx(st._h)
    assert sc.lib().qpsk_rx_sync(ctx) == sc.QPSK_ESTALL
    assert sc.lib().qpsk_rx_reset(ctx) == 0
    assert sc.lib().qpsk_rx_sync(ctx) == 0
    got = []
    for k in range(2):
        st.acquire()[...] = x[:, k * fpc:(k + 1) * fpc]
        st.submit()
    while st.pending:
        got.append(st.retrieve()[0])
    st.close()
    assert (np.concatenate(got, axis=1) == oracle.cpu_rx(x)[0]).all()


def test_stream_reset_with_chunks_pending(monkeypatch):
    """qpsk_rx_reset() on a stream's context while chunks are in flight is
    refused (QPSK_EBUSY, include/qpsk_batch.h), and so are state snapshots:
    the chunks run on the state a reset would clear.  Three chunks, a stall in
    the first (QPSK_DEBUG_STALL=first): reset before retrieving -> EBUSY; every
    pre-reset chunk, the stalled one and the two that ran on its state, comes
    back QPSK_ESTALL (its epoch is taken at submit); after the drain the reset
    succeeds and the next chunks are the oracle's bits (VERDICT round 4,
    item 3)."""
    nch, fpc = 96, 3
    x = oracle.synth(19, nch, 2 * fpc, 6.0)
    monkeypatch.setenv("QPSK_DEBUG_STALL", "first")
    st = sc.Stream(nch, fpc, nslot=3)
    monkeypatch.delenv("QPSK_DEBUG_STALL")
    for k in range(3):
        st.acquire()[...] = x[:, (k % 2) * fpc:(k % 2 + 1) * fpc]
        st.submit()
    L = sc.lib()
    ctx = L.qpsk_stream_ctx(st._h)
    assert L.qpsk_rx_reset(ctx) == sc.QPSK_EBUSY
    snap = np.zeros(L.qpsk_rx_state_size(nch), np.uint8)
    assert L.qpsk_rx_state_save(ctx, 0, nch, snap.ctypes.data, snap.size) == sc.QPSK_EBUSY
    assert st.pending == 3
    with pytest.raises(sc.QpskError) as ei:
        st.retrieve()
    assert ei.value.code == sc.QPSK_ESTALL
    assert L.qpsk_rx_reset(ctx) == sc.QPSK_EBUSY     # two still pending
    for _ in range(2):
        with pytest.raises(sc.QpskError) as ei:
            st.retrieve()
        assert ei.value.code == sc.QPSK_ESTALL
    assert L.qpsk_rx_reset(ctx) == 0
    assert L.qpsk_rx_sync(ctx) == 0
    got = []
    for k in range(2):
        st.acquire()[...] = x[:, k * fpc:(k + 1) * fpc]
        st.submit()
    while st.pending:
        got.append(st.retrieve()[0])
    st.close()
    assert (np.concatenate(got, axis=1) == oracle.cpu_rx(x)[0]).all()


def test_stream_busy_and_misuse():
    st = sc.Stream(64, 2, nslot=2)
    for _ in range(2):
        st.acquire()
        st.submit()
    with pytest.raises(sc.QpskError):   # both slots in flight
        st.acquire()
    st.retrieve()
    st.acquire()                          # a slot is free again
    a = st.acquire()                      # acquiring again returns the same buffer
    assert a.shape == (64, 2, 1880)
    st.submit()
    st.retrieve()
    st.retrieve()
    with pytest.raises(sc.QpskError):   # nothing left to retrieve
        st.retrieve()
    with pytest.raises(sc.QpskError):   # submit without acquire
        st.submit()
    st.close()


def test_c_stream_driver(golden_dir, tmp_path):
    """examples/qpsk_rx_stream.c: .raw channel files read chunk by chunk into
    pinned stream slots; per-channel record files equal the reference's
    (sample file md5) and the oracle's, for chunk sizes that do and do not
    divide the stream."""
    import hashlib
    import json
    import os
    import subprocess
    exe = os.path.abspath(os.path.join(golden_dir, "..", "..", "examples", "qpsk_rx_stream"))
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.dirname(exe)], check=True)
    exp = json.load(open(os.path.join(golden_dir, "sample_expected.json")))
    paths = [os.path.join(golden_dir, "preamble_qpsk_8k.raw")]
    syn = oracle.synth(98, 3, 14, 6.0)
    for i in range(3):
        p = tmp_path / f"syn{i}.raw"
        syn[i].tofile(p)
        paths.append(str(p))
    bits, valid, _ = oracle.cpu_rx(syn)
    for fpc in (4, 7, 20):
        pre = tmp_path / f"f{fpc}_"
        subprocess.run([exe, "-f", str(fpc), *paths, "-o", str(pre)], check=True)
        got0 = open(f"{pre}0.bin", "rb").read()
        assert hashlib.md5(got0).hexdigest() == exp["output_md5"], fpc
        for i in range(3):
            assert open(f"{pre}{i + 1}.bin", "rb").read() == sc.records(bits[i], valid[i]), (fpc, i)


@pytest.mark.parametrize("mode", [1, 3])
def test_stream_in_variant_modes(mode):
    """qpsk_stream_create_mode: the dec752 / FFT-hunt receivers behind the
    streaming pipeline equal the oracle's same mode over the whole stream."""
    nch, fpc, nchunk = 96, 3, 4
    x = oracle.synth(18, nch, fpc * nchunk, 5.0)
    eb, ev, _ = oracle.cpu_rx(x, mode=mode)
    st = sc.Stream(nch, fpc, nslot=2, mode=mode)
    got_b, got_v = [], []
    for k in range(nchunk):
        if st.pending == 2:
            b, v = st.retrieve()
            got_b.append(b)
            got_v.append(v)
        buf = st.acquire()
        buf[...] = x[:, k * fpc:(k + 1) * fpc]
        st.submit()
    while st.pending:
        b, v = st.retrieve()
        got_b.append(b)
        got_v.append(v)
    st.close()
    rxcheck.assert_same({"bits": np.concatenate(got_b, axis=1), "valid": np.concatenate(got_v, axis=1)},
                        {"bits": eb, "valid": ev})
