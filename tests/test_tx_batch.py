"""The batched transmitter's contract (include/qpsk_tx.h) on the host:
qpsk_tx_batch_host, the twin the GPU transmitter is compared with
(tests/test_gpu_tx.py), against the reference-made TX golden, the oracle's TX
restatement, the unmodified reference transmitter (when its build is present)
and the committed synthetic inputs.  Everything is exact equality of int16
samples.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import singlecarrier_amd as sc
from tx_geometry import golden_payload, packet_calls, with_gaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = sc.QPSK_EINVAL


def host_raw(st, nch, bits, npk, gap, out, ld, threads=2):
    return sc.lib().qpsk_tx_batch_host(sc._ptr(st) if st is not None else None, nch,
                                       sc._ptr(bits) if bits is not None else None, npk, gap,
                                       sc._ptr(out) if out is not None else None, ld, threads)


def test_golden_made_by_the_unmodified_reference(golden_dir):
    bits, samples = golden_payload(golden_dir)
    assert samples.shape == (5640,)
    got = sc.tx_batch_host(bits, gap=0)
    np.testing.assert_array_equal(got[0], samples)
    st = sc.tx_states(1)
    parts = [sc.tx_batch_host(bits[:, k:k + 1], gap=0, states=st)[0] for k in range(3)]
    np.testing.assert_array_equal(np.concatenate(parts), samples)


def test_against_the_oracle_and_the_reference():
    nch, npk, gap = 5, 2, 903
    bits = np.random.default_rng(20).integers(0, 2, (nch, npk, 8, 62), dtype=np.uint8)
    got = sc.tx_batch_host(bits, gap=gap)
    assert got.shape == (nch, npk * 2783)
    for c in range(nch):
        calls = packet_calls(bits[c])
        np.testing.assert_array_equal(got[c], with_gaps(oracle.cpu_tx(calls), gap))
        if oracle.ref_available():
            np.testing.assert_array_equal(got[c], with_gaps(oracle.ref_tx(calls), gap))
    g = got.reshape(nch, npk, 2783)
    assert not g[:, :, 1880:].any()
    assert g[:, :, :1880].any()


def test_a_long_stream_against_the_oracle_and_the_reference():
    """2,049 packets on one channel (3.85 M TX samples, the carrier renormalised
    thousands of times): the long-run pin under the GPU sweeps of
    tests/test_gpu_tx_sweep.py, which compare with this host twin alone"""
    npk = 2049
    bits = np.random.default_rng(2049).integers(0, 2, (1, npk, 8, 62), dtype=np.uint8)
    got = sc.tx_batch_host(bits, gap=0)
    assert got.shape == (1, npk * 1880)
    calls = packet_calls(bits[0])
    np.testing.assert_array_equal(got[0], np.concatenate(oracle.cpu_tx(calls)))
    if oracle.ref_available():
        np.testing.assert_array_equal(got[0], np.concatenate(oracle.ref_tx(calls)))
    # the gap moves samples and changes none
    gapped = sc.tx_batch_host(bits, gap=7).reshape(npk, 1887)
    np.testing.assert_array_equal(gapped[:, :1880].reshape(-1), got[0])
    assert not gapped[:, 1880:].any()
    # in 8 calls of uneven size on a carried state
    st = sc.tx_states(1)
    cuts = [0, 1, 2, 259, 260, 1024, 2000, 2048, 2049]
    parts = [sc.tx_batch_host(bits[:, lo:hi], gap=0, states=st)[0] for lo, hi in zip(cuts, cuts[1:])]
    np.testing.assert_array_equal(np.concatenate(parts), got[0])


def test_only_a_byte_equal_to_one_is_a_one():
    """qpsk_mod's `== 1` (src/qpsk.c:252-253): 0, 2 and 255 all map to +1."""
    bits = np.random.default_rng(21).choice(np.array([0, 1, 2, 255], np.uint8), (3, 2, 8, 62))
    assert set(np.unique(bits)) == {0, 1, 2, 255}
    np.testing.assert_array_equal(sc.tx_batch_host(bits, gap=7),
                                  sc.tx_batch_host((bits == 1).astype(np.uint8), gap=7))


M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def _draw(s0, n):
    """Draw n (1-based) of splitmix64 started at s0 (include/qpsk_synth.h)."""
    z = (s0 + n * GOLD) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def test_tie_to_the_committed_synthetic_inputs():
    """The generator's documented draws, regenerated here: dibit of data symbol
    d of packet k = draw 2 + 248 k + d of splitmix64(seed ^ c K), I = dibit >> 1,
    Q = dibit & 1, delay = draw 1 mod 2783.  The batched transmitter on that
    payload is the generator's stream from its delay onward."""
    seed, nch, nf = 1, 4, 8          # the seed of tests/golden/synth_s1_clean.npz
    ns = nf * 1880
    npk = ns // 2783 + 1
    x = sc.synth(seed, nch, nf).reshape(nch, ns)
    bits = np.zeros((nch, npk, 8, 62), np.uint8)
    delay = []
    for c in range(nch):
        s0 = seed ^ ((c * GOLD) & M64)
        delay.append(_draw(s0, 1) % 2783)
        for k in range(npk):
            for d in range(248):
                dib = _draw(s0, 2 + 248 * k + d) & 3
                bits[c, k, d // 31, 2 * (d % 31) + 1] = dib >> 1
                bits[c, k, d // 31, 2 * (d % 31)] = dib & 1
    tx = sc.tx_batch_host(bits, gap=903)
    for c in range(nch):
        n = ns - delay[c]
        assert 0 < n <= tx.shape[1]
        assert not x[c, :delay[c]].any()
        np.testing.assert_array_equal(tx[c, :n], x[c, delay[c]:])


def test_layout_tail_survives_and_odd_ld():
    nch, npk, gap = 3, 2, 903
    need = npk * 2783
    bits = np.random.default_rng(22).integers(0, 2, (nch, npk, 8, 62), dtype=np.uint8)
    ref = sc.tx_batch_host(bits, gap=gap)
    for ld in (need + 13, need + 1):      # need is even: both are odd
        out = np.full((nch, ld), 0x5A5A, np.int16)
        assert host_raw(sc.tx_states(nch), nch, bits, npk, gap, out, ld) == 0
        np.testing.assert_array_equal(out[:, :need], ref)
        assert (out[:, need:] == 0x5A5A).all()


def test_arguments():
    L = sc.lib()
    nch, npk, gap = 2, 2, 5
    need = npk * 1885
    bits = np.zeros((nch, npk, 8, 62), np.uint8)
    out = np.full((nch, need), 0x5A5A, np.int16)
    st = sc.tx_states(nch)
    assert host_raw(st, nch, bits, -1, gap, out, need) == EINVAL          # npackets < 0
    assert host_raw(st, nch, bits, npk, gap, out, need - 1) == EINVAL     # ld too small
    assert host_raw(st, nch, None, npk, gap, out, need) == EINVAL         # NULL bits
    assert host_raw(st, nch, bits, npk, gap, None, need) == EINVAL        # NULL out
    assert host_raw(st, nch, bits, npk, -1, out, need) == EINVAL          # gap < 0
    assert host_raw(st, 0, bits, npk, gap, out, need) == EINVAL           # nch < 1
    assert host_raw(None, nch, bits, npk, gap, out, need) == EINVAL       # NULL states
    # nch * npackets >= 2^28 is refused before anything is read or written
    assert host_raw(st, 2, bits, 1 << 27, gap, out, (1 << 27) * 1885) == EINVAL
    assert (out == 0x5A5A).all()
    st0 = st.copy()
    assert host_raw(st, nch, None, 0, gap, None, 0) == 0                  # npackets == 0: no-op
    assert host_raw(st, nch, bits, 0, gap, out, need) == 0
    assert (out == 0x5A5A).all() and (st == st0).all()
    # the device entry points refuse a NULL context the same way, without a GPU
    assert L.qpsk_tx_batch(None, sc._ptr(bits), npk, sc._ptr(out), need) == EINVAL
    assert L.qpsk_tx_batch_device(None, sc._ptr(bits), npk, sc._ptr(out), need, None) == EINVAL
    for a, g in ((0, 903), (4, -1), (-3, 0)):
        err = C.c_int(0)
        assert not L.qpsk_tx_create(0, a, g, C.byref(err))
        assert err.value == EINVAL
    assert not L.qpsk_tx_create(0, 0, 903, None)                          # err may be NULL


def test_no_gpu_is_a_loud_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(sc.QpskError):
        sc.Transmitter(4)


def test_example_builds(golden_dir, tmp_path):
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "qpsk_tx_raw"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = os.path.join(ROOT, "examples", "qpsk_tx_raw")
    assert os.path.exists(exe)
    # its host path (-c) on the golden payload writes the reference's samples,
    # one channel and two files batched as channels
    bits, samples = golden_payload(golden_dir)
    (tmp_path / "a.bits").write_bytes(bits.tobytes() + b"\x01" * 100)    # a short tail is dropped
    r = subprocess.run([exe, "-c", "-g", "0", str(tmp_path / "a.bits"), str(tmp_path / "a.raw")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(np.fromfile(tmp_path / "a.raw", "<i2"), samples)
    r = subprocess.run([exe, "-b", "-c", "-g", "903", str(tmp_path / "a.bits"), str(tmp_path / "a.bits"),
                        "-o", str(tmp_path / "ch")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = sc.tx_batch_host(bits, gap=903)[0]
    for c in range(2):
        np.testing.assert_array_equal(np.fromfile(tmp_path / f"ch{c}.raw", "<i2"), want)
