"""Transmitter channels that come and go (include/qpsk_tx.h), the part that
needs no GPU: the carrier's period the per-channel index rests on, the host
twin qpsk_tx_batch_masked_host against an independent restatement
(tests/tx_mask_cases.py: the plain host transmitter on each channel's active
packets alone), and the argument checks that run before any HIP call.
Everything is exact equality."""
import os
import subprocess

import numpy as np
import pytest

import singlecarrier_amd as sc
import tx_mask_geometry as mg
from tx_geometry import golden_payload
from tx_mask_cases import HEADER, PACKET, Restated, Twin, masks, payload, snapshot

EINVAL = sc.QPSK_EINVAL


def test_the_carrier_is_periodic_from_packet_8_on():
    """qpsk_tx_phase_table over 72 packets: packet p + 1 is packet p negated,
    bit for bit, for every p >= 8, and the transient really ends at 8.  The
    9-row carrier table of a general context (row min(p, 8), negated for odd
    p > 8) is exact because of this and of nothing else."""
    npk = 72
    t = sc.tx_phase_table(npk * PACKET).reshape(npk, PACKET, 2)
    u = t.view(np.uint32)
    neg = (-t).view(np.uint32)
    for p in range(8, npk - 1):
        assert (u[p + 1] == neg[p]).all(), f"packet {p + 1} is not packet {p} negated"
    assert (u[8] != neg[7]).any(), "the transient ends before packet 8"
    # hence own index p rides row min(p, 8), negated when p > 8 and p is odd
    for p in range(npk):
        row = t[min(p, 8)]
        np.testing.assert_array_equal(u[p], (-row if p > 8 and p % 2 else row).view(np.uint32))
    assert np.isfinite(t).all()


@pytest.mark.parametrize("gap", [903, 0, 5])
def test_masked_host_against_the_restatement(gap):
    """Random masks with the rows the header's cases name (a channel idle
    throughout, a first packet in a later slot, a last active slot that is not
    the last, a long idle run, idle first and last slots), over three calls so
    that the state carried over an idle tail is used."""
    nch = 11
    twin, rest = Twin(nch), Restated(nch)
    for call, npk in enumerate((12, 5, 7)):
        bits, m = payload(100 + call, nch, npk), masks(200 + call, nch, npk)
        got = twin.call(bits, gap, m)
        np.testing.assert_array_equal(got, rest.call(bits, gap, m != 0))
        g = got.reshape(nch, npk, PACKET + gap)
        assert not g[m == 0].any() and not g[:, :, PACKET:].any()
        assert g[m != 0][:, :PACKET].any(axis=1).all()
    np.testing.assert_array_equal(twin.st, rest.st)


@pytest.mark.parametrize("gap", [903, 0])
@pytest.mark.parametrize("kind", ["sweep", "joins"])
def test_masked_host_against_the_restatement_on_the_sweep_masks(kind, gap):
    """The masks of tests/test_gpu_tx_mask_sweep.py, where the twin is the
    yardstick, cut down to two calls of their first slots: 136 channels x 40
    slots of the de Bruijn mask hold every 4-slot window in every channel, and
    the first 80 slots of the join mask several channels' first packets, later
    than slot 0, while others stay idle throughout.  The second call starts
    from the state the first left, in the sweep mask behind idle tails of up
    to 4 slots."""
    if kind == "sweep":
        nch, npk = mg.SWEEP_NCH, 40
        mask = mg.sweep_mask(nch, 2 * npk, 300 + gap)
        win = mg.windows(mask[:, :npk])[:, 1:npk - 2]
        assert all(set(row.tolist()) == set(range(16)) for row in win)
        tails = npk - 1 - np.array([np.flatnonzero(r)[-1] for r in mask[:, :npk]])
        assert (tails > 0).sum() >= 8 and tails.max() == 4    # B's longest run of zeros
    else:
        npk = 80
        mask = mg.join_case(gap).mask[:, :2 * npk]
        nch = mask.shape[0]
        first = np.array([np.flatnonzero(r)[0] if r.any() else -1 for r in mask])
        assert ((0 < first) & (first < npk)).sum() >= 3 and (first >= npk).sum() >= 3
        assert (first < 0).sum() >= 3                         # and channels that do not join in these slots
    twin, rest = Twin(nch), Restated(nch)
    for call in range(2):
        bits, m = payload(310 + call, nch, npk), mask[:, npk * call:npk * call + npk]
        got = twin.call(bits, gap, m)
        np.testing.assert_array_equal(got, rest.call(bits, gap, m != 0))
        g = got.reshape(nch, npk, PACKET + gap)
        assert not g[m == 0].any() and g[m != 0][:, :PACKET].any(axis=1).all()
    np.testing.assert_array_equal(twin.st, rest.st)


def test_an_idle_slot_reads_no_bits_and_moves_no_state():
    nch, npk, gap = 3, 4, 5
    bits = payload(1, nch, npk)
    st = sc.tx_states(nch)
    sc.tx_batch_host(bits, gap=gap, states=st)          # some history and phase to keep
    st0 = st.copy()
    out = sc.tx_batch_host(bits, gap=gap, states=st, active=np.zeros((nch, npk), np.uint8))
    assert out.shape == (nch, npk * (PACKET + gap)) and not out.any()
    assert st.tobytes() == st0.tobytes()
    # the bits row of an idle slot is not read: any bytes there give the same samples
    m = np.array([[1, 0, 1, 0], [0, 0, 0, 1], [1, 1, 0, 1]], np.uint8)
    other = bits.copy()
    other[m == 0] = 1 - other[m == 0]
    a = sc.tx_batch_host(bits, gap=gap, states=st0.copy(), active=m)
    b = sc.tx_batch_host(other, gap=gap, states=st0.copy(), active=m)
    np.testing.assert_array_equal(a, b)


def test_idle_first_and_last_slots():
    nch, npk, gap = 2, 6, 903
    bits = payload(2, nch, npk)
    m = np.ones((nch, npk), np.uint8)
    m[0, 0] = m[1, npk - 1] = 0
    got = sc.tx_batch_host(bits, gap=gap, active=m).reshape(nch, npk, PACKET + gap)
    np.testing.assert_array_equal(got[0, 1:], sc.tx_batch_host(bits[:1, 1:], gap=gap).reshape(npk - 1, -1))
    np.testing.assert_array_equal(got[1, :-1], sc.tx_batch_host(bits[1:, :-1], gap=gap).reshape(npk - 1, -1))
    assert not got[0, 0].any() and not got[1, -1].any()


def test_splits_1_3_1_equal_5():
    nch, gap = 9, 0
    bits, m = payload(3, nch, 5), masks(4, nch, 5)
    whole = sc.tx_batch_host(bits, gap=gap, active=m)
    twin = Twin(nch)
    parts = [twin.call(bits[:, lo:hi], gap, m[:, lo:hi]) for lo, hi in ((0, 1), (1, 4), (4, 5))]
    np.testing.assert_array_equal(np.concatenate(parts, axis=1), whole)


def test_an_all_ones_mask_is_the_plain_call():
    nch, npk, gap = 4, 3, 7
    bits = payload(5, nch, npk)
    sa, sb, sn = sc.tx_states(nch), sc.tx_states(nch), sc.tx_states(nch)
    plain = sc.tx_batch_host(bits, gap=gap, states=sa)
    np.testing.assert_array_equal(sc.tx_batch_host(bits, gap=gap, states=sb, active=np.full((nch, npk), 0xFF, np.uint8)),
                                  plain)
    np.testing.assert_array_equal(sc.tx_batch_host(bits, gap=gap, states=sn, active=None), plain)
    assert sa.tobytes() == sb.tobytes() == sn.tobytes()


def test_the_golden_stream_with_idle_slots_inserted(golden_dir):
    """tx_golden.npz, three packets the unmodified reference made, sent in
    slots 1, 4 and 5 of 7: the golden's samples, packet by packet, with runs
    of zeros between them."""
    bits, samples = golden_payload(golden_dir)
    gap, slots = 11, (1, 4, 5)
    wide = payload(6, 1, 7)
    wide[0, slots] = bits[0]
    m = np.zeros((1, 7), np.uint8)
    m[0, slots] = 1
    got = sc.tx_batch_host(wide, gap=gap, active=m).reshape(7, PACKET + gap)
    np.testing.assert_array_equal(got[slots, :PACKET].reshape(-1), samples)
    got[slots, :PACKET] = 0
    assert not got.any()


def _masked_host_raw(st, nch, bits, active, npk, gap, out, ld):
    p = lambda a: sc._ptr(a) if a is not None else None
    return sc.lib().qpsk_tx_batch_masked_host(p(st), nch, p(bits), p(active), npk, gap, p(out), ld, 2)


def test_masked_host_arguments_and_write_set():
    nch, npk, gap = 2, 2, 5
    need = npk * (PACKET + gap)
    bits, m = payload(7, nch, npk), np.array([[1, 0], [0, 1]], np.uint8)
    out = np.full((nch, need + 3), 0x5A5A, np.int16)
    st = sc.tx_states(nch)
    for args in ((st, nch, bits, m, -1, gap, out, need), (st, nch, bits, m, npk, gap, out, need - 1),
                 (st, nch, None, m, npk, gap, out, need), (st, nch, bits, m, npk, gap, None, need),
                 (st, nch, bits, m, npk, -1, out, need), (st, 0, bits, m, npk, gap, out, need),
                 (None, nch, bits, m, npk, gap, out, need), (st, 2, bits, m, 1 << 27, gap, out, (1 << 27) * (PACKET + gap))):
        assert _masked_host_raw(*args) == EINVAL
    assert (out == 0x5A5A).all() and st.tobytes() == sc.tx_states(nch).tobytes()
    assert _masked_host_raw(st, nch, None, None, 0, gap, None, 0) == 0      # npackets == 0: no-op
    assert _masked_host_raw(st, nch, bits, m, npk, gap, out, need + 3) == 0
    np.testing.assert_array_equal(out[:, :need], sc.tx_batch_host(bits, gap=gap, active=m))
    assert (out[:, need:] == 0x5A5A).all()                                   # exactly npackets * P per row


def test_snapshot_size():
    L = sc.lib()
    assert HEADER == 16
    for n in (1, 2, 30, 65536, (1 << 28) - 1):
        assert L.qpsk_tx_state_size(n) == 16 + 12 * n
    for n in (0, -1, -(1 << 31)):
        assert L.qpsk_tx_state_size(n) == 0
    assert len(snapshot([3, 0], [0x01ff01ff, 0])) == L.qpsk_tx_state_size(2)


def test_the_new_calls_refuse_a_null_context_without_a_gpu():
    """The checks that run before any HIP call, as far as they can be reached
    without a context (tests/test_gpu_tx_mask.py refuses short, foreign and
    wrong-version snapshots on a real one)."""
    L = sc.lib()
    bits, m = payload(8, 1, 1), np.ones((1, 1), np.uint8)
    out = np.zeros((1, PACKET), np.int16)
    snap = np.frombuffer(snapshot([0], [0]), np.uint8).copy()
    idx = np.zeros(1, np.uint64)
    p = sc._ptr
    assert L.qpsk_tx_batch_masked(None, p(bits), p(m), 1, p(out), PACKET) == EINVAL
    assert L.qpsk_tx_batch_masked_device(None, p(bits), p(m), 1, p(out), PACKET, None) == EINVAL
    assert L.qpsk_tx_batch_masked_fmt(None, p(bits), p(m), 1, p(out), sc.OUT_ALAW, PACKET) == EINVAL
    assert L.qpsk_tx_batch_masked_device_fmt(None, p(bits), p(m), 1, p(out), sc.OUT_ALAW, PACKET, None) == EINVAL
    assert L.qpsk_tx_reset_channels(None, 0, 1) == EINVAL
    assert L.qpsk_tx_channel_packets(None, 0, 1, p(idx)) == EINVAL
    assert L.qpsk_tx_state_save(None, 0, 1, p(snap), snap.size) == EINVAL
    assert L.qpsk_tx_state_load(None, 0, 1, p(snap), snap.size) == EINVAL


def test_example_sends_every_file_to_its_own_end(tmp_path):
    """examples/qpsk_tx_raw -b -a on the host path: files of 3, 1 and 2 packets
    give three lines of 3 slots, a line idle once its file has ended; without
    -a the batch still stops at the shortest file."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["make", "-s", "-C", os.path.join(root, "examples"), "qpsk_tx_raw"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe, gap, have = os.path.join(root, "examples", "qpsk_tx_raw"), 7, (3, 1, 2)
    bits = payload(10, 3, 3)
    files = []
    for c, n in enumerate(have):
        files.append(str(tmp_path / f"in{c}.bits"))
        (tmp_path / f"in{c}.bits").write_bytes(bits[c, :n].tobytes())
    m = np.array([[k < n for k in range(3)] for n in have], np.uint8)
    want = sc.tx_batch_host(bits, gap=gap, active=m)
    for flags, rows in ((["-a"], want), ([], sc.tx_batch_host(bits[:, :1], gap=gap))):
        r = subprocess.run([exe, "-b", *flags, "-c", "-g", str(gap), *files, "-o", str(tmp_path / "ch")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for c in range(3):
            np.testing.assert_array_equal(np.fromfile(tmp_path / f"ch{c}.raw", "<i2"), rows[c])
    assert not want[1, PACKET + gap:].any() and want[1, :PACKET].any()


def test_python_mirror_checks_the_mask_shape():
    bits = payload(9, 2, 3)
    with pytest.raises(ValueError):
        sc.tx_batch_host(bits, active=np.ones((2, 4), np.uint8))
    with pytest.raises(ValueError):
        sc.tx_batch_host(bits, active=np.ones((3, 3), np.uint8))
    # any dtype: nonzero is active (256 is not 0)
    a = sc.tx_batch_host(bits, gap=0, active=np.array([[256, 0, -1], [0, 0, 7]], np.int64))
    b = sc.tx_batch_host(bits, gap=0, active=np.array([[True, False, True], [False, False, True]]))
    np.testing.assert_array_equal(a, b)
