"""The batched GPU transmitter (include/qpsk_tx.h, singlecarrier_amd/csrc/
qpsk_tx.hip) against its host twin qpsk_tx_batch_host (pinned to the reference
by tests/test_tx_batch.py), the reference-made TX golden and the oracle's TX
restatement.  Everything is exact equality of int16 samples."""
import numpy as np
import pytest

import oracle
import rxcheck
import singlecarrier_amd as sc
from tx_geometry import golden_payload, packet_calls, with_gaps

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT = 0x5A5A
# tx_batch_kernel loops over 16 channels of one of 8 alignment classes, so one
# block row covers 128 channels; 150 exceeds that and is no multiple of it
NCH_PAST_GROUP = 150


def payload(seed, nch, npk):
    return np.random.default_rng(seed).integers(0, 2, (nch, npk, 8, 62), dtype=np.uint8)


def device_run(tx, bits, ld=None, offset=0, splits=None):
    """bits through modulate_device into a sentinel-filled buffer whose rows
    start `offset` int16 past a 16-byte boundary and are `ld` apart; `splits`
    sends the packets in that many calls.  Returns (rows [nch][need], the whole
    buffer, the mask of samples the calls were to write)."""
    nch, npk = bits.shape[:2]
    P = 1880 + tx.gap
    need = npk * P
    ld = need if ld is None else ld
    pad = 64
    total = pad + offset + nch * ld + pad
    buf = torch.full((total + 8,), SENT, dtype=torch.int16, device="cuda")
    base = (-(buf.data_ptr() // 2)) % 8          # first 16-byte-aligned element
    buf = buf[base:base + total]
    assert buf.data_ptr() % 16 == 0
    rows = buf[pad + offset:pad + offset + nch * ld].as_strided((nch, need), (ld, 1))
    d_bits = torch.from_numpy(bits).cuda()
    k = 0
    for n in (splits or [npk]):
        tx.modulate_device(d_bits[:, k:k + n].contiguous(), rows[:, k * P:], None)
        k += n
    assert k == npk
    tx.sync()
    whole = buf.cpu().numpy()
    mask = np.zeros(total, bool)
    for c in range(nch):
        mask[pad + offset + c * ld:pad + offset + c * ld + need] = True
    return rows.cpu().numpy(), whole, mask


def test_golden(golden_dir):
    bits, samples = golden_payload(golden_dir)
    tx = sc.Transmitter(1, gap=0)
    np.testing.assert_array_equal(tx.modulate(bits)[0], samples)
    tx.close()
    tx = sc.Transmitter(2, gap=0)
    out = tx.modulate(np.concatenate([bits, bits]))
    np.testing.assert_array_equal(out[0], samples)
    np.testing.assert_array_equal(out[1], samples)
    tx.close()


@pytest.mark.parametrize("gap", [0, 1, 7, 903])
@pytest.mark.parametrize("nch", [1, 3, 67, NCH_PAST_GROUP])
def test_device_equals_host_twin_and_oracle(nch, gap):
    npk = 5
    bits = payload(100 + nch + gap, nch, npk)
    host = sc.tx_batch_host(bits, gap=gap)
    tx = sc.Transmitter(nch, gap=gap)
    one, _, _ = device_run(tx, bits)
    assert tx.packets() == npk
    np.testing.assert_array_equal(one, host)
    tx.reset()
    parts, _, _ = device_run(tx, bits, splits=[1, 3, 1])
    np.testing.assert_array_equal(parts, host)
    tx.close()
    if gap == 903 and nch == 3:
        for c in range(nch):
            want = with_gaps(oracle.cpu_tx(packet_calls(bits[c])), gap)
            np.testing.assert_array_equal(one[c], want)
            np.testing.assert_array_equal(parts[c], want)


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("extra", [0, 1, 13])
def test_alignment_and_sentinels(offset, extra):
    nch, npk, gap = 11, 3, 903
    bits = payload(7, nch, npk)
    host = sc.tx_batch_host(bits, gap=gap)
    tx = sc.Transmitter(nch, gap=gap)
    aligned, _, _ = device_run(tx, bits)
    np.testing.assert_array_equal(aligned, host)
    tx.reset()
    got, whole, mask = device_run(tx, bits, ld=npk * (1880 + gap) + extra, offset=offset)
    np.testing.assert_array_equal(got, aligned)
    # before the first row, the row tails, after the last row
    assert (whole[~mask] == SENT).all()
    tx.close()


def test_byte_values_reset_and_packets():
    nch, gap = 5, 7
    bits = np.random.default_rng(21).choice(np.array([0, 1, 2, 255], np.uint8), (nch, 2, 8, 62))
    tx = sc.Transmitter(nch, gap=gap)
    assert tx.packets() == 0
    a = tx.modulate(bits)
    np.testing.assert_array_equal(a, sc.tx_batch_host((bits == 1).astype(np.uint8), gap=gap))
    assert tx.packets() == 2
    b = tx.modulate(bits)            # continues the stream: filter memory and carrier carried
    assert tx.packets() == 4
    np.testing.assert_array_equal(np.concatenate([a, b], axis=1),
                                  sc.tx_batch_host(np.concatenate([bits, bits], axis=1), gap=gap))
    assert (a != b).any()
    tx.reset()
    assert tx.packets() == 0
    np.testing.assert_array_equal(tx.modulate(bits), a)
    assert tx.modulate(bits[:, :0]).shape == (nch, 0) and tx.packets() == 2   # npackets == 0
    tx.close()


def test_transmit_into_receive_on_the_device():
    """No host copy between the two: the transmitter's output buffer, viewed as
    frames, is the receiver's input."""
    nch, npk, gap, nf = 8, 8, 903, 12
    bits = payload(30, nch, npk)
    x = np.zeros((nch, nf * 1880), np.int16)
    x[:, :npk * 2783] = sc.tx_batch_host(bits, gap=gap)
    eb, ev, _ = oracle.cpu_rx(x.reshape(nch, nf, 1880))
    assert ev.any()                  # seed 30: 27 valid frames
    out = torch.zeros((nch, nf * 1880), dtype=torch.int16, device="cuda")
    assert out.stride(0) == 22560
    tx = sc.Transmitter(nch, gap=gap)
    rx = sc.Receiver(nch)
    d_bits = torch.empty((nch, nf, 62), dtype=torch.uint8, device="cuda")
    d_valid = torch.empty((nch, nf), dtype=torch.uint8, device="cuda")
    tx.modulate_device(torch.from_numpy(bits).cuda(), out)
    rx.demod_device(out.view(nch, nf, 1880), d_bits, d_valid)
    torch.cuda.synchronize()
    rx.sync()
    np.testing.assert_array_equal(out.cpu().numpy(), x)
    rxcheck.assert_same({"bits": d_bits.cpu().numpy(), "valid": d_valid.cpu().numpy()}, {"bits": eb, "valid": ev})
    tx.close()
    rx.close()


def test_two_contexts_on_two_streams():
    nch, gap = 9, 903
    ba, bb = payload(41, nch, 4), payload(42, nch, 4)
    ta, tb = sc.Transmitter(nch, gap=gap), sc.Transmitter(nch, gap=gap)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da, db = torch.from_numpy(ba).cuda(), torch.from_numpy(bb).cuda()
    oa = torch.zeros((nch, 4 * 2783), dtype=torch.int16, device="cuda")
    ob = torch.zeros((nch, 4 * 2783), dtype=torch.int16, device="cuda")
    cuts = [(0, 1), (1, 3), (3, 4)]
    pa = [da[:, lo:hi].contiguous() for lo, hi in cuts]   # made before the streams read them
    pb = [db[:, lo:hi].contiguous() for lo, hi in cuts]
    torch.cuda.synchronize()
    for (lo, _), xa, xb in zip(cuts, pa, pb):   # interleaved calls, each context on its own stream
        ta.modulate_device(xa, oa[:, lo * 2783:], sa)
        tb.modulate_device(xb, ob[:, lo * 2783:], sb)
    ta.sync()
    tb.sync()
    for t, b, o in ((ta, ba, oa), (tb, bb, ob)):
        single = sc.Transmitter(nch, gap=gap)
        np.testing.assert_array_equal(o.cpu().numpy(), single.modulate(b))
        np.testing.assert_array_equal(o.cpu().numpy(), sc.tx_batch_host(b, gap=gap))
        single.close()
        t.close()
