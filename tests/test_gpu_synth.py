"""GPU synthesis of the benchmark input (qpsk_synth_device, singlecarrier_amd/
csrc/qpsk_synth_dev.hip) against the host generator qpsk_synth_batch(), whose
transmitter reproduces the reference's qpsk_tx_frame (src/qpsk.c:278-322)
bit for bit (tests/test_abi.py, tests/golden/tx_golden.npz).  The device
formulation is parallel over (channel, TX block) instead of stateful, so this
is a parity test of that reformulation: noiseless output must be identical,
sample for sample."""
import ctypes as C

import numpy as np
import pytest

import oracle
import rxcheck
import singlecarrier_amd as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.mark.parametrize("seed,nch,nf,c0", [(3, 300, 5, 0), (1, 64, 40, 0), (7, 130, 9, 4000),
                                            (11, 1, 2, 123456)])
def test_noiseless_identical_to_host(seed, nch, nf, c0):
    d = sc.synth_device(seed, nch, nf, c0=c0).cpu().numpy()
    h = sc.synth(seed, nch, nf, c0=c0)
    assert d.shape == h.shape
    bad = d != h
    assert not bad.any(), f"{int(bad.sum())} samples differ, first at {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("ebn0", [0.0, 4.0, 9.0])
def test_awgn_matches_host(ebn0):
    """Same counter-based Box-Muller; the double log/cos come from the device
    libm, so equality is checked, not assumed: every sample identical."""
    d = sc.synth_device(5, 128, 6, ebn0).cpu().numpy()
    h = sc.synth(5, 128, 6, ebn0)
    ndiff = int((d != h).sum())
    assert ndiff == 0, f"{ndiff} of {d.size} noisy samples differ (max |diff| " \
                       f"{int(np.abs(d.astype(int) - h).max())})"


def test_odd_lengths_and_tail():
    """nsamples that end inside a packet, in a gap and before the first sample."""
    for ns in (1, 700, 2783 + 1900, 3 * 2783 - 5):
        out = torch.empty((40, ns), dtype=torch.int16, device="cuda")
        assert sc.lib().qpsk_synth_device(9, 0, 40, 1000.0, out.data_ptr(), ns, None) == 0
        torch.cuda.synchronize()
        h = np.empty((40, ns), np.int16)
        sc.lib().qpsk_synth_batch(9, 0, 40, 1000.0, h.ctypes.data, ns, 4)
        assert (out.cpu().numpy() == h).all(), ns


def test_rx_on_device_synthesised_input():
    """The receive path fed straight from the device generator (no host copy of
    the input), checked against the oracle on the same samples."""
    nch, nf = 200, 12
    x = sc.synth_device(42, nch, nf, 6.0)
    bits = torch.empty((nch, nf, 62), dtype=torch.uint8, device="cuda")
    valid = torch.empty((nch, nf), dtype=torch.uint8, device="cuda")
    rx = sc.Receiver(nch)
    rx.demod_device(x, bits, valid)
    torch.cuda.synchronize()
    eb, ev, _ = oracle.cpu_rx(x.cpu().numpy())
    rxcheck.assert_same({"bits": bits.cpu().numpy(), "valid": valid.cpu().numpy()}, {"bits": eb, "valid": ev})
    assert ev.any()
    rx.close()


GOLDEN = ["synth_s1_clean", "synth_s2_eb8", "synth_s3_eb4", "synth_s4_eb0",
          "synth_d752_s1_clean", "synth_d752_s2_eb4"]


@pytest.mark.parametrize("name", GOLDEN)
def test_device_generator_reproduces_golden_inputs(golden_dir, name):
    """The GPU generator against the committed golden inputs: the input_sha256
    each golden set records (tests/golden/make_golden.py, made with the
    oracle's generator oracle/cpu_ref.c qc_synth, whose TX is the reference's
    qpsk_tx_frame, src/qpsk.c:278-322, checked by tests/test_oracle.py)."""
    import hashlib
    import os
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    d = sc.synth_device(int(g["seed"]), int(g["nch"]), int(g["nframes"]),
                        float(g["ebn0_db"])).cpu().numpy()
    assert hashlib.sha256(d.tobytes()).hexdigest() == str(g["input_sha256"])


@pytest.mark.parametrize("seed,nch,nf,ebn0,c0", [(3, 256, 32, 1000.0, 0), (3, 512, 16, 0.0, 65024),
                                                 (8, 97, 7, 5.0, 31), (9, 64, 3, 10.0, 1 << 20)])
def test_device_generator_equals_oracle(seed, nch, nf, ebn0, c0):
    """qpsk_synth_device against the oracle's generator (oracle.synth, the
    test-side restatement of the reference TX, src/qpsk.c:380-413), noiseless
    and AWGN, at channel offsets inside and beyond the C3 batch."""
    d = sc.synth_device(seed, nch, nf, ebn0, c0=c0).cpu().numpy()
    o = oracle.synth(seed, nch, nf, ebn0, c0=c0)
    nd = int((d != o).sum())
    assert nd == 0, f"{nd} of {d.size} samples differ"
