"""Random call traffic on the GPU (run with -m gpu): the seeded scripts of
tests/traffic.py through the lifecycle calls in orders nobody wrote down, every
output compared with the model's (the oracle on every channel's own stream from
its latest start; records, levels and the gate restated in numpy).
tests/test_traffic_model.py shows on the CPU what the scripts cover, observe and
catch.

A failure names the seed, the op index and the op; traffic.replay(script[:k + 1],
"rx", mode, seed) shows the same difference."""
import pytest

import rxcheck
import singlecarrier_amd as sc
import traffic

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEC = sc.MODE_DEC752
CONFIGS = [(shape, width, sc.MODE_REFERENCE) for shape, width in rxcheck.ALL_SHAPES] + \
          [(shape, width, mode) for mode in (DEC, DEC | sc.MODE_FFT_HUNT) for shape, width in (("4x2", None), ("1x8", "16"))]
IDS = [f"{s}-{w or 'auto'}-mode{m}" for s, w, m in CONFIGS]


@pytest.mark.parametrize("seed", traffic.RX_SEEDS)
@pytest.mark.parametrize("shape,width,mode", CONFIGS, ids=IDS)
def test_receive_scripts(shape, width, mode, seed, monkeypatch):
    """130 and 40 channels, at most 40 frames and 24 ops: frames and
    channel_frames after every op, every call's outputs, and at the end every
    range's snapshot against a plain receiver's, byte for byte."""
    rxcheck.force_shape(monkeypatch, shape, width)
    traffic.run_rx(traffic.gen_rx(seed), traffic.GpuRx, mode, seed)


@pytest.mark.parametrize("seed", traffic.TX_SEEDS)
def test_transmit_scripts(seed):
    """24 channels on contexts of gaps 0, 1 and 903, at most 30 slots: int16
    device, fused planar A-law and interleaved mu-law blocks against Restated,
    sample for sample; packets and channel_packets after every op."""
    traffic.run_tx(traffic.gen_tx(seed), traffic.GpuTx, seed)


@pytest.mark.parametrize("gap", [0, 903])
def test_the_exchange(gap):
    """A trunk whose calls come and go: the masked transmitter writes 32 channels
    of interleaved A-law into one device buffer, restarting a channel in front
    of each call; a receiver reads the same buffer through the squelched record
    call and restarts its channels at the same moments."""
    stats = traffic.run_exchange(traffic.EX_SEED, gap)
    print(gap, stats)
    assert stats["observed"] >= 40
