"""bench.py --dump-outputs on CPU: the channel sample is fixed by the shape
alone, the files stay inside the 64 MB budget at the flagship shape, and
dump_outputs() writes float arrays that equal the tensors it was given."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_channels_fixed_sorted_within_budget():
    a = bench.dump_channels(65536, 32)
    assert (a == bench.dump_channels(65536, 32)).all()
    assert a.dtype == np.int64 and (np.diff(a) > 0).all() and 0 <= a[0] and a[-1] < 65536
    # flagship shape: sampled bits + the whole valid + the ids, as written
    total = a.size * 32 * 62 * 4 + 65536 * 32 * 4 + a.size * 8
    assert a.size < 65536 and total <= 64_000_000
    # a shard that fits is written whole
    assert (bench.dump_channels(4096, 8) == np.arange(4096)).all()


def test_dump_outputs_files(tmp_path):
    rng = np.random.default_rng(1)
    bits = torch.from_numpy(rng.integers(0, 2, (100, 4, 62), dtype=np.uint8))
    valid = torch.from_numpy(rng.integers(0, 2, (100, 4), dtype=np.uint8))
    w = bench.dump_outputs(str(tmp_path / "d"), bits, valid, c0=300, suffix="_rank1")
    assert w == {"channels_rank1.npy": [100], "bits_rank1.npy": [100, 4, 62],
                 "valid_rank1.npy": [100, 4]}
    b = np.load(tmp_path / "d" / "bits_rank1.npy")
    v = np.load(tmp_path / "d" / "valid_rank1.npy")
    c = np.load(tmp_path / "d" / "channels_rank1.npy")
    assert b.dtype == np.float32 and v.dtype == np.float32 and c.dtype == np.float64
    assert (b == bits.numpy()).all() and (v == valid.numpy()).all()
    assert (c == np.arange(300, 400)).all()


def test_dump_outputs_samples_a_large_shard(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BITS_BYTES", 10 * 4 * 62 * 4)     # 10 channels of 4 frames
    monkeypatch.setattr(bench, "DUMP_VALID_BYTES", 50 * 4 * 4)         # < 100 channels
    rng = np.random.default_rng(2)
    bits = torch.from_numpy(rng.integers(0, 2, (100, 4, 62), dtype=np.uint8))
    valid = torch.from_numpy(rng.integers(0, 2, (100, 4), dtype=np.uint8))
    bench.dump_outputs(str(tmp_path), bits, valid)
    c = np.load(tmp_path / "channels.npy").astype(np.int64)
    assert c.size == 10 and (c == bench.dump_channels(100, 4)).all()
    assert (np.load(tmp_path / "bits.npy") == bits.numpy()[c]).all()
    assert (np.load(tmp_path / "valid.npy") == valid.numpy()[c]).all()
