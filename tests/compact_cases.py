"""Inputs of the compaction tests (tests/test_compact_host.py on the CPU,
tests/test_gpu_compact.py on the GPU): random dense receive outputs and
sentinel-filled record arrays.  Plain module."""
import numpy as np

import singlecarrier_amd as sc

SENT = 0xA5   # the fill of every output array before a call


def random_dense(rng, nch, nf, density, odd_bytes=False):
    valid = (rng.random((nch, nf)) < density).astype(np.uint8)
    valid *= rng.integers(1, 4, (nch, nf), dtype=np.uint8)   # any nonzero flag is valid
    bits = rng.integers(0, 2, (nch, nf, 62), dtype=np.uint8)
    if odd_bytes:
        bits[rng.random(bits.shape) < 0.2] = 2
        bits[rng.random(bits.shape) < 0.2] = 255
    trace = rng.integers(-2**31, 2**31 - 1, (nch, nf, 4)).astype(np.int32)
    soft = rng.standard_normal((nch, nf, 31, 2)).astype(np.float32)
    return bits, valid, trace, soft


def filled(cap, ngroups):
    o = {"rec": np.zeros(cap, sc.REC_DTYPE), "trace": np.zeros((cap, 4), np.int32),
         "soft": np.zeros((cap, 31, 2), np.float32), "groups": np.zeros(ngroups + 1, np.uint32)}
    for a in o.values():
        a.view(np.uint8)[...] = SENT
    return o
