"""Inputs and numpy restatements of the level meter and squelch tests
(tests/test_level_host.py on the CPU, tests/test_gpu_level.py on the GPU),
written from include/qpsk_level.h alone.  Plain module."""
import functools

import numpy as np

import singlecarrier_amd as sc

SENT = 0xA5          # the fill of every output array before a call
N = sc.FRAME_SIZE
MIN_SUMSQ = 10**9    # the squelch level of the oracle case
SINGLE_AT = (0, 7, 8, 1871, 1872, 1879)   # the ends of the first and last 16-byte words of a row


def special_rows() -> np.ndarray:
    """int16 [12][1880]: both rails, alternating rails, one sample at the edges
    of a row's first and last 16-byte words, and silence."""
    rows = [np.full(N, -32768), np.full(N, 32767), np.where(np.arange(N) % 2 == 0, 32767, -32767)]
    for k, at in enumerate(SINGLE_AT):
        r = np.zeros(N)
        r[at] = (-32768, 32767, -1, 1, 12345, -32767)[k]
        rows.append(r)
    rows += [np.zeros(N), np.where(np.arange(N) % 2 == 0, -32768, 32767), np.arange(N) - 940]
    return np.ascontiguousarray(np.stack(rows).astype(np.int16))


def rows(n: int, seed: int = 1) -> np.ndarray:
    """int16 [n][1880]: random rows (full range, and a quiet line) with the
    special rows spread among them and one of them last."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, (n, N)).astype(np.int16)
    x[1::5] = rng.integers(-200, 201, x[1::5].shape).astype(np.int16)
    sp = special_rows()
    for k in reversed(range(min(n, len(sp)))):
        x[n - 1 - (k * 3) % n] = sp[k]   # k = 0 (a row of -32768) is written last, to the last row
    return x


def restate_level(x) -> np.ndarray:
    """LEVEL_DTYPE [...] of int16 [...][1880], in numpy int64."""
    v = np.asarray(x).astype(np.int64)
    out = np.zeros(v.shape[:-1], sc.LEVEL_DTYPE)
    out["sumsq"] = (v * v).sum(-1)
    out["sum"] = v.sum(-1)
    out["peak"] = np.abs(v).max(-1)
    out["clipped"] = ((v == 32767) | (v == -32768)).sum(-1)
    return out


def restate_squelch(level, prev, min_sumsq, valid, bits=None, soft=None):
    """(valid_out, last, bits, soft) by the header's definition; prev None is
    the start of a stream."""
    nch, nf = valid.shape
    q = level["sumsq"].reshape(nch, nf).astype(object)   # python ints: no width to think about
    p0 = np.zeros(nch, object) if prev is None else prev["sumsq"].astype(object)
    p = np.concatenate([p0[:, None], q[:, :-1]], axis=1) if nf else q
    keep = np.maximum(q, p) >= min_sumsq
    out = np.where(keep, valid, 0).astype(np.uint8)
    gone = (valid != 0) & ~keep
    if bits is not None:
        bits = bits.copy()
        bits[gone] = 0
    if soft is not None:
        soft = soft.copy()
        soft[gone] = 0.0
    if nf:
        last = level.reshape(nch, nf)[:, -1].copy()
    else:
        last = np.zeros(nch, sc.LEVEL_DTYPE) if prev is None else prev.copy()
    return out, last, bits, soft


def random_squelch_case(rng, nch, nf):
    """Levels around MIN_SUMSQ, flags 0..3, sentinel-like dense rows."""
    level = np.zeros((nch, nf), sc.LEVEL_DTYPE)
    level["sumsq"] = rng.choice([0, 1, MIN_SUMSQ - 1, MIN_SUMSQ, MIN_SUMSQ + 1, sc.FULL_SUMSQ], (nch, nf))
    level["sum"] = rng.integers(-1000, 1000, (nch, nf))
    level["peak"] = rng.integers(0, 32769, (nch, nf))
    level["clipped"] = rng.integers(0, 1881, (nch, nf))
    prev = np.zeros(nch, sc.LEVEL_DTYPE)
    prev["sumsq"] = rng.choice([0, MIN_SUMSQ - 1, MIN_SUMSQ, sc.FULL_SUMSQ], nch)
    prev["sum"] = rng.integers(-1000, 1000, nch)
    valid = rng.integers(0, 4, (nch, nf)).astype(np.uint8)
    bits = rng.integers(1, 256, (nch, nf, sc.NBITS)).astype(np.uint8)          # no zero byte:
    soft = (rng.integers(1, 1000, (nch, nf, sc.DATA_SYMBOLS, 2))).astype(np.float32)   # a zeroed row shows
    return level, prev, valid, bits, soft


@functools.lru_cache(maxsize=None)
def oracle_case(mode: int = 0):
    """The squelch on the oracle: oracle.synth(7, 8, 8, 1000.0, c0=100) with
    frame (c, f) zeroed unless (c + f) % 3 == 0.  Returns (x, dense outputs of
    the oracle, levels by numpy); read-only, made once per mode."""
    import oracle
    import rxcheck
    x = oracle.synth(7, 8, 8, 1000.0, c0=100)
    c, f = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    x[(c + f) % 3 != 0] = 0
    d = rxcheck.expected(x, mode)
    level = restate_level(x)
    x.setflags(write=False)
    level.setflags(write=False)
    return x, d, level


def oracle_classes(d, level):
    """The oracle case's frames by class: (kept on their own energy, kept only
    because of the previous frame, squelched, invalid), boolean [8][8] each."""
    q = level["sumsq"]
    v = d["valid"] != 0
    own = q >= MIN_SUMSQ
    before = np.concatenate([np.zeros((q.shape[0], 1), bool), own[:, :-1]], axis=1)
    return v & own, v & ~own & before, v & ~own & ~before, ~v


@functools.lru_cache(maxsize=None)
def silence_case(mode: int = 0):
    """All-zero input of 2 x 6 frames and the oracle's dense outputs."""
    import rxcheck
    x = np.zeros((2, 6, N), np.int16)
    x.setflags(write=False)
    return x, rxcheck.expected(x, mode)


def squelched_records(d, level, prev, min_sumsq, order, cap=None):
    """The records the squelch calls must give: the oracle's dense outputs
    through the host twins (squelch_host, then compact_host)."""
    s = sc.squelch_host(level, d["valid"], min_sumsq, prev=prev)
    exp = sc.compact_host(d["bits"], s["valid"], d["trace"], d["soft"], order=order, cap=cap)
    return exp, s["last"]


def filled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = SENT
    return a
