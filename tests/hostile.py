"""Deterministic hostile inputs: int16 streams on which the reference's Kalman
equalizer leaves fp32 range inside a frame (soft symbols of 1e36, inf, NaN on
valid frames) and on which its C99 complex products take the Annex G recovery.

Plain module, integer arithmetic only (numpy int64, shifts and masks), so the
samples are the same on every machine and numpy version.  The rows are data:
tests/golden/hostile_params.json, chosen by a CPU sweep against the unmodified
reference (tests/golden/make_golden.py --hostile-sweep).  t is the sample index
of the whole stream (frame n holds t in [1880 n, 1880 n + 1880)); a phase step
of k per sample is k * 8000 / 65536 Hz.

Group "wave" (rows of hostile_params.json["wave"]):
  square(k, p, a)   a if ((t*k + p) & 65535) < 32768 else -a
  tri(k, p, a)      ph = (t*k + p) & 65535;
                    v = (ph if ph < 32768 else 65535 - ph) - 16384;  (v*a) >> 14
  {"sum": [r1, r2]} (r1 + r2) >> 1
  {"gate": g, ...}  the row's samples where ((t*g) & 65535) < 32768, else 0
Group "impaired" (rows of ["impaired"]): integer impairments of the modem's own
noiseless signal oracle.synth(seed, ...)[c]:
  echo (d, num)     x[t] + ((x[t - d] * num) >> 1)   (num 2, -2, 1: gains 1, -1, 1/2)
  gain g            x * g
  dc o              x + o
  step (at, sh)     x >> sh before sample `at`, x from there on
each clipped to int16.
"""
import functools
import json
import os

import numpy as np

import oracle
from rxcheck import frozen

FRAME = 1880
NFRAMES = 12
PARAMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hostile_params.json")


def _t(nframes):
    return np.arange(nframes * FRAME, dtype=np.int64)


def square(k, p, a, nframes=NFRAMES):
    ph = (_t(nframes) * k + p) & 65535
    return np.where(ph < 32768, a, -a).astype(np.int64)


def tri(k, p, a, nframes=NFRAMES):
    ph = (_t(nframes) * k + p) & 65535
    v = np.where(ph < 32768, ph, 65535 - ph) - 16384
    return (v * a) >> 14


def wave(row, nframes=NFRAMES):
    """One row of the "wave" group as int64 samples."""
    if "sum" in row:
        a, b = (wave(r, nframes) for r in row["sum"])
        y = (a + b) >> 1
    else:
        y = {"square": square, "tri": tri}[row["kind"]](row["k"], row["p"], row["a"], nframes)
    if "gate" in row:
        y = np.where(((_t(nframes) * row["gate"]) & 65535) < 32768, y, 0)
    return y


def impair(x, row):
    """One row of the "impaired" group applied to the int16 stream x."""
    x = x.astype(np.int64)
    kind = row["kind"]
    if kind == "echo":
        d = row["d"]
        delayed = np.concatenate([np.zeros(d, np.int64), x[:-d]])
        y = x + ((delayed * row["num"]) >> 1)
    elif kind == "gain":
        y = x * row["g"]
    elif kind == "dc":
        y = x + row["o"]
    elif kind == "step":
        y = np.where(_t(x.size // FRAME) < row["at"], x >> row["sh"], x)
    else:
        raise ValueError(kind)
    return y


def _i16(y, nframes):
    return np.clip(y, -32768, 32767).astype(np.int16).reshape(nframes, FRAME)


def params():
    with open(PARAMS) as f:
        return json.load(f)


def waves(rows=None, nframes=NFRAMES):
    """The "wave" group [nch][nframes][1880] int16."""
    rows = params()["wave"] if rows is None else rows
    return np.stack([_i16(wave(r, nframes), nframes) for r in rows])


def impaired(rows=None, nframes=NFRAMES):
    """The "impaired" group [nch][nframes][1880] int16."""
    rows = params()["impaired"] if rows is None else rows
    out = []
    for r in rows:
        x = oracle.synth(r["seed"], 1, nframes, 1000.0, c0=r["c"])[0].reshape(-1)
        out.append(_i16(impair(x, r), nframes))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def group(name):
    """A group's samples at the table's frame count, made once, read-only."""
    return frozen(waves() if name == "wave" else impaired())[0]


@functools.lru_cache(maxsize=None)
def expected(name, mode=0):
    """The oracle's (bits, valid, trace) for a group, computed once, read-only."""
    return frozen(*oracle.cpu_rx(group(name), trace=True, mode=mode))
