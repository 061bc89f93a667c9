"""The receive-path tests' one comparison with the oracle, and the helpers they
share.  Plain module (no test, no fixture), imported like tests/timing.py.

A receive result is the dict a Receiver.demod(trace=True, soft=True) call
returns: bits [nch][nf][62] u8, valid [nch][nf] u8, trace [nch][nf][4] int32 in
TRACE_COLS order, soft [nch][nf][31][2] float32.  `differences` compares one
with the oracle's:
- valid, bits and each of the four trace columns exact;
- soft symbols of valid frames bit for bit (the uint32 views: the sign of zero
  and a NaN's payload count).  nan_as_class=True lets an expected NaN accept
  any NaN (a GPU's NaN payloads and signs need not be x86's); without it the
  expected soft symbols of valid frames must hold no NaN, so a corpus that needs
  the class rule has to ask for it;
- soft symbols of invalid frames all bits zero (-0 is a difference).
Only the keys present in the result are compared: trace and soft are optional.
Shapes must match (nothing is broadcast) and soft symbols are float32.

What does not come through here, on purpose:
- tests/test_gpu_rx_writeset.py compares whole guarded buffers (the outputs and
  the bytes around them) with an image built from `dense`;
- tests/test_gpu_frame_index.py's call of more than 2^32 samples compares its
  2.3 million channel-frames on the device, by these rules written in torch;
- results that are bits or flags alone (a stream's chunks after a stall, a
  second context's bits, the drop-in qpsk_rx_frame, files of records) and
  golden files kept as md5 sums or JSON;
- one GPU result against another (split calls, snapshots), and records against
  compact_host.
"""
import ctypes

import numpy as np

import oracle

KEYS = ("bits", "valid", "trace", "soft")
TRACE_COLS = ("max_index", "matches", "valid", "rx_timing")
# every forced (QPSK_SHAPE, QPSK_WIDTH): the lane backs (4x2, 2x4 dual, 1x8 W = 64) and the quad backs (W = 32, 16)
ALL_SHAPES = [("4x2", None), ("2x4d", None), ("1x8", "64"), ("1x8", "32"), ("1x8", "16")]


def frozen(*items):
    """Marks arrays, dicts of arrays and Nones read-only; returns them."""
    for it in items:
        for a in (it.values() if isinstance(it, dict) else (it,)):
            if a is not None:
                a.setflags(write=False)
    return items


def dense(bits, valid, tr):
    """The oracle's (bits, valid, trace records) as the dict a
    Receiver.demod(trace=True, soft=True) call returns: the four trace columns
    as int32 [nch][nf][4], soft as float32 with invalid frames zeroed."""
    trace = np.stack([tr[k] for k in TRACE_COLS], axis=-1).astype(np.int32)
    soft = np.ascontiguousarray(tr["soft"], np.float32).copy()
    soft[valid == 0] = 0.0
    return {"bits": bits, "valid": valid, "trace": trace, "soft": soft}


def expected(x, mode=0):
    """The oracle's dense outputs for x from a fresh start, read-only."""
    return frozen(dense(*oracle.cpu_rx(x, trace=True, mode=mode)))[0]


def same_soft(got, exp):
    """Soft symbols with NaN as a class: finite values and infinities bit for
    bit, an expected NaN against any NaN.  Returns the mask of differing
    elements."""
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    nan = np.isnan(exp)
    return np.where(nan, ~np.isnan(got), got.view(np.uint32) != exp.view(np.uint32))


def _first(mask):
    """(count, first channel-frame) of a [nch][nframes][...] mask"""
    m = mask.reshape(mask.shape[0], mask.shape[1], -1).any(-1)
    cf = np.argwhere(m)
    return int(m.sum()), (tuple(int(v) for v in cf[0]) if len(cf) else None)


def differences(got, exp, *, nan_as_class=False):
    """{output name: (count of differing channel-frames, first (channel, frame))}
    of a receive result against exp, a `dense` dict or the oracle's (bits,
    valid, tr) triple.  Names: valid, bits, trace.<column>, soft(valid),
    soft(invalid) != 0."""
    if not isinstance(exp, dict):
        exp = dense(*exp)
    for k in KEYS:
        if k in got:   # nothing is broadcast
            assert got[k].shape == exp[k].shape, f"{k}: shape {got[k].shape}, expected {exp[k].shape}"
    vm = np.asarray(exp["valid"]).astype(bool)[..., None, None]
    checks = [("valid", got["valid"] != exp["valid"]), ("bits", got["bits"] != exp["bits"])]
    if "trace" in got:
        for col, k in enumerate(TRACE_COLS):
            checks.append(("trace." + k, got["trace"][..., col] != exp["trace"][..., col]))
    if "soft" in got:
        gs, es = np.ascontiguousarray(got["soft"]), np.ascontiguousarray(exp["soft"])
        assert gs.dtype == es.dtype == np.float32, f"soft: dtypes {gs.dtype}, {es.dtype}"   # and nothing is cast
        if nan_as_class:
            diff = same_soft(gs, es)
        else:
            assert not (np.isnan(es) & vm).any(), "expected NaN on valid frames: this corpus needs nan_as_class=True"
            diff = gs.view(np.uint32) != es.view(np.uint32)
        checks.append(("soft(valid)", diff & vm))
        checks.append(("soft(invalid) != 0", (gs.view(np.uint32) != 0) & ~vm))
    bad = {}
    for name, mask in checks:
        n, at = _first(mask)
        if n:
            bad[name] = (n, at)
    return bad


def assert_same(got, exp, what="", *, nan_as_class=False):
    """Every output of a receive result against the oracle's; the message names
    each differing output with its count and first differing (channel, frame)."""
    bad = differences(got, exp, nan_as_class=nan_as_class)
    for name, (n, at) in bad.items():
        print(f"{what}: {name} differs on {n} channel-frames, first at (channel, frame) {at}")
    assert not bad, f"{what}: {bad}"


def demod_in_calls(rx, x, calls, **kw):
    """x fed to rx as consecutive contiguous calls of the given frame counts
    (trace=True, soft=True unless overridden); the calls' outputs concatenated."""
    assert sum(calls) == x.shape[1]
    kw = {"trace": True, "soft": True, **kw}
    parts, a = [], 0
    for n in calls:
        parts.append(rx.demod(np.ascontiguousarray(x[:, a:a + n]), **kw))
        a += n
    return {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0]}


def force_shape(monkeypatch, shape, width):
    """QPSK_SHAPE / QPSK_WIDTH for the contexts made from here on (None: pick_shape's choice)."""
    if shape:
        monkeypatch.setenv("QPSK_SHAPE", shape)
    if width:
        monkeypatch.setenv("QPSK_WIDTH", width)


def live_handles():
    """The library's count of live HIP allocations and handles (internal)."""
    import singlecarrier_amd as sc
    f = sc.lib().qpsk_hip_live_handles
    f.restype = ctypes.c_long
    return int(f())
