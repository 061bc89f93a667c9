"""Stream order of the device entry points with work still in flight (run with
-m gpu).

Every device call takes a `stream`, enqueues there and returns.  The rest of
the suite calls them on an idle GPU and synchronises before it looks, so a
launch or an upload on the wrong stream would still read finished input and
still be done in time.  Here a bounded delay (tests/gpu_delay.py: a kernel that
waits on the device's wall clock) sits on the caller's stream in front of the
work: when the host has finished enqueueing, nothing behind the delay has
started.  The real input is copied into the
device buffer on that stream (before, the buffer holds another seed's stream:
a premature read gives plausible output), the outputs are cloned on that
stream, and input and outputs are overwritten behind the clones, so work that
ran early or late computes from, or leaves, something else.

D, the delay: with warm contexts and no delay the longest enqueue sequence of
this module takes E of host time (measured by the `D` fixture on the three
receive sequences of section A); D = max(100 ms, 20 E), at most 500 ms; 20
covers host jitter on a shared machine.  Each test times its own delay with
events and asserts it lasted 0.9 D (`_Late.premise`); a test that claims "did
not wait" also asserts that the host time of its whole enqueue sequence stayed
below D / 2 and that the delay was still running when the last enqueue
returned (`_Late.check`).  A warm-up's tensors are released before the delayed
pass, so that pass finds its memory in torch's cache and allocates nothing
while the delay runs.

Expected values: oracle.cpu_rx over the whole stream in one call,
sc.tx_batch_host and the host twins of the stateless passes.  Every comparison
is on the bits.
"""
import ctypes as C
import time

import numpy as np
import pytest

import gpu_delay
import oracle
import rxcheck
import singlecarrier_amd as sc
from rxcheck import KEYS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NCH, NF = 96, 12
CUTS = ((0, 1), (1, 4), (4, 12))         # calls of 1 + 3 + 8 frames
SEED, DECOY = 41, 42
ALAW_I = sc.IN_ALAW | sc.IN_INTERLEAVED
ORDERS = [sc.REC_BY_CHANNEL, sc.REC_BY_FRAME]
KNOBS = ("QPSK_SHAPE", "QPSK_WIDTH", "QPSK_HEADPASS")
SHAPES = {"default": {},                                  # 96 channels: quad backs, W = 16
          "1x8w64": {"QPSK_SHAPE": "1x8", "QPSK_WIDTH": "64"},   # lane backs
          "2x4d": {"QPSK_SHAPE": "2x4d"},
          "4x2": {"QPSK_SHAPE": "4x2"},
          "4x2head": {"QPSK_SHAPE": "4x2", "QPSK_HEADPASS": "1"}}   # head_kernel: a third launch in front
# what the context then reports (qpsk_rx_plan_name)
PLANS = {"default": "1x8q16", "1x8w64": "1x8d64", "2x4d": "2x4d", "4x2": "4x2", "4x2head": "4x2+head"}


# ------------------------------------------------------------------ expected
def _cut(d, a, e, c0=0, c1=None):
    return {k: np.ascontiguousarray(d[k][c0:c1, a:e]) for k in KEYS}


def _pieces_depend(d, counts=None):
    """Every call has valid frames, the second and third valid and invalid
    ones: each piece then depends on the state the previous one left."""
    got = [(int(d["valid"][:, a:e].sum()), d["valid"][:, a:e].size) for a, e in CUTS]
    if counts is not None:
        assert got == counts
    assert got[0][0] > 0 and all(0 < n < size for n, size in got[1:]), got


@pytest.fixture(scope="module")
def signal():
    """The stream of every receive test, another seed's as the decoy, and the
    oracle's outputs of the first; made once, never changed."""
    x = oracle.synth(SEED, NCH, NF, 1000.0)
    decoy = oracle.synth(DECOY, NCH, NF, 1000.0)
    exp = {oracle.MODE_REF: rxcheck.expected(x)}
    _pieces_depend(exp[oracle.MODE_REF], [(96, 96), (210, 288), (270, 768)])
    m = oracle.MODE_DEC752 | oracle.MODE_FFT_HUNT
    exp[m] = rxcheck.expected(x, m)
    _pieces_depend(exp[m])
    for a in (x, decoy):
        a.setflags(write=False)
    return x, decoy, exp


@pytest.fixture(scope="module")
def alaw(signal):
    """The stream as interleaved A-law codes [T][nch] (the decoy alike) and the
    oracle's outputs of what the codes decode to."""
    x, decoy, _ = signal
    codes = [sc.output_convert_host(a.reshape(NCH, -1), sc.OUT_ALAW | sc.OUT_INTERLEAVED) for a in (x, decoy)]
    exp = rxcheck.expected(sc.input_convert_host(codes[0], ALAW_I, NCH))
    _pieces_depend(exp)
    return codes[0], codes[1], exp


def _same(got, exp):
    for k in KEYS:
        np.testing.assert_array_equal(got[k], exp[k], err_msg=k)


def _rec_same(got, exp_dense, order):
    """The record tensors of a device call (on the host) against the host
    compaction of the oracle's dense outputs."""
    exp = sc.compact_host(exp_dense["bits"], exp_dense["valid"], exp_dense["trace"], exp_dense["soft"], order=order)
    count = int(got["count"].view(np.uint32)[0])
    assert count == exp["count"]
    np.testing.assert_array_equal(got["groups"].view(np.uint32), exp["groups"])
    rec = np.ascontiguousarray(got["rec"][:count]).view(sc.REC_DTYPE).reshape(-1)
    assert rec.tobytes() == exp["rec"].tobytes()
    np.testing.assert_array_equal(got["trace"][:count], exp["trace"])
    assert got["soft"][:count].tobytes() == exp["soft"].tobytes()


# ------------------------------------------------------------------ the delayed sequence
def _pinned(a):
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()


def _outs(nch, nf):
    z = dict(device="cuda")
    return {"bits": torch.zeros((nch, nf, sc.NBITS), dtype=torch.uint8, **z),
            "valid": torch.zeros((nch, nf), dtype=torch.uint8, **z),
            "trace": torch.zeros((nch, nf, 4), dtype=torch.int32, **z),
            "soft": torch.zeros((nch, nf, sc.DATA_SYMBOLS, 2), dtype=torch.float32, **z)}


def _clobber(t):
    t.view(torch.uint8).fill_(0xA5)


class _Late:
    """One delayed sequence on stream S.  feed(): device buffers that hold a
    decoy now and get their real contents from pinned memory on S, behind the
    delay.  After the calls: keep() clones results on S, finish() overwrites
    the fed inputs (zeros) and the given outputs (0xA5) on S and stops the
    host clock.  delay_ms None: no delay (warm-up, and the measurement of E)."""

    def __init__(self, S, delay_ms):
        self.S, self.asked = S, delay_ms
        self.fed, self.kept = [], []
        self.delay = gpu_delay.put(S, delay_ms) if delay_ms else None
        self.t0 = time.perf_counter()
        self.host_ms = self.running = None

    def feed(self, pairs):
        with torch.cuda.stream(self.S):
            for dev, pin in pairs:
                dev.copy_(pin, non_blocking=True)
                self.fed.append(dev)

    def keep(self, tensors):
        """tensors: a dict (None values are left out); returns the dict of clones"""
        with torch.cuda.stream(self.S):
            c = {k: v.clone() for k, v in tensors.items() if v is not None}
        self.kept.append(c)
        return c

    def finish(self, outputs=()):
        with torch.cuda.stream(self.S):
            for t in self.fed:
                t.zero_()
            for t in outputs:
                if t is not None:
                    _clobber(t)
        self.host_ms = (time.perf_counter() - self.t0) * 1e3
        self.running = self.delay.running() if self.delay else None
        return self

    def premise(self):
        """(after a synchronisation) the delay was a delay"""
        if self.delay is None:
            return
        lasted = self.delay.ms()
        print(f"delay {lasted:.1f} ms of {self.asked:.1f} ms asked")
        assert lasted >= 0.9 * self.asked, f"premise: the delay lasted {lasted:.2f} ms of {self.asked:.1f} ms asked"

    def check(self, did_not_wait):
        """(after a synchronisation) the premise, and where claimed, that the
        host got through the whole sequence while the delay ran"""
        if self.delay is None:
            return
        self.premise()
        print(f"host {self.host_ms:.3f} ms, delay running at the last enqueue: {self.running}")
        if did_not_wait:
            assert self.host_ms < self.asked / 2, \
                f"the enqueue sequence took {self.host_ms:.2f} ms of host time behind a delay of {self.asked:.1f} ms"
            assert self.running, "the delay had ended when the last enqueue returned: a call waited for the stream"


def _host(c):
    return {k: v.cpu().numpy() for k, v in c.items()}


def _rx_sequence(rx, kind, S, s_arg, real, decoy, delay_ms, order=None, streams=None):
    """Section A's sequence: the three calls of CUTS on rx.  kind: "plain"
    (demod_device), "fmt" (demod_device_fmt, interleaved A-law) or "rec"
    (demod_records_device).  s_arg: the calls' stream argument (None with S
    torch's null stream).  streams: the stream of each call when the caller
    chains two (section C); the clones are then made on S behind the last.
    Returns (the _Late, the three calls' outputs on the host): left for the
    caller to synchronise."""
    def piece(a, lo, hi):
        if kind == "fmt":   # [T][nch]
            return a[lo * sc.FRAME_SIZE:hi * sc.FRAME_SIZE]
        return a[:, lo:hi]

    pins = [_pinned(piece(real, a, e)) for a, e in CUTS]
    devs = [torch.from_numpy(np.ascontiguousarray(piece(decoy, a, e))).cuda() for a, e in CUTS]
    outs = [_outs(NCH, e - a) for a, e in CUTS] if kind != "rec" else []
    torch.cuda.synchronize()
    late = _Late(S, delay_ms)
    late.feed(zip(devs, pins))
    for i, dx in enumerate(devs):
        s = s_arg
        if streams is not None:
            s = streams[i]
            if i > 0:
                s.wait_stream(streams[i - 1])
        if kind == "plain":
            rx.demod_device(dx, stream=s, **outs[i])
        elif kind == "fmt":
            rx.demod_device_fmt(dx, ALAW_I, stream=s, **outs[i])
        else:
            outs.append(rx.demod_records_device(dx, order=order, trace=True, soft=True, stream=s))
    if streams is not None:
        S.wait_stream(streams[-1])
    clones = [late.keep(o) for o in outs]
    late.finish([t for o in outs for t in o.values()])
    return late, clones, (pins, devs, outs)


def _rx_check(clones, exp, kind, order=None):
    for (a, e), c in zip(CUTS, clones):
        if kind == "rec":
            _rec_same(_host(c), _cut(exp, a, e), order)
        else:
            _same(_host(c), _cut(exp, a, e))


def _drain(rx, *streams):
    for s in streams:
        s.synchronize()
    rx.sync()


def _plan(rx):
    """The rx_kernel shape the context's calls launch (+head: with the head
    pre-pass), by the library's internal qpsk_rx_plan_name."""
    f = sc.lib().qpsk_rx_plan_name
    f.restype, f.argtypes = C.c_char_p, [C.c_void_p]
    return f(rx._h).decode()


def _receiver(monkeypatch, shape="default", mode=sc.MODE_REFERENCE):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in SHAPES[shape].items():
        monkeypatch.setenv(k, v)
    rx = sc.Receiver(NCH, mode=mode)
    for k in SHAPES[shape]:
        monkeypatch.delenv(k)
    assert _plan(rx) == PLANS[shape]   # the knobs took: the case runs the kernels it names
    return rx


@pytest.fixture(scope="module")
def D(signal, alaw):
    """The module's delay in ms, from E: the host time of the longest enqueue
    sequence (section A's, in its three kinds) on warm contexts without a delay."""
    x, decoy, _ = signal
    S = torch.cuda.Stream()
    probe = [gpu_delay.put(S, ms).ms() for ms in (1.0, 1.0, 20.0)]   # the first loads the kernel
    rx = sc.Receiver(NCH)
    times = {}
    for kind, real, dec in (("plain", x, decoy), ("fmt", alaw[0], alaw[1]), ("rec", x, decoy)):
        runs = []
        for _ in range(4):   # the first is the warm-up
            late, clones, hold = _rx_sequence(rx, kind, S, S, real, dec, None, order=sc.REC_BY_CHANNEL)
            _drain(rx, S)
            rx.reset()
            runs.append(late.host_ms)
            del late, clones, hold
        times[kind] = float(np.median(runs[1:]))
    rx.close()
    E = max(times.values())
    d = min(500.0, max(100.0, 20.0 * E))
    print(f"\nasync contract: wall clock {gpu_delay.clock_khz()} kHz, delays of 1 and 20 ms lasted "
          f"{probe[1]:.3f} and {probe[2]:.3f} ms; enqueue host time " + ", ".join(f"{k} {v:.3f} ms" for k, v in times.items()) +
          f"; E = {E:.3f} ms, D = {d:.1f} ms")
    return d


def test_the_delay_is_bounded():
    S = torch.cuda.Stream()
    for ms in (0, -1, gpu_delay.MAX_MS + 1):
        with pytest.raises(ValueError):
            gpu_delay.put(S, ms)
    assert gpu_delay.MAX_MS <= 1000.0


# ------------------------------------------------------------------ A. receive
def _section_a(rx, kind, D, real, decoy, exp, order=None, null_stream=False):
    S = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    s_arg = None if null_stream else S
    # warm-up with the same call sizes, then reset
    warm = _rx_sequence(rx, kind, S, s_arg, real, decoy, None, order=order)
    _drain(rx, S)
    del warm   # its tensors go back to torch's cache: the delayed pass allocates nothing new
    rx.reset()
    late, clones, hold = _rx_sequence(rx, kind, S, s_arg, real, decoy, D, order=order)
    _drain(rx, S)
    late.check(did_not_wait=True)
    _rx_check(clones, exp, kind, order)
    rx.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_receive_behind_and_in_front_of_its_stream(signal, D, monkeypatch, shape):
    x, decoy, exp = signal
    _section_a(_receiver(monkeypatch, shape), "plain", D, x, decoy, exp[oracle.MODE_REF])


def test_receive_dec752_fft_hunt(signal, D, monkeypatch):
    x, decoy, exp = signal
    m = sc.MODE_DEC752 | sc.MODE_FFT_HUNT
    _section_a(_receiver(monkeypatch, mode=m), "plain", D, x, decoy, exp[m])


def test_receive_fmt_interleaved_alaw(alaw, D, monkeypatch):
    codes, decoy, exp = alaw
    _section_a(_receiver(monkeypatch), "fmt", D, codes, decoy, exp)


@pytest.mark.parametrize("order", ORDERS)
def test_receive_records(signal, D, monkeypatch, order):
    x, decoy, exp = signal
    _section_a(_receiver(monkeypatch), "rec", D, x, decoy, exp[oracle.MODE_REF], order=order)


def test_receive_on_the_null_stream(signal, D, monkeypatch):
    """stream=None: the caller's work, the delay and the calls on torch's
    current stream, the legacy null stream"""
    x, decoy, exp = signal
    assert torch.cuda.current_stream().cuda_stream == 0
    _section_a(_receiver(monkeypatch), "plain", D, x, decoy, exp[oracle.MODE_REF], null_stream=True)


# ------------------------------------------------------------------ B. buffers that grow
@pytest.mark.parametrize("kind,shape", [("plain", "default"), ("plain", "4x2head"), ("fmt", "default"),
                                        ("rec", "default")])
def test_buffers_grow_with_calls_pending(signal, alaw, D, monkeypatch, kind, shape):
    """A fresh context, calls of 1, 3 and 8 frames back to back behind the
    delay: the job queue (with the head pre-pass, its buffer too), the
    converted block or the record buffers grow at every call.  A growing call
    may wait for the device (include/qpsk_batch.h), so no "did not wait" here."""
    x, decoy, exp = signal
    real, dec, e = (alaw[0], alaw[1], alaw[2]) if kind == "fmt" else (x, decoy, exp[oracle.MODE_REF])
    rx = _receiver(monkeypatch, shape)
    S = torch.cuda.Stream()
    late, clones, hold = _rx_sequence(rx, kind, S, S, real, dec, D, order=sc.REC_BY_FRAME)
    _drain(rx, S)
    late.check(did_not_wait=False)
    _rx_check(clones, e, kind, sc.REC_BY_FRAME)
    rx.close()


# ------------------------------------------------------------------ C. chained streams, timing
def test_two_chained_streams_and_timing(signal, D, monkeypatch):
    x, decoy, exp = signal
    rx = _receiver(monkeypatch)
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    chain = [S1, S2, S1]
    warm = _rx_sequence(rx, "plain", S1, None, x, decoy, None, streams=chain)
    _drain(rx, S1, S2)
    del warm
    rx.reset()
    rx.timing(True)
    assert rx.collect_timing_split() == (0.0, 0.0, 0)
    late, clones, hold = _rx_sequence(rx, "plain", S1, None, x, decoy, D, streams=chain)
    rx.sync()
    ms_rx, ms_data, frames = rx.collect_timing_split()
    _drain(rx, S1, S2)
    late.check(did_not_wait=True)
    assert frames == NF
    assert np.isfinite(ms_rx) and np.isfinite(ms_data) and ms_rx >= 0 and ms_data >= 0
    rx.timing(False)
    _rx_check(clones, exp[oracle.MODE_REF], "plain")
    rx.close()


def test_timing_pool_folds_with_calls_enqueued():
    """70 timed one-frame device calls without a collect in between: the
    64-slot event pool folds once, with calls still enqueued behind it"""
    nch, nf = 8, 70
    x = oracle.synth(43, nch, nf, 1000.0)
    exp = rxcheck.expected(x)
    assert 0 < exp["valid"].sum() < nch * nf
    S = torch.cuda.Stream()
    # call n's arrays are block n: [nf][nch][1][...]
    dx = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))[:, :, None]).cuda()
    o = _outs(nf * nch, 1)
    o = {k: v.view((nf, nch, 1) + tuple(v.shape[2:])) for k, v in o.items()}
    rx = sc.Receiver(nch)
    rx.timing(True)
    torch.cuda.synchronize()
    for n in range(nf):
        rx.demod_device(dx[n], o["bits"][n], o["valid"][n], o["trace"][n], o["soft"][n], stream=S)
    rx.sync()
    ms_rx, ms_data, frames = rx.collect_timing_split()
    S.synchronize()
    assert frames == nf
    assert np.isfinite(ms_rx) and np.isfinite(ms_data) and ms_rx > 0 and ms_data > 0
    rx.close()
    got = {k: np.ascontiguousarray(np.moveaxis(v.cpu().numpy()[:, :, 0], 0, 1)) for k, v in o.items()}
    _same(got, exp)


# ------------------------------------------------------------------ D. state calls, a call in flight
class _InFlight:
    """A context that received frames 0..4 (synchronised), with the device
    call of frames 4..8 pending on S behind the delay."""

    def __init__(self, monkeypatch, signal, D):
        self.x, decoy, exp = signal
        self.exp = exp[oracle.MODE_REF]
        self.rx = _receiver(monkeypatch)
        self.S = torch.cuda.Stream()
        first = _outs(NCH, 4)
        self.rx.demod_device(torch.from_numpy(self.x[:, :4].copy()).cuda(), stream=self.S, **first)
        _drain(self.rx, self.S)
        _same(_host(first), _cut(self.exp, 0, 4))
        self.pin = _pinned(self.x[:, 4:8])
        self.dx = torch.from_numpy(decoy[:, 4:8].copy()).cuda()
        self.out = _outs(NCH, 4)
        torch.cuda.synchronize()
        self.late = _Late(self.S, D)
        self.late.feed([(self.dx, self.pin)])
        self.rx.demod_device(self.dx, stream=self.S, **self.out)

    def was_pending(self):
        """(right after the call under test returned) the premise of section D"""
        self.S.synchronize()
        self.late.premise()
        _same(_host(self.out), _cut(self.exp, 4, 8))

    def last(self, c0=0, c1=None):
        """frames 8..12 through a device call, on the host"""
        o = _outs(NCH, 4)
        self.rx.demod_device(torch.from_numpy(self.x[:, 8:12].copy()).cuda(), stream=self.S, **o)
        _drain(self.rx, self.S)
        return _host(o)


def _sync_twin(signal, nframes=8):
    """A context that ran the same frames synchronously, in the same calls"""
    x = signal[0]
    rx = sc.Receiver(NCH)
    for a in range(0, nframes, 4):
        rx.demod(x[:, a:a + 4])
    return rx


def test_sync_covers_the_call_in_flight(signal, D, monkeypatch):
    """When sync() returns, a copy made on a fresh stream that never waited
    for S holds the final outputs."""
    f = _InFlight(monkeypatch, signal, D)
    assert f.late.delay.running()
    f.rx.sync()
    fresh = torch.cuda.Stream()
    with torch.cuda.stream(fresh):
        c = {k: v.clone() for k, v in f.out.items()}
    fresh.synchronize()
    _same(_host(c), _cut(f.exp, 4, 8))
    f.was_pending()
    f.rx.close()


def test_reset_channels_with_a_call_in_flight(signal, D, monkeypatch):
    c0, n = 5, 7
    f = _InFlight(monkeypatch, signal, D)
    assert f.late.delay.running()
    f.rx.reset_channels(c0, n)
    f.was_pending()   # the pending call's outputs are the continued stream's, on every channel
    got = f.last()
    fresh = rxcheck.expected(f.x[c0:c0 + n, 8:12])
    assert (fresh["valid"] != f.exp["valid"][c0:c0 + n, 8:12]).any()   # a reset is visible
    _same({k: got[k][c0:c0 + n] for k in KEYS}, fresh)
    _same({k: got[k][:c0] for k in KEYS}, _cut(f.exp, 8, 12, 0, c0))
    _same({k: got[k][c0 + n:] for k in KEYS}, _cut(f.exp, 8, 12, c0 + n))
    f.rx.close()


def test_state_save_with_a_call_in_flight(signal, D, monkeypatch):
    f = _InFlight(monkeypatch, signal, D)
    assert f.late.delay.running()
    snap = f.rx.state_save()
    f.was_pending()
    twin = _sync_twin(signal)
    assert snap == twin.state_save()
    twin.close()
    f.rx.close()


def test_state_join_with_a_call_in_flight(signal, D, monkeypatch):
    """a range joined from another context's snapshot while the call is
    pending: the call's outputs are the continued stream's, and every range's
    state is that of a context that did the same synchronously"""
    c0, n = 5, 7
    donor = sc.Receiver(n)
    donor.demod(signal[1][c0:c0 + n, :3])
    part = donor.state_save()
    donor.close()
    f = _InFlight(monkeypatch, signal, D)
    assert f.late.delay.running()
    f.rx.state_join(part, c0, n)
    f.was_pending()
    twin = _sync_twin(signal)
    twin.state_join(part, c0, n)
    for a, m in ((0, c0), (c0, n), (c0 + n, NCH - c0 - n)):
        assert f.rx.state_save(a, m) == twin.state_save(a, m)
    twin.close()
    f.rx.close()


def test_reset_with_a_call_in_flight(signal, D, monkeypatch):
    f = _InFlight(monkeypatch, signal, D)
    assert f.late.delay.running()
    f.rx.reset()
    f.was_pending()
    assert f.rx.frames == 0
    fresh = sc.Receiver(NCH)
    assert f.rx.state_save() == fresh.state_save()
    fresh.close()
    f.rx.close()


# ------------------------------------------------------------------ E. a host call behind a pending device call
def _section_e(monkeypatch, D, kind, real, decoy, exp, order=None):
    """Device call of frames 0..4 on S behind the delay, then, with no
    synchronisation, the host call of frames 4..12 (the context's buffers are
    as large as either call needs: neither grows one)."""
    def piece(a, lo, hi):
        return a[lo * sc.FRAME_SIZE:hi * sc.FRAME_SIZE] if kind == "fmt" else a[:, lo:hi]

    rx = _receiver(monkeypatch)
    S = torch.cuda.Stream()
    late = out = None
    for delay in (None, D):   # the first pass is the warm-up
        pin = _pinned(piece(real, 0, 4))
        dx = torch.from_numpy(np.ascontiguousarray(piece(decoy, 0, 4))).cuda()
        torch.cuda.synchronize()
        late = _Late(S, delay)
        late.feed([(dx, pin)])
        if kind == "plain":
            out = _outs(NCH, 4)
            rx.demod_device(dx, stream=S, **out)
        elif kind == "fmt":
            out = _outs(NCH, 4)
            rx.demod_device_fmt(dx, ALAW_I, stream=S, **out)
        else:
            out = rx.demod_records_device(dx, order=order, trace=True, soft=True, stream=S)
        pending = late.delay.running() if delay else None
        x2 = np.ascontiguousarray(piece(real, 4, 12))
        if kind == "plain":
            host = rx.demod(x2, trace=True, soft=True)
        elif kind == "fmt":
            host = rx.demod_fmt(x2, ALAW_I, trace=True, soft=True)
        else:
            host = rx.demod_records(x2, order=order, trace=True, soft=True)
        _drain(rx, S)
        if delay is None:
            rx.reset()
    late.premise()
    assert pending   # the device call had not started when the host call was made
    if kind == "rec":
        _rec_same(_host(out), _cut(exp, 0, 4), order)
        e = _cut(exp, 4, 12)
        want = sc.compact_host(e["bits"], e["valid"], e["trace"], e["soft"], order=order)
        assert host["count"] == want["count"]
        np.testing.assert_array_equal(host["groups"], want["groups"])
        assert host["rec"].tobytes() == want["rec"].tobytes()
        np.testing.assert_array_equal(host["trace"], want["trace"])
        assert host["soft"].tobytes() == want["soft"].tobytes()
    else:
        _same(_host(out), _cut(exp, 0, 4))
        _same(host, _cut(exp, 4, 12))
    rx.close()


def test_host_demod_behind_a_pending_device_call(signal, D, monkeypatch):
    x, decoy, exp = signal
    _section_e(monkeypatch, D, "plain", x, decoy, exp[oracle.MODE_REF])


def test_host_demod_fmt_behind_a_pending_device_call(alaw, D, monkeypatch):
    codes, decoy, exp = alaw
    _section_e(monkeypatch, D, "fmt", codes, decoy, exp)


def test_host_demod_records_behind_a_pending_device_call(signal, D, monkeypatch):
    x, decoy, exp = signal
    _section_e(monkeypatch, D, "rec", x, decoy, exp[oracle.MODE_REF], order=sc.REC_BY_CHANNEL)


def test_host_modulate_behind_a_pending_device_call(D):
    nch, gap = 9, 903
    P = sc.TX_PACKET + gap
    bits = _payload(7, nch, 5)
    want = sc.tx_batch_host(bits, gap=gap)
    tx = sc.Transmitter(nch, gap=gap)
    S = torch.cuda.Stream()
    late = out = host = pending = None
    for delay in (None, D):   # warm-up: both staging slots and the carrier table at 3 packets
        pin = _pinned(bits[:, :2])
        db = torch.from_numpy(_payload(8, nch, 2)).cuda()
        out = torch.zeros((nch, 2 * P), dtype=torch.int16, device="cuda")
        if delay is None:
            warm = [(torch.from_numpy(bits[:, :3].copy()).cuda(),
                     torch.zeros((nch, 3 * P), dtype=torch.int16, device="cuda")) for _ in range(2)]
            for wb, wo in warm:
                tx.modulate_device(wb, wo, stream=S)
            tx.sync()
            tx.reset()
        torch.cuda.synchronize()
        late = _Late(S, delay)
        late.feed([(db, pin)])
        tx.modulate_device(db, out, stream=S)
        pending = late.delay.running() if delay else None
        host = tx.modulate(bits[:, 2:])
        S.synchronize()
        tx.sync()
        if delay is None:
            tx.reset()
    late.premise()
    assert pending
    np.testing.assert_array_equal(out.cpu().numpy(), want[:, :2 * P])
    np.testing.assert_array_equal(host, want[:, 2 * P:])
    tx.close()


# ------------------------------------------------------------------ F. transmitter
def _payload(seed, nch, npk):
    return np.random.default_rng(seed).integers(0, 2, (nch, npk, 8, sc.NBITS), dtype=np.uint8)


def _tx_sequence(tx, S, delay_ms, bits, decoy, splits, fmt=None):
    """The packets of `bits` in calls of `splits` on S, each call's payload fed
    late and its block cloned on S.  Returns (the _Late, the clones)."""
    nch, P = tx.nch, sc.TX_PACKET + tx.gap
    cuts = np.concatenate([[0], np.cumsum(splits)])
    pins = [_pinned(bits[:, a:e]) for a, e in zip(cuts[:-1], cuts[1:])]
    devs = [torch.from_numpy(np.ascontiguousarray(decoy[:, a:e])).cuda() for a, e in zip(cuts[:-1], cuts[1:])]
    if fmt is None:
        outs = [torch.zeros((nch, n * P), dtype=torch.int16, device="cuda") for n in splits]
    else:   # interleaved codes
        outs = [torch.zeros((n * P, nch), dtype=torch.uint8, device="cuda") for n in splits]
    torch.cuda.synchronize()
    late = _Late(S, delay_ms)
    late.feed(zip(devs, pins))
    for db, o in zip(devs, outs):
        if fmt is None:
            tx.modulate_device(db, o, stream=S)
        else:
            tx.modulate_device_fmt(db, o, fmt, stream=S)
    clones = [late.keep({"out": o})["out"] for o in outs]
    late.finish(outs)
    return late, clones, (pins, devs, outs)


@pytest.mark.parametrize("gap", [903, 0])
def test_transmit_calls_back_to_back(D, gap):
    """1 + 3 + 1 packets on a fresh context: the second call replaces the
    carrier table while the first call's kernels are pending, the third reuses
    the first call's staging slot"""
    nch, splits = 9, [1, 3, 1]
    bits, decoy = _payload(21 + gap, nch, 5), _payload(22 + gap, nch, 5)
    want = sc.tx_batch_host(bits, gap=gap)
    tx = sc.Transmitter(nch, gap=gap)
    S = torch.cuda.Stream()
    late, clones, hold = _tx_sequence(tx, S, D, bits, decoy, splits)
    S.synchronize()
    tx.sync()
    late.check(did_not_wait=False)
    np.testing.assert_array_equal(np.concatenate([c.cpu().numpy() for c in clones], axis=1), want)
    assert tx.packets() == 5
    tx.close()


@pytest.mark.parametrize("gap", [903, 0])
def test_two_equal_transmit_calls_do_not_wait(D, gap):
    """after a warm-up of the same two calls, two calls find both staging
    slots free and the carrier table large enough: neither waits"""
    nch, splits = 9, [2, 2]
    bits, decoy = _payload(31 + gap, nch, 4), _payload(32 + gap, nch, 4)
    want = sc.tx_batch_host(bits, gap=gap)
    tx = sc.Transmitter(nch, gap=gap)
    S = torch.cuda.Stream()
    warm = _tx_sequence(tx, S, None, bits, decoy, splits)
    S.synchronize()
    del warm
    tx.reset()
    late, clones, hold = _tx_sequence(tx, S, D, bits, decoy, splits)
    S.synchronize()
    tx.sync()
    late.check(did_not_wait=True)
    np.testing.assert_array_equal(np.concatenate([c.cpu().numpy() for c in clones], axis=1), want)
    tx.close()


def test_transmit_fmt_interleaved_alaw(D):
    """modulate_device_fmt through the context's int16 block and the tile transpose"""
    nch, gap, splits = 9, 903, [1, 3, 1]
    fmt = sc.OUT_ALAW | sc.OUT_INTERLEAVED
    bits, decoy = _payload(41, nch, 5), _payload(42, nch, 5)
    want = sc.output_convert_host(sc.tx_batch_host(bits, gap=gap), fmt)   # [n][nch]
    tx = sc.Transmitter(nch, gap=gap)
    S = torch.cuda.Stream()
    late, clones, hold = _tx_sequence(tx, S, D, bits, decoy, splits, fmt=fmt)
    S.synchronize()
    tx.sync()
    late.check(did_not_wait=False)
    np.testing.assert_array_equal(np.concatenate([c.cpu().numpy() for c in clones], axis=0), want)
    tx.close()


def test_transmit_reset_with_a_call_pending(D):
    nch, gap = 9, 903
    P = sc.TX_PACKET + gap
    bits = _payload(51, nch, 5)          # packet 0 synchronised, 1..2 pending, 3..4 after the reset
    cont = sc.tx_batch_host(bits[:, :3], gap=gap)
    anew = sc.tx_batch_host(bits[:, 3:], gap=gap)
    tx = sc.Transmitter(nch, gap=gap)
    S = torch.cuda.Stream()
    warm = [(torch.from_numpy(bits[:, :2].copy()).cuda(),
             torch.zeros((nch, 2 * P), dtype=torch.int16, device="cuda")) for _ in range(2)]
    for wb, wo in warm:   # both staging slots at 2 packets
        tx.modulate_device(wb, wo, stream=S)
    tx.sync()
    tx.reset()
    o0 = torch.zeros((nch, P), dtype=torch.int16, device="cuda")
    tx.modulate_device(torch.from_numpy(bits[:, :1].copy()).cuda(), o0, stream=S)
    tx.sync()
    pin, db = _pinned(bits[:, 1:3]), torch.from_numpy(_payload(52, nch, 2)).cuda()
    o1 = torch.zeros((nch, 2 * P), dtype=torch.int16, device="cuda")
    o2 = torch.zeros((nch, 2 * P), dtype=torch.int16, device="cuda")
    d2 = torch.from_numpy(bits[:, 3:].copy()).cuda()
    torch.cuda.synchronize()
    late = _Late(S, D)
    late.feed([(db, pin)])
    tx.modulate_device(db, o1, stream=S)
    pending = late.delay.running()
    tx.reset()
    assert tx.packets() == 0
    tx.modulate_device(d2, o2, stream=S)
    S.synchronize()
    tx.sync()
    late.premise()
    assert pending
    np.testing.assert_array_equal(o0.cpu().numpy(), cont[:, :P])
    np.testing.assert_array_equal(o1.cpu().numpy(), cont[:, P:])
    np.testing.assert_array_equal(o2.cpu().numpy(), anew)
    tx.close()


# ------------------------------------------------------------------ G. the stateless device passes
def _pass(D, feeds, run, outputs=None):
    """One stateless pass on S behind the delay.  feeds: (real host array,
    decoy host array) pairs; run(S, *device inputs) -> dict of result tensors
    (outputs: those among them, or other tensors, to overwrite afterwards;
    default every result).  Twice: the first pass, without a delay, is the
    warm-up.  Returns the clones on the host."""
    S = torch.cuda.Stream()

    def once(delay):   # (a function: the warm-up's tensors are released when it returns)
        pins = [_pinned(real) for real, _ in feeds]
        devs = [torch.from_numpy(np.ascontiguousarray(decoy)).cuda() for _, decoy in feeds]
        torch.cuda.synchronize()
        late = _Late(S, delay)
        late.feed(zip(devs, pins))
        res = run(S, *devs)
        clones = late.keep(res)
        late.finish(list(res.values()) if outputs is None else outputs(res))
        S.synchronize()
        late.check(did_not_wait=True)
        return _host(clones)

    once(None)
    return once(D)


NCH_G = 130   # three channel tiles of the conversions, the last one ragged


@pytest.mark.parametrize("fmt", [sc.IN_ULAW | sc.IN_PLANAR, ALAW_I, sc.IN_S16 | sc.IN_PLANAR])
def test_input_convert_device_in_order(D, fmt):
    rng = np.random.default_rng(60 + fmt)
    shape = (sc.FRAME_SIZE, NCH_G) if fmt == ALAW_I else (NCH_G, sc.FRAME_SIZE)
    def block():
        if fmt & 0x0f == sc.IN_S16:
            return rng.integers(-32768, 32768, shape).astype(np.int16)
        return rng.integers(0, 256, shape).astype(np.uint8)
    real, decoy = block(), block()
    got = _pass(D, [(real, decoy)], lambda S, x: {"out": sc.input_convert_device(x, fmt, NCH_G, stream=S)})
    np.testing.assert_array_equal(got["out"], sc.input_convert_host(real, fmt, NCH_G))


def test_output_convert_device_in_order(D):
    """interleaved mu-law into a column range of a wider trunk: the other
    columns keep their contents"""
    fmt = sc.OUT_ULAW | sc.OUT_INTERLEAVED
    n, ld, col = sc.FRAME_SIZE, 160, 7
    rng = np.random.default_rng(70)
    real, decoy = (rng.integers(-32768, 32768, (NCH_G, n)).astype(np.int16) for _ in range(2))

    def run(S, x):
        with torch.cuda.stream(S):
            trunk = torch.full((n, ld), 0x11, dtype=torch.uint8, device="cuda")
        sc.output_convert_device(x, fmt, trunk[:, col:col + NCH_G], stream=S)
        return {"trunk": trunk}

    got = _pass(D, [(real, decoy)], run)
    want = np.full((n, ld), 0x11, np.uint8)
    want[:, col:col + NCH_G] = sc.output_convert_host(real, fmt)
    np.testing.assert_array_equal(got["trunk"], want)


def test_pack_bits_device_in_order(D):
    rng = np.random.default_rng(80)
    real, decoy = (rng.integers(0, 2, (NCH_G, 3, sc.NBITS), dtype=np.uint8) for _ in range(2))
    got = _pass(D, [(real, decoy)], lambda S, b: {"words": sc.pack_bits_device(b, stream=S)})
    np.testing.assert_array_equal(got["words"].view(np.uint64), sc.pack_bits(real))


@pytest.mark.parametrize("order", ORDERS)
def test_compact_device_in_order(D, order):
    nf = 5
    rng = np.random.default_rng(90 + order)
    def dense():
        return [rng.integers(0, 2, (NCH_G, nf, sc.NBITS), dtype=np.uint8),
                rng.integers(0, 2, (NCH_G, nf), dtype=np.uint8),
                rng.integers(-1000, 1000, (NCH_G, nf, 4)).astype(np.int32),
                rng.standard_normal((NCH_G, nf, sc.DATA_SYMBOLS, 2)).astype(np.float32)]
    real, decoy = dense(), dense()
    assert 0 < real[1].sum() < real[1].size and (real[1] != decoy[1]).any()

    def run(S, bits, valid, trace, soft):
        o = sc.compact_device(bits, valid, trace, soft, order=order, stream=S)
        return {k: o[k] for k in ("rec", "trace", "soft", "groups", "count")}

    got = _pass(D, list(zip(real, decoy)), run)
    _rec_same(got, dict(zip(KEYS, real)), order)


@pytest.mark.parametrize("n", [4, 256])
def test_fft_run_device_in_place_in_order(D, n):
    rng = np.random.default_rng(100 + n)
    def block():
        return (rng.standard_normal((37, n)) + 1j * rng.standard_normal((37, n))).astype(np.complex64)
    real, decoy = block(), block()
    plan = sc.FftPlan(n)
    # in place: the result is the fed buffer itself, cloned before it is zeroed
    got = _pass(D, [(real, decoy)], lambda S, x: {"x": plan.run_device(x, out=x, stream=S)}, outputs=lambda res: [])
    plan.close()
    assert got["x"].tobytes() == oracle.cpu_fft(real).tobytes()
