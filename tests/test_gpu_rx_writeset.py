"""Where a receive call's results land (run with -m gpu).

The arithmetic of the receiver is compared with the oracle everywhere else;
here the comparison is of memory.  The input and the four outputs of a call
lie inside one sentinel-filled buffer, each with at least 256 guard bytes on
both sides and each at the minimum alignment the call accepts past a 16-byte
line (bits + 2, soft + 8, valid + 1, trace and in + 0: include/qpsk_input.h
"Pointer rules of the device receive calls", csrc/qpsk_rx_plan.h).  After the
call the whole buffer must equal an image built on the host: the same sentinel
fill with the input and the oracle's bits, valid flags, four trace columns and
soft symbols pasted in, invalid frames' bits and soft symbols zero.  One
equality so covers the guards, the bytes between the arrays, the input (read
only), the place of an output that was not asked for, and every output byte:
no memset stands in front of a call, so the zeros of invalid frames are the
kernels' own.  Every case runs under two fills (0xA5, 0x5A): no expected byte
can hide behind the fill.

A pointer below its alignment is refused with QPSK_EINVAL before anything is
launched or counted; those cases check the refusal, never a misaligned launch.

The expectations come from three oracle runs of one input (one per receiver
mode used) and a few small ones, shared by all cases and read-only.
"""
import functools

import numpy as np
import pytest

import oracle
import rxcheck
import singlecarrier_amd as sc
from plan_check import plan_limits, run_plan_check

pytestmark = pytest.mark.gpu

GUARD = 256
FILLS = (0xA5, 0x5A)
NAMES = ("in", "bits", "valid", "trace", "soft")
# minimum legal start of each array past a 16-byte line
START = {"in": 0, "bits": 2, "valid": 1, "trace": 0, "soft": 8}
# every forced (QPSK_SHAPE, QPSK_WIDTH) pair and pick_shape's own choice
SHAPES = rxcheck.ALL_SHAPES + [(None, None)]
SHAPE_IDS = ["4x2", "2x4d", "1x8w64", "1x8w32", "1x8w16", "picked"]


# ---------------------------------------------------------------- inputs and expectations
@functools.lru_cache(maxsize=None)
def _input(name):
    """int16 [nch][F][1880], read-only.  "noisy": 279 channels x 23 frames at
    5 dB, channel 1 all zero and channel 2 saturated (every case is a prefix
    [:nch, :F] of it: the receiver is causal and channels are independent);
    "other": another draw, for the stale-output case; "zero" (this receiver
    finds every frame of silence valid: 128 matches); "clean" (noiseless);
    "noise": full-scale white noise, whose frames from the third on are all
    invalid (the first two are valid from the initial state, whatever comes)."""
    if name == "noisy":
        x = oracle.synth(4242, 279, 23, 5.0)
        x[1] = 0
        x[2] = np.clip(x[2].astype(np.int32) * 1000, -32768, 32767).astype(np.int16)
    elif name == "other":
        x = oracle.synth(4243, 130, 5, 5.0)
        x[3] = 0
    elif name == "zero":
        x = np.zeros((130, 3, 1880), np.int16)
    elif name == "noise":
        x = np.random.default_rng(4246).integers(-32768, 32768, (130, 6, 1880)).astype(np.int16)
    else:
        assert name == "clean"
        x = oracle.synth(4244, 130, 5, 1000.0)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _oracle(name, mode=sc.MODE_REFERENCE):
    """The oracle's outputs for _input(name) as the arrays a call writes."""
    x = _input(name)
    o = rxcheck.expected(x, mode)
    assert not o["bits"][o["valid"] == 0].any()
    return {"in": x, **o}


def _expect(name, nch, F, mode=sc.MODE_REFERENCE, f0=0):
    """The arrays of the call on _input(name)[:nch, f0:f0 + F] that follows f0 frames."""
    o = _oracle(name, mode)
    return {k: np.ascontiguousarray(o[k][:nch, f0:f0 + F]) for k in NAMES}


def test_inputs_hold_valid_and_invalid_frames():
    v = _oracle("noisy")["valid"]
    assert 0 < v[:257, :5].sum() < v[:257, :5].size and v[:63, :5].any() and v[:, :2].any()
    assert v[1].all()       # the all-zero channel: 128 matches in every frame
    for mode in (sc.MODE_DEC752, sc.MODE_DEC752 | sc.MODE_FFT_HUNT):
        vm = _oracle("noisy", mode)["valid"][:130, :5]
        assert 0 < vm.sum() < vm.size
    assert _oracle("zero")["valid"].all()
    assert not _oracle("noise")["valid"][:, 3:].any()
    c = _oracle("clean")["valid"]
    assert c.sum() > 0.6 * c.size
    a, b = _oracle("noisy")["valid"][:130, :5], _oracle("other")["valid"]
    assert ((a == 1) & (b == 0)).any() and ((a == 0) & (b == 1)).any()


# ---------------------------------------------------------------- the guarded buffer
class Guarded:
    """The five arrays of a call of nch channels x F frames inside one
    sentinel-filled buffer, on the device (torch) or on the host (numpy, at an
    odd byte offset each: host pointers need no alignment)."""

    def __init__(self, nch, F, fill, device=True, x=None):
        self.nch, self.F, self.fill, self.device = nch, F, fill, device
        cf = nch * F
        self.shape = {"in": (nch, F, 1880), "bits": (nch, F, 62), "valid": (nch, F), "trace": (nch, F, 4),
                      "soft": (nch, F, 31, 2)}
        self.dtype = {"in": np.int16, "bits": np.uint8, "valid": np.uint8, "trace": np.int32, "soft": np.float32}
        self.nbytes = {"in": 3760 * cf, "bits": 62 * cf, "valid": cf, "trace": 16 * cf, "soft": 248 * cf}
        self.off, end = {}, 0
        for k in NAMES:
            line = (end + GUARD + 15) // 16 * 16
            self.off[k] = line + (START[k] if device else 1 + 2 * NAMES.index(k))
            end = self.off[k] + self.nbytes[k]
        self.total = end + GUARD
        if device:
            import torch
            self.raw = torch.full((self.total + 16,), fill, dtype=torch.uint8, device="cuda")
            self.base = (-self.raw.data_ptr()) % 16
        else:
            self.raw = np.full(self.total + 16, fill, np.uint8)
            self.base = (-self.raw.ctypes.data) % 16
        self.buf = self.raw[self.base:self.base + self.total]
        for k in NAMES:   # the guards are there, and the arrays start where they should
            assert self.off[k] >= GUARD and self.addr(k) % 16 == self.off[k] % 16
        if x is not None:
            self.put("in", x)

    def addr(self, k, shift=0):
        p = self.buf.data_ptr() if self.device else self.buf.ctypes.data
        return p + self.off[k] + shift

    def put(self, k, a):
        b = np.ascontiguousarray(a, self.dtype[k]).view(np.uint8).reshape(-1)
        assert b.size == self.nbytes[k]
        if self.device:
            import torch
            self.buf[self.off[k]:self.off[k] + b.size].copy_(torch.from_numpy(b.copy()))
        else:
            self.buf[self.off[k]:self.off[k] + b.size] = b

    def view(self, k, shift=0):
        """Array k as a tensor of its type and shape, `shift` bytes further on."""
        import torch
        tt = {"in": torch.int16, "bits": torch.uint8, "valid": torch.uint8, "trace": torch.int32,
              "soft": torch.float32}[k]
        o = self.off[k] + shift
        return self.buf[o:o + self.nbytes[k]].view(tt).view(self.shape[k])

    def image(self, arrays):
        """The expected buffer: the fill with `arrays` (name -> array) pasted in."""
        img = np.full(self.total, self.fill, np.uint8)
        for k, a in arrays.items():
            b = np.ascontiguousarray(a, self.dtype[k]).view(np.uint8).reshape(-1)
            assert b.size == self.nbytes[k], k
            img[self.off[k]:self.off[k] + b.size] = b
        return img

    def bytes(self):
        return self.buf.cpu().numpy() if self.device else np.array(self.buf)

    def check(self, arrays, what=""):
        """The whole buffer against image(arrays); a difference is reported by
        the array or gap it lies in, with its first offsets."""
        got, img = self.bytes(), self.image(arrays)
        if np.array_equal(got, img):
            return
        bad = np.flatnonzero(got != img)
        msg = []
        edges = [(0, "guard before in")]
        for i, k in enumerate(NAMES):
            edges.append((self.off[k], k + ("" if k in arrays else " (not given)")))
            edges.append((self.off[k] + self.nbytes[k], f"guard after {k}"))
        starts = np.array([e[0] for e in edges])
        where = np.searchsorted(starts, bad, side="right") - 1
        for r in np.unique(where):
            b = bad[where == r]
            unit = {"bits": 62, "valid": 1, "trace": 16, "soft": 248, "in": 3760}.get(edges[r][1].split()[0], 1)
            rel = b - starts[r]
            msg.append(f"{edges[r][1]}: {b.size} bytes differ, first at +{rel[:6].tolist()} "
                       f"(rows {np.unique(rel // unit)[:6].tolist()}), got {got[b[:6]].tolist()} "
                       f"want {img[b[:6]].tolist()}")
        raise AssertionError(f"{what} nch={self.nch} F={self.F} fill={self.fill:#x}: " + "; ".join(msg))


def _device_call(rx, g, trace=True, soft=True, shifts=None):
    """demod_device on g's arrays (trace / soft given or NULL; shifts: name ->
    bytes added to that pointer)."""
    s = shifts or {}
    rx.demod_device(g.view("in", s.get("in", 0)), g.view("bits", s.get("bits", 0)), g.view("valid"),
                    g.view("trace", s.get("trace", 0)) if trace else None,
                    g.view("soft", s.get("soft", 0)) if soft else None)


def _given(exp, trace, soft):
    return {k: v for k, v in exp.items() if k in ("in", "bits", "valid") or (k == "trace" and trace)
            or (k == "soft" and soft)}


def _run(nch, F, name="noisy", mode=sc.MODE_REFERENCE, trace=True, soft=True, what="", f0=0):
    """One fresh context per fill: the call into a guarded buffer (after f0
    frames through the plain host call), the whole buffer against the oracle's
    image."""
    exp = _expect(name, nch, F, mode, f0)
    for fill in FILLS:
        g = Guarded(nch, F, fill, x=exp["in"])
        rx = sc.Receiver(nch, mode=mode)
        try:
            if f0:
                rx.demod(np.ascontiguousarray(_input(name)[:nch, :f0]))
            _device_call(rx, g, trace, soft)
            rx.sync()
            assert rx.frames == f0 + F
        finally:
            rx.close()
        g.check(_given(exp, trace, soft), what)
    return exp


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("F", [1, 2, 5])
@pytest.mark.parametrize("nch", [1, 63, 65, 130, 257])
@pytest.mark.parametrize("shape,width", SHAPES, ids=SHAPE_IDS)
def test_every_back_on_ragged_channel_counts(shape, width, nch, F, monkeypatch):
    """Lane backs (4x2, 2x4 dual, 1x8 W = 64) and quad backs (W = 32, 16, and
    what pick_shape takes for these sizes): the lanes and quads past nch store
    nothing; F = 1, 2, 5 ends on either chain of the dual-chain shapes and on
    an odd tail."""
    rxcheck.force_shape(monkeypatch, shape, width)
    _run(nch, F, what=f"{shape}/{width}")


@pytest.mark.parametrize("trace", [False, True], ids=["notrace", "trace"])
@pytest.mark.parametrize("soft", [False, True], ids=["nosoft", "soft"])
@pytest.mark.parametrize("shape,width", [("4x2", None), ("1x8", "16"), ("1x8", "64")], ids=["4x2", "1x8w16", "1x8w64"])
def test_optional_outputs(shape, width, soft, trace, monkeypatch):
    """An output that is not asked for is not written: its place in the buffer
    stays sentinel.  soft without trace runs nowhere else."""
    rxcheck.force_shape(monkeypatch, shape, width)
    _run(130, 5, trace=trace, soft=soft, what=f"{shape}/{width} trace={trace} soft={soft}")


@pytest.mark.parametrize("mode", [sc.MODE_DEC752, sc.MODE_DEC752 | sc.MODE_FFT_HUNT], ids=["dec752", "dec752+fft"])
def test_modes(mode):
    _run(130, 5, mode=mode, what=f"mode {mode}")


def test_headpass(monkeypatch):
    monkeypatch.setenv("QPSK_HEADPASS", "1")
    _run(130, 5, what="headpass")


@pytest.mark.parametrize("shape,width", [("4x2", None), ("1x8", "16")], ids=["lane", "quad"])
def test_force_exact(shape, width, monkeypatch):
    """Every frame and every data job through the exact-division redo paths
    (train<true>, quad_redo_frame's job store, data_steps<true>)."""
    rxcheck.force_shape(monkeypatch, shape, width)
    monkeypatch.setenv("QPSK_FORCE_EXACT", "1")
    _run(130, 5, what=f"force exact {shape}")


@pytest.mark.parametrize("shape,width", [("4x2", None), ("1x8", "16")], ids=["lane", "quad"])
def test_stale_outputs_are_overwritten(shape, width, monkeypatch):
    """A second call, on a fresh context and another input, into the same
    outputs as they were left: rows that were valid and are invalid now come
    out zero, everything equals the oracle's for the second input."""
    rxcheck.force_shape(monkeypatch, shape, width)
    nch, F = 130, 5
    first, second = _expect("noisy", nch, F), _expect("other", nch, F)
    for fill in FILLS:
        g = Guarded(nch, F, fill, x=first["in"])
        for exp in (first, second):
            g.put("in", exp["in"])
            rx = sc.Receiver(nch)
            try:
                _device_call(rx, g)
                rx.sync()
            finally:
                rx.close()
            g.check(exp, "stale")


@pytest.mark.parametrize("name,f0,F", [("zero", 0, 3), ("clean", 0, 5), ("noise", 3, 3)])
@pytest.mark.parametrize("shape,width", [("4x2", None), ("1x8", "16")], ids=["lane", "quad"])
def test_all_valid_mostly_valid_and_all_invalid(shape, width, name, f0, F, monkeypatch):
    """All-zero input: every frame is valid here, so every bits and soft row
    is rx_data_kernel's.  Noiseless input: most are.  White noise from its
    fourth frame on: no frame is valid, every row is the back waves' zeros and
    the data kernel has no job."""
    rxcheck.force_shape(monkeypatch, shape, width)
    _run(130, F, name=name, what=name, f0=f0)


REFUSED = [("bits", 1), ("soft", 4), ("trace", 4), ("trace", 8), ("in", 2)]


@pytest.mark.parametrize("k,shift", REFUSED, ids=[f"{k}+{s}" for k, s in REFUSED])
def test_misaligned_pointers_are_refused(k, shift):
    """Each pointer one element (trace: one and two) past its place: QPSK_EINVAL,
    nothing launched (the buffer is all sentinel but for the input), nothing
    counted; the next call on the context is a first call."""
    import torch
    nch, F = 65, 2
    exp = _expect("noisy", nch, F)
    g = Guarded(nch, F, FILLS[0], x=exp["in"])
    rx = sc.Receiver(nch)
    try:
        with pytest.raises(sc.QpskError) as e:
            _device_call(rx, g, shifts={k: shift})
        assert e.value.code == sc.QPSK_EINVAL
        torch.cuda.synchronize()
        assert rx.frames == 0
        g.check({"in": exp["in"]}, f"refused {k}+{shift}")
        _device_call(rx, g)
        rx.sync()
        assert rx.frames == F
    finally:
        rx.close()
    g.check(exp, f"after refused {k}+{shift}")


def test_misaligned_outputs_are_refused_through_the_format_call():
    """qpsk_rx_batch_device_fmt with planar int16 forwards to the plain call
    and inherits its refusal."""
    import torch
    nch, F = 65, 2
    fmt = sc.IN_S16 | sc.IN_PLANAR
    exp = _expect("noisy", nch, F)
    g = Guarded(nch, F, FILLS[1], x=exp["in"])
    src = g.view("in").view(nch, F * 1880)
    rx = sc.Receiver(nch)
    try:
        for k, shift in (("trace", 8), ("soft", 4), ("bits", 1)):
            with pytest.raises(sc.QpskError) as e:
                rx.demod_device_fmt(src, fmt, g.view("bits", shift if k == "bits" else 0), g.view("valid"),
                                    g.view("trace", shift if k == "trace" else 0),
                                    g.view("soft", shift if k == "soft" else 0))
            assert e.value.code == sc.QPSK_EINVAL
        torch.cuda.synchronize()
        assert rx.frames == 0
        g.check({"in": exp["in"]}, "refused fmt")
        rx.demod_device_fmt(src, fmt, g.view("bits"), g.view("valid"), g.view("trace"), g.view("soft"))
        rx.sync()
        g.check(exp, "after refused fmt")
    finally:
        rx.close()


def test_the_format_call_refuses_in_front_of_its_conversion():
    """Mu-law input: the conversion writes a block the context owns, which it
    allocates on the first such call.  A refused call must not get that far:
    the library's count of live allocations stays (an inherited refusal, behind
    the conversion, would have raised it by the block), and the first accepted
    call raises it.  That call's outputs equal the oracle's for the decoded
    input."""
    import torch
    nch, F = 65, 2
    fmt = sc.IN_ULAW | sc.IN_PLANAR
    codes = np.random.default_rng(4247).integers(0, 256, (nch, F * 1880), dtype=np.uint8)
    x = sc.input_convert_host(codes, fmt, nch)
    exp = rxcheck.expected(x)
    src = torch.from_numpy(codes).cuda()
    g = Guarded(nch, F, FILLS[1])
    rx = sc.Receiver(nch)
    try:
        live = rxcheck.live_handles()
        for k, shift in (("trace", 8), ("soft", 4), ("bits", 1)):
            with pytest.raises(sc.QpskError) as e:
                rx.demod_device_fmt(src, fmt, g.view("bits", shift if k == "bits" else 0), g.view("valid"),
                                    g.view("trace", shift if k == "trace" else 0),
                                    g.view("soft", shift if k == "soft" else 0))
            assert e.value.code == sc.QPSK_EINVAL
            assert rxcheck.live_handles() == live
        torch.cuda.synchronize()
        assert rx.frames == 0
        g.check({}, "refused ulaw")
        rx.demod_device_fmt(src, fmt, g.view("bits"), g.view("valid"), g.view("trace"), g.view("soft"))
        rx.sync()
        assert rxcheck.live_handles() > live and rx.frames == F
        g.check(exp, "after refused ulaw")
    finally:
        rx.close()


def test_the_record_call_refuses_in_front_of_its_buffers():
    """qpsk_rx_batch_records_device with d_in one element off: QPSK_EINVAL
    before the context's record buffers are made (the count of live
    allocations stays) and before anything is counted."""
    nch, F = 65, 2
    exp = _expect("noisy", nch, F)
    g = Guarded(nch, F, FILLS[0], x=exp["in"])
    rx = sc.Receiver(nch)
    try:
        live = rxcheck.live_handles()
        with pytest.raises(sc.QpskError) as e:
            rx.demod_records_device(g.view("in", 2), trace=True, soft=True)
        assert e.value.code == sc.QPSK_EINVAL
        assert rxcheck.live_handles() == live and rx.frames == 0
        o = rx.demod_records_device(g.view("in"), trace=True, soft=True)
        rx.sync()
        assert rxcheck.live_handles() > live and rx.frames == F
        assert int(o["count"].cpu().numpy().view(np.uint32)[0]) == int(exp["valid"].sum())
    finally:
        rx.close()
    g.check({"in": exp["in"]}, "record call")


# ---------------------------------------------------------------- the host call
@pytest.fixture(scope="module")
def limits(tmp_path_factory):
    """(kZeroCopyCF, the largest pinned cf) of csrc/qpsk_rx_plan.h, from a plain
    build (no sanitizer) of the program of tests/plan_check.py."""
    return plan_limits(run_plan_check(tmp_path_factory.mktemp("plan"), sanitize=False))


def _host_call(nch, F, trace=True, soft=True):
    exp = _expect("noisy", nch, F)
    for fill in FILLS:
        g = Guarded(nch, F, fill, device=False, x=exp["in"])
        assert all(g.addr(k) % 2 == 1 for k in NAMES)
        rx = sc.Receiver(nch)
        try:
            rc = sc.lib().qpsk_rx_batch(rx._h, g.addr("in"), F, g.addr("bits"), g.addr("valid"),
                                        g.addr("trace") if trace else None, g.addr("soft") if soft else None)
            assert rc == 0 and rx.frames == F
        finally:
            rx.close()
        g.check(_given(exp, trace, soft), f"host call trace={trace} soft={soft}")


@pytest.mark.parametrize("nch,F,path", [(8, 8, "zero-copy"), (13, 5, "pinned"), (97, 23, "pinned"),
                                        (279, 8, "pageable")], ids=["cf64", "cf65", "cf2231", "cf2232"])
def test_host_call_at_the_staging_limits(nch, F, path, limits):
    """qpsk_rx_batch into guarded host arrays at odd addresses: the last
    zero-copy size and the first staged one, the last pinned size and the
    first pageable one.  (The kernels of a host call write into the context's
    staging block, which is not sentinel: these cases pin the copies out of
    it, the device cases above pin the kernels.)"""
    zero_copy, pinned = limits
    cf = nch * F
    assert path == ("zero-copy" if cf <= zero_copy else "pinned" if cf <= pinned else "pageable")
    assert cf in (zero_copy, zero_copy + 1, pinned, pinned + 1)
    _host_call(nch, F)


@pytest.mark.parametrize("trace", [False, True], ids=["notrace", "trace"])
@pytest.mark.parametrize("soft", [False, True], ids=["nosoft", "soft"])
def test_host_call_optional_outputs(soft, trace, limits):
    assert 13 * 5 == limits[0] + 1
    _host_call(13, 5, trace, soft)
