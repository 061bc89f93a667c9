"""G.711 and timeslot-interleaved input on the GPU (include/qpsk_input.h): the
converter against its host twin, the receive path behind it against the
oracle on the decoded samples, streams, handles and the C example.  Run with
-m gpu."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

import oracle
import singlecarrier_amd as sc
from g711 import TABLES, expand
from rxcheck import assert_same, expected, live_handles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (3, 7), (63, 63), (65, 80), (130, 131), (257, 300)]
ENCS = [sc.IN_S16, sc.IN_ALAW, sc.IN_ULAW]
SENTINEL = 0x5A5A
GUARD = 64   # int16 in front of and behind the output: 128 bytes, so the output stays 16-byte aligned


def _placements(enc):
    """bytes past a 16-byte boundary the source starts at"""
    return (0, 2) if enc == sc.IN_S16 else (0, 1, 3)


def _source(rng, enc, layout, nch, ld, nframes, offset):
    """(numpy block, torch block) of one random source: planar [nch][T] or
    interleaved [T][nch] with rows ld apart, the device copy `offset` bytes
    past a 16-byte boundary"""
    import torch
    T = nframes * sc.FRAME_SIZE
    es = 2 if enc == sc.IN_S16 else 1
    n = (T - 1) * ld + nch if layout == sc.IN_INTERLEAVED else nch * T
    flat = rng.integers(0, 256, n * es, dtype=np.uint8)
    dev = torch.zeros(n * es + 16 + offset, dtype=torch.uint8, device="cuda")
    base = (-dev.data_ptr()) % 16 + offset
    d = dev[base:base + n * es]
    d.copy_(torch.from_numpy(flat))
    assert d.data_ptr() % 16 == offset
    h = flat.view(np.int16) if es == 2 else flat
    d = d.view(torch.int16) if es == 2 else d
    if layout == sc.IN_INTERLEAVED:
        return (np.lib.stride_tricks.as_strided(h, (T, nch), (ld * es, es)),
                torch.as_strided(d, (T, nch), (ld, 1), d.storage_offset()))
    return h.reshape(nch, T), d.view(nch, T)


def _convert_guarded(d, fmt, nch, nframes, stream=None, dec=None):
    """the device conversion into the middle of a sentinel-filled buffer:
    (output, True when nothing around it was touched)"""
    import torch
    n = nch * nframes * sc.FRAME_SIZE
    full = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int16, device="cuda")
    out = full[GUARD:GUARD + n].view(nch, nframes, sc.FRAME_SIZE)
    assert out.data_ptr() % 16 == 0
    if dec is None:
        sc.input_convert_device(d, fmt, nch, out=out, stream=stream)
    else:
        ld = d.stride(0) if (fmt & 0x10) and d.shape[0] > 1 else nch
        s = torch.cuda.current_stream()
        sc._check(sc.lib().qpsk_input_convert_device_dec(fmt, d.data_ptr(), ld, nch, nframes, out.data_ptr(),
                                                         C.c_void_p(s.cuda_stream), dec))
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    full = full.cpu().numpy()
    clean = (full[:GUARD] == SENTINEL).all() and (full[GUARD + n:] == SENTINEL).all()
    return full[GUARD:GUARD + n].reshape(nch, nframes, sc.FRAME_SIZE), bool(clean)


@pytest.mark.parametrize("nframes", [1, 3])
@pytest.mark.parametrize("nch,ld", SHAPES)
def test_converter_equals_the_host_twin(nch, ld, nframes):
    """every format and source placement; one frame is 29 * 64 + 24 samples,
    so the time axis has a ragged last tile too"""
    rng = np.random.default_rng(100 * nch + nframes)
    for enc in ENCS:
        for layout in (sc.IN_PLANAR, sc.IN_INTERLEAVED):
            for offset in _placements(enc):
                fmt = enc | layout
                h, d = _source(rng, enc, layout, nch, ld, nframes, offset)
                want = sc.input_convert_host(h, fmt, nch)
                got, clean = _convert_guarded(d, fmt, nch, nframes)
                what = f"fmt {fmt:#x} nch {nch} ld {ld} frames {nframes} offset {offset}"
                np.testing.assert_array_equal(got, want, err_msg=what)
                assert clean, what + ": wrote outside nch * T"


def test_converter_on_a_stream_of_its_own():
    import torch
    rng = np.random.default_rng(9)
    s = torch.cuda.Stream()
    for fmt in (sc.IN_ALAW | sc.IN_INTERLEAVED, sc.IN_ULAW | sc.IN_PLANAR):
        h, d = _source(rng, fmt & 0x0f, fmt & 0x10, 130, 131, 1, 1)
        torch.cuda.synchronize()
        got, clean = _convert_guarded(d, fmt, 130, 1, stream=s)
        np.testing.assert_array_equal(got, sc.input_convert_host(h, fmt, 130))
        assert clean


@pytest.mark.parametrize("enc,ld,offset,width", [
    (sc.IN_ALAW, 80, 0, 16), (sc.IN_ALAW, 72, 0, 8), (sc.IN_ULAW, 300, 0, 4), (sc.IN_ULAW, 70, 0, 2),
    (sc.IN_ALAW, 80, 8, 8), (sc.IN_ALAW, 80, 3, 1), (sc.IN_ALAW, 131, 0, 1),
    (sc.IN_S16, 80, 0, 16), (sc.IN_S16, 300, 0, 8), (sc.IN_S16, 70, 0, 4), (sc.IN_S16, 131, 0, 2),
    (sc.IN_S16, 80, 2, 2)])
def test_every_load_width_of_the_interleaved_kernel(enc, ld, offset, width):
    """the load width follows the alignment of the block and of its row stride;
    each width is a kernel of its own, and so is each G.711 decoder"""
    rng = np.random.default_rng(ld + offset)
    nch, fmt = 65, enc | sc.IN_INTERLEAVED
    h, d = _source(rng, enc, sc.IN_INTERLEAVED, nch, ld, 1, offset)
    assert sc.lib().qpsk_input_load_width(d.data_ptr(), ld, d.element_size()) == width
    want = sc.input_convert_host(h, fmt, nch)
    for dec in ((0,) if enc == sc.IN_S16 else (0, 1)):
        got, clean = _convert_guarded(d, fmt, nch, 1, dec=dec)
        np.testing.assert_array_equal(got, want, err_msg=f"decoder {dec}")
        assert clean


def test_both_decoders_of_the_planar_kernel():
    rng = np.random.default_rng(21)
    for enc in (sc.IN_ALAW, sc.IN_ULAW):
        for offset in (0, 3):
            h, d = _source(rng, enc, sc.IN_PLANAR, 3, 3, 1, offset)
            for dec in (0, 1):
                got, clean = _convert_guarded(d, enc, 3, 1, dec=dec)
                np.testing.assert_array_equal(got, sc.input_convert_host(h, enc, 3), err_msg=f"decoder {dec}")
                assert clean


# ------------------------------------------------------------------ the kernels' loops
def test_interleaved_kernel_loops_over_more_than_2_to_20_tiles():
    """one channel x 71,400 frames = 134,232,000 samples: 1,048,688 tiles of 128
    samples on a grid capped at 2^20 blocks, so the first 112 blocks take a
    second tile"""
    nch, nframes = 1, 71400
    assert -(-nframes * sc.FRAME_SIZE // 128) == 2**20 + 112
    rng = np.random.default_rng(20)
    fmt = sc.IN_ALAW | sc.IN_INTERLEAVED
    h, d = _source(rng, sc.IN_ALAW, sc.IN_INTERLEAVED, nch, 1, nframes, 0)
    want = sc.input_convert_host(h, fmt, nch)
    got, clean = _convert_guarded(d, fmt, nch, nframes)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, f"{bad.size} samples differ, the first at {int(bad[0])} (tile {int(bad[0]) // 128})"
    assert clean, "wrote outside nch * T"


def test_planar_kernel_loops_over_more_than_2_to_28_groups():
    """one channel x 2,284,700 frames = 4,295,236,000 codes: 2^28 + 16,794 groups
    of 16 on a grid of 2^20 blocks x 256 lanes, so the first 66 blocks take a
    second group, at element indices past 2^32.  Source and expectation repeat a
    block of prime length on the device; the block's samples are the host
    twin's.  Needs about 14 GB of device memory: skipped below 24 GiB free,
    never shrunk (below 2^28 groups the loop does not iterate)."""
    import torch
    nch, nframes, L = 1, 2_284_700, 1_000_003
    T = nframes * sc.FRAME_SIZE
    assert (T + 15) // 16 == 2**28 + 16794
    if torch.cuda.mem_get_info()[0] < 24 * 2**30:
        pytest.skip("needs about 14 GB of device memory")
    # the host twin takes whole frames: 532 frames hold the block's 1,000,003 codes
    codes = np.random.default_rng(28).integers(0, 256, 532 * sc.FRAME_SIZE, dtype=np.uint8)
    samples = sc.input_convert_host(codes[None], sc.IN_ULAW, 1).reshape(-1)[:L]
    src = full = blk = exp = out = flat = None
    try:
        src = torch.from_numpy(codes[:L]).cuda().repeat(-(-T // L))[:T].view(1, T)
        full = torch.full((GUARD + T + GUARD,), SENTINEL, dtype=torch.int16, device="cuda")
        out = full[GUARD:GUARD + T].view(nch, nframes, sc.FRAME_SIZE)
        assert out.data_ptr() % 16 == 0
        sc.input_convert_device(src, sc.IN_ULAW, nch, out=out)
        torch.cuda.synchronize()
        assert bool((full[:GUARD] == SENTINEL).all()) and bool((full[GUARD + T:] == SENTINEL).all()), "wrote outside T"
        blk = torch.from_numpy(samples).cuda()
        flat = out.view(-1)
        step = 2**26
        for lo in range(0, T, step):
            hi = min(lo + step, T)
            exp = blk[torch.arange(lo, hi, device="cuda") % L]
            assert torch.equal(flat[lo:hi], exp), f"samples [{lo}, {hi}) of {T} differ (groups {lo // 16}..)"
    finally:
        del src, full, blk, exp, out, flat
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ the receive path
def _encode(x, enc):
    """every sample to the code of the nearest table value"""
    tab = TABLES[enc]
    order = np.argsort(tab, kind="stable")
    vals = tab[order]
    i = np.clip(np.searchsorted(vals, x), 1, 255)
    i = np.where(np.abs(vals[i - 1] - x) <= np.abs(vals[i] - x), i - 1, i)
    return order[i].astype(np.uint8)


class Case:
    """a synthetic batch as G.711 codes, what the codes decode to (this file's
    tables), and the oracle's receive of that"""

    def __init__(self, enc, nch, nframes, mode=0):
        x = oracle.synth(7, nch, nframes)
        self.enc, self.nch, self.nframes, self.mode = enc, nch, nframes, mode
        self.codes = _encode(x.reshape(nch, -1).astype(np.int64), enc)        # [nch][T]
        self.y = expand(self.codes, enc).reshape(nch, nframes, sc.FRAME_SIZE)
        self.exp = expected(self.y, mode)
        self.bits, self.valid = self.exp["bits"], self.exp["valid"]

    def block(self, layout, ld=None):
        if layout == sc.IN_PLANAR:
            return self.codes
        wide = np.full((self.codes.shape[1], ld), 0xEE, np.uint8)   # the other columns of the trunk
        wide[:, :self.nch] = self.codes.T
        return wide[:, :self.nch]

    def check(self, out):
        assert_same(out, self.exp)


@pytest.fixture(scope="module")
def cases():
    c = {enc: Case(enc, 96, 8) for enc in (sc.IN_ALAW, sc.IN_ULAW)}
    for case in c.values():
        # at least a quarter of the 768 channel-frames valid: the comparison is not empty
        assert case.valid.size == 768 and int(case.valid.sum()) >= 192
    return c


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                                      b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k], err_msg=k)


@pytest.mark.parametrize("layout", [sc.IN_PLANAR, sc.IN_INTERLEAVED])
@pytest.mark.parametrize("enc", [sc.IN_ALAW, sc.IN_ULAW])
def test_demod_fmt_equals_the_oracle_on_the_decoded_samples(cases, enc, layout):
    case = cases[enc]
    rx = sc.Receiver(96)
    out = rx.demod_fmt(case.block(layout, 100), enc | layout, trace=True, soft=True)
    rx.close()
    case.check(out)
    rx = sc.Receiver(96)
    _same(out, rx.demod(case.y, trace=True, soft=True))
    rx.close()


@pytest.mark.parametrize("layout", [sc.IN_PLANAR, sc.IN_INTERLEAVED])
def test_two_calls_equal_one(cases, layout):
    case = cases[sc.IN_ALAW]
    rx = sc.Receiver(96)
    T3 = 3 * sc.FRAME_SIZE
    if layout == sc.IN_PLANAR:
        parts = [np.ascontiguousarray(case.codes[:, :T3]), np.ascontiguousarray(case.codes[:, T3:])]
    else:
        b = case.block(layout, 100)
        parts = [b[:T3], b[T3:]]
    outs = [rx.demod_fmt(p, sc.IN_ALAW | layout, trace=True, soft=True) for p in parts]
    rx.close()
    assert outs[0]["valid"].shape == (96, 3) and outs[1]["valid"].shape == (96, 5)
    case.check({k: np.concatenate([o[k] for o in outs], axis=1) for k in outs[0]})


def test_interleaved_int16_equals_demod_of_the_transpose(cases):
    y = cases[sc.IN_ULAW].y
    wide = np.zeros((8 * sc.FRAME_SIZE, 100), np.int16)
    wide[:, :96] = y.reshape(96, -1).T
    rx = sc.Receiver(96)
    got = rx.demod_fmt(wide[:, :96], sc.IN_S16 | sc.IN_INTERLEAVED, trace=True, soft=True)
    rx.close()
    rx = sc.Receiver(96)
    _same(got, rx.demod(y, trace=True, soft=True))
    # planar int16 is the plain call
    rx.reset()
    _same(got, rx.demod_fmt(y.reshape(96, -1), sc.IN_S16 | sc.IN_PLANAR, trace=True, soft=True))
    rx.close()


@pytest.mark.parametrize("enc,layout,mode", [(sc.IN_ALAW, sc.IN_INTERLEAVED, 0), (sc.IN_ULAW, sc.IN_PLANAR, 0),
                                             (sc.IN_ALAW, sc.IN_INTERLEAVED, sc.MODE_DEC752)])
def test_the_dual_chain_shape(enc, layout, mode):
    """300 channels x 4 frames"""
    case = Case(enc, 300, 4, mode)
    assert int(case.valid.sum()) >= 300
    rx = sc.Receiver(300, mode=mode)
    out = rx.demod_fmt(case.block(layout, 300), enc | layout, trace=True, soft=True)
    rx.close()
    case.check(out)


@pytest.mark.parametrize("enc,layout", [(sc.IN_ALAW, sc.IN_INTERLEAVED), (sc.IN_ULAW, sc.IN_PLANAR),
                                        (sc.IN_S16, sc.IN_INTERLEAVED)])
def test_demod_device_fmt_on_a_torch_stream(cases, enc, layout):
    import torch
    case = cases[sc.IN_ALAW if enc == sc.IN_S16 else enc]
    if enc == sc.IN_S16:
        block = np.ascontiguousarray(case.y.reshape(96, -1).T)
    else:
        block = np.ascontiguousarray(case.block(layout, 96))
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    rx = sc.Receiver(96)
    out = {"bits": torch.zeros((96, 8, sc.NBITS), dtype=torch.uint8, device=dev),
           "valid": torch.zeros((96, 8), dtype=torch.uint8, device=dev),
           "trace": torch.zeros((96, 8, 4), dtype=torch.int32, device=dev),
           "soft": torch.zeros((96, 8, sc.DATA_SYMBOLS, 2), dtype=torch.float32, device=dev)}
    x = torch.from_numpy(block).to(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        # two calls: the context's converted block is reused
        rx.demod_device_fmt(x[:3 * sc.FRAME_SIZE] if layout else x[:, :3 * sc.FRAME_SIZE].contiguous(), enc | layout,
                            out["bits"][:, :3].contiguous(), out["valid"][:, :3].contiguous())
        rx.sync()
        rx.reset()
        rx.demod_device_fmt(x, enc | layout, out["bits"], out["valid"], out["trace"], out["soft"])
    rx.sync()
    case.check({k: v.cpu().numpy() for k, v in out.items()})
    rx.close()


# ------------------------------------------------------------------ streams
def test_a_stream_of_interleaved_alaw_equals_the_batch(cases):
    case = cases[sc.IN_ALAW]
    fmt = sc.IN_ALAW | sc.IN_INTERLEAVED
    st = sc.Stream(96, 4, fmt=fmt)
    with pytest.raises(sc.QpskError) as ei:   # no int16 [nch][frames][1880] input on this stream
        st.acquire()
    assert ei.value.code == sc.QPSK_EINVAL
    T4 = 4 * sc.FRAME_SIZE
    for k in range(2):
        buf = st.acquire_raw()
        assert buf.shape == (T4, 96) and buf.dtype == np.uint8
        assert buf.nbytes == sc.input_bytes(fmt, 96, 4, 96)
        buf[...] = case.codes[:, k * T4:(k + 1) * T4].T
        st.submit()
    got = [st.retrieve() for _ in range(2)]
    st.close()
    case.check({k: np.concatenate([g[i] for g in got], axis=1) for i, k in enumerate(("bits", "valid"))})


def test_a_default_stream_is_unaffected(cases):
    case = cases[sc.IN_ULAW]
    st = sc.Stream(96, 4)
    got = []
    for k in range(2):
        st.acquire()[...] = case.y[:, 4 * k:4 * k + 4]
        st.submit()
    # acquire_raw on a plain stream is the int16 buffer itself
    got = [st.retrieve() for _ in range(2)]
    raw = st.acquire_raw()
    assert raw.shape == (96, 4 * sc.FRAME_SIZE) and raw.dtype == np.int16
    st.close()
    case.check({k: np.concatenate([g[i] for g in got], axis=1) for i, k in enumerate(("bits", "valid"))})


def test_handles_are_back_at_their_base(cases):
    """receivers and streams that went through the format paths (the source
    block and the converted block of the context, a slot's pinned and device
    blocks) leave nothing alive"""
    import torch
    case = cases[sc.IN_ALAW]
    gc.collect()
    base = live_handles()
    rx = sc.Receiver(96)
    rx.demod_fmt(case.codes, sc.IN_ALAW)
    x = torch.from_numpy(np.ascontiguousarray(case.codes.T)).cuda()
    bits = torch.zeros((96, 8, sc.NBITS), dtype=torch.uint8, device="cuda")
    valid = torch.zeros((96, 8), dtype=torch.uint8, device="cuda")
    rx.demod_device_fmt(x, sc.IN_ALAW | sc.IN_INTERLEAVED, bits, valid)
    rx.sync()
    assert live_handles() > base
    rx.close()
    assert live_handles() == base, "Receiver"
    st = sc.Stream(96, 8, nslot=2, fmt=sc.IN_ALAW)
    st.acquire_raw()[...] = case.codes
    st.submit()
    np.testing.assert_array_equal(st.retrieve()[1], case.valid)
    st.close()
    assert live_handles() == base, "Stream"


# ------------------------------------------------------------------ the C example
def test_c_driver_takes_alaw(golden_dir, tmp_path):
    """examples/qpsk_rx_raw -f alaw: the sample capture as A-law codes gives the
    records of the oracle on the decoded capture, one channel and batched"""
    exe = os.path.join(ROOT, "examples", "qpsk_rx_raw")
    frames = sc.read_raw(os.path.join(golden_dir, "preamble_qpsk_8k.raw"))
    codes = _encode(frames.astype(np.int64), sc.IN_ALAW)
    y = expand(codes, sc.IN_ALAW)
    bits, valid, _ = oracle.cpu_rx(y[None])
    want = sc.records(bits[0], valid[0])
    assert len(want) >= 496
    path = tmp_path / "capture.al"
    codes.tofile(path)
    one = tmp_path / "one.bin"
    r = subprocess.run([exe, "-f", "alaw", str(path), str(one)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert one.read_bytes() == want
    pre = tmp_path / "b_"
    r = subprocess.run([exe, "-b", "-f", "alaw", str(path), str(path), "-o", str(pre)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(f"{pre}0.bin", "rb").read() == want and open(f"{pre}1.bin", "rb").read() == want


def test_c_stream_driver_takes_alaw_files_and_a_trunk(cases, tmp_path):
    """examples/qpsk_rx_stream -f alaw: one file of codes per channel, and -i NCH:
    one timeslot-interleaved trunk file; chunks of 3 frames do not divide the 8"""
    exe = os.path.join(ROOT, "examples", "qpsk_rx_stream")
    case = cases[sc.IN_ALAW]
    nch = 3
    want = [sc.records(case.bits[c], case.valid[c]) for c in range(nch)]
    assert sum(len(w) for w in want) >= 496
    paths = []
    for c in range(nch):
        paths.append(str(tmp_path / f"ch{c}.al"))
        case.codes[c].tofile(paths[-1])
    trunk = tmp_path / "trunk.al"
    np.ascontiguousarray(case.codes[:nch].T).tofile(trunk)
    for pre, args in ((tmp_path / "p_", paths), (tmp_path / "t_", ["-i", str(nch), str(trunk)])):
        r = subprocess.run([exe, "-f", "3", "-f", "alaw", *args, "-o", str(pre)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        for c in range(nch):
            assert open(f"{pre}{c}.bin", "rb").read() == want[c], (args[0], c)
