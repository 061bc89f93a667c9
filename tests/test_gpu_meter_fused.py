"""The level meter inside the input conversion, and the squelched record calls
and record streams for every input format, on the GPU (include/qpsk_input.h,
include/qpsk_level.h) against the host twins and the oracle on the decoded
samples; cases of tests/meter_cases.py.  Everything is integer arithmetic:
every comparison is for equality.  Run with -m gpu."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

import gpu_delay
import singlecarrier_amd as sc
from level_cases import MIN_SUMSQ, SENT, squelched_records
from meter_cases import N, as_layout, block, decoded, format_case, silence_format_case, source
from rxcheck import live_handles

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = [sc.REC_BY_CHANNEL, sc.REC_BY_FRAME]
IL, PL = sc.IN_INTERLEAVED, sc.IN_PLANAR
FORMATS = [sc.IN_ALAW | PL, sc.IN_ULAW | IL, sc.IN_S16 | IL]   # of the record calls
GUARD = 64        # bytes of sentinel on either side of every output
DEC_DEFAULT = -1


def _place(flat: np.ndarray, offset: int):
    """a flat numpy source on the device, `offset` bytes past a 16-byte boundary"""
    raw = flat.view(np.uint8)
    dev = torch.zeros(raw.size + 32 + offset, dtype=torch.uint8, device="cuda")
    base = (-dev.data_ptr()) % 16 + offset
    d = dev[base:base + raw.size]
    d.copy_(torch.from_numpy(raw))
    assert d.data_ptr() % 16 == offset % 16
    return d


def _sentinel(nbytes: int):
    """(whole buffer, the nbytes in its middle, 16-byte aligned) filled with the sentinel"""
    whole = torch.full((GUARD + nbytes + GUARD + 16,), SENT, dtype=torch.uint8, device="cuda")
    base = (-whole.data_ptr()) % 16 + GUARD
    assert (whole.data_ptr() + base) % 16 == 0
    return whole, whole[base:base + nbytes]


def _fused(d, fmt, ld, nch, nf, dec=DEC_DEFAULT, cap=0):
    """the fused call into sentinel-filled buffers: (the whole output buffer as
    bytes, the levels, True when the guards of the levels and of the work area
    are intact)"""
    n = nch * nf * N
    wo, out = _sentinel(2 * n)
    wl, lv = _sentinel(16 * nch * nf)
    need = sc.input_level_work_bytes(fmt, nch, nf, ld)
    ww, work = _sentinel(need)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sc._check(sc.lib().qpsk_input_convert_level_device_grid(fmt, d.data_ptr(), ld, nch, nf, out.data_ptr(),
                                                           lv.data_ptr(), work.data_ptr() if need else None, need, s,
                                                           dec, cap))
    torch.cuda.synchronize()
    clean = True
    for whole, body in ((wl, lv), (ww, work)):
        a = body.data_ptr() - whole.data_ptr()
        g = torch.cat([whole[:a], whole[a + body.numel():]])
        clean = clean and bool((g == SENT).all())
    level = lv.cpu().numpy().view(sc.LEVEL_DTYPE).reshape(nch, nf)
    return wo.cpu().numpy(), level, clean


def _plain(d, fmt, ld, nch, nf, dec=DEC_DEFAULT):
    """qpsk_input_convert_device into a buffer like _fused's: the whole buffer as bytes"""
    wo, out = _sentinel(2 * nch * nf * N)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sc._check(sc.lib().qpsk_input_convert_device_dec(fmt, d.data_ptr(), ld, nch, nf, out.data_ptr(), s, dec))
    torch.cuda.synchronize()
    return wo.cpu().numpy(), out.cpu().numpy().view(np.int16).reshape(nch, nf, N)


def _check_fused(x, enc, layout, ld, offset, what, dec=DEC_DEFAULT, caps=(0,)):
    """the fused pass on block x: d_out is the plain conversion's whole buffer,
    the levels are level_host of it, written once into pre-filled memory"""
    nch, nf, _ = x.shape
    fmt = enc | layout
    d = _place(source(x, layout, ld), offset)
    want_buf, want = _plain(d, fmt, ld, nch, nf, dec)
    np.testing.assert_array_equal(want, decoded(x, enc), err_msg=what)
    level = sc.level_host(want)
    for cap in caps:
        buf, got, clean = _fused(d, fmt, ld, nch, nf, dec, cap)
        assert buf.tobytes() == want_buf.tobytes(), f"{what} cap {cap}: d_out differs from the plain conversion's"
        bad = np.flatnonzero(got.reshape(-1) != level.reshape(-1))
        assert bad.size == 0, f"{what} cap {cap}: {bad.size} levels differ, the first at row {int(bad[0])}: " \
                              f"{got.reshape(-1)[bad[0]]} for {level.reshape(-1)[bad[0]]}"
        assert clean, f"{what} cap {cap}: wrote outside d_level or the work area"


# ------------------------------------------------------------------ 1. the fused pass equals the twins
@pytest.mark.parametrize("nf", [1, 2, 3, 7])
@pytest.mark.parametrize("nch", [1, 8, 63, 64, 65, 129])
def test_fused_pass_equals_the_twins(nch, nf):
    """frame boundaries at offsets 88, 48 and 8 of a 128-sample tile, and in the
    middle of a planar group of 16 codes on odd rows"""
    for enc in (sc.IN_S16, sc.IN_ALAW, sc.IN_ULAW):
        x = block(enc, nch, nf, seed=100 * nch + nf)
        for ld in (nch, nch + 1, nch + 64):
            _check_fused(x, enc, IL, ld, 0, f"enc {enc} interleaved {nch} x {nf} ld {ld}")
        for offset in ((0,) if enc == sc.IN_S16 else (0, 5)):
            _check_fused(x, enc, PL, nch, offset, f"enc {enc} planar {nch} x {nf} offset {offset}")


@pytest.mark.parametrize("enc,ld,offset,width", [
    (sc.IN_ALAW, 80, 0, 16), (sc.IN_ALAW, 72, 0, 8), (sc.IN_ULAW, 300, 0, 4), (sc.IN_ULAW, 70, 0, 2),
    (sc.IN_ALAW, 80, 8, 8), (sc.IN_ALAW, 80, 3, 1), (sc.IN_ALAW, 131, 0, 1),
    (sc.IN_S16, 80, 0, 16), (sc.IN_S16, 300, 0, 8), (sc.IN_S16, 70, 0, 4), (sc.IN_S16, 131, 0, 2),
    (sc.IN_S16, 80, 2, 2)])
def test_every_load_width_of_the_fused_interleaved_kernel(enc, ld, offset, width):
    """each load width is a kernel of its own, and so is each G.711 decoder"""
    nch, nf = 65, 2
    x = block(enc, nch, nf, seed=ld + offset)
    d = _place(source(x, IL, ld), offset)
    assert sc.lib().qpsk_input_load_width(d.data_ptr(), ld, 2 if enc == sc.IN_S16 else 1) == width
    for dec in ((0,) if enc == sc.IN_S16 else (0, 1)):
        _check_fused(x, enc, IL, ld, offset, f"enc {enc} ld {ld} offset {offset} decoder {dec}", dec=dec)


@pytest.mark.parametrize("enc", [sc.IN_ALAW, sc.IN_ULAW])
def test_every_source_offset_of_the_fused_planar_kernel(enc):
    """a wave reads a row as aligned 8-byte words shifted by the source's byte
    offset: every offset in 16 bytes, both decoders"""
    x = block(enc, 5, 3, seed=enc)
    for offset in range(16):
        for dec in (0, 1):
            _check_fused(x, enc, PL, 5, offset, f"enc {enc} offset {offset} decoder {dec}", dec=dec)


# ------------------------------------------------------------------ 2. several tiles per block
def test_several_tiles_per_block():
    """a grid capped at 1 and at 3 workgroups: each takes several tiles (65 x 3
    interleaved: 2 x 45 tiles) or several groups of rows (planar 5 x 3: 4 groups
    of 4 rows), and the accumulators start anew each time"""
    for enc in (sc.IN_S16, sc.IN_ALAW, sc.IN_ULAW):
        x = block(enc, 65, 3, seed=7)
        _check_fused(x, enc, IL, 65, 0, f"enc {enc} interleaved 65 x 3", caps=(0, 1, 3))
    for enc in (sc.IN_ALAW, sc.IN_ULAW):
        x = block(enc, 5, 3, seed=8)
        _check_fused(x, enc, PL, 5, 3, f"enc {enc} planar 5 x 3", caps=(0, 1, 3))


def test_python_wrapper_and_planar_int16():
    """input_convert_level_device; planar int16 has no conversion pass (a copy
    and the meter's own kernel) behind the same entry point"""
    for fmt, nch in ((sc.IN_ULAW | IL, 9), (sc.IN_ALAW | PL, 3), (sc.IN_S16 | PL, 6)):
        x = block(fmt & 0x0f, nch, 2, seed=fmt)
        h = as_layout(x, fmt & 0x10)
        out, level = sc.input_convert_level_device(torch.from_numpy(h).cuda(), fmt, nch)
        torch.cuda.synchronize()
        want, lv = sc.input_convert_level_host(h, fmt, nch)
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        assert sc.level_from_tensor(level).tobytes() == lv.tobytes()
    _check_fused(block(sc.IN_S16, 6, 2, seed=1), sc.IN_S16, PL, 6, 0, "planar int16")


# ------------------------------------------------------------------ 3. the record calls
def _same(got, exp):
    assert got["count"] == exp["count"]
    np.testing.assert_array_equal(got["groups"], exp["groups"])
    assert got["rec"].tobytes() == exp["rec"].tobytes()
    np.testing.assert_array_equal(got["trace"], exp["trace"])
    assert got["soft"].tobytes() == exp["soft"].tobytes()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_demod_records_squelch_fmt(fmt, order):
    codes, y, d, level = format_case(fmt & 0x0f, 0)
    nch, nf = d["valid"].shape
    h = as_layout(codes, fmt & 0x10)
    plain = int((d["valid"] != 0).sum())
    whole, _ = squelched_records(d, level, None, MIN_SUMSQ, order)
    count = whole["count"]
    assert 5 < count < plain   # the squelch drops some of the frames the receiver calls valid
    for cap in (None, count - 5):
        exp, last = squelched_records(d, level, None, MIN_SUMSQ, order, cap)
        rx = sc.Receiver(nch)
        got = rx.demod_records_squelch_fmt(h, fmt, MIN_SUMSQ, order=order, cap=cap, trace=True, soft=True)
        assert rx.frames == nf
        rx.close()
        assert len(got["rec"]) == (count if cap is None else cap)
        _same(got, exp)
        assert got["level"].tobytes() == level.tobytes()
        assert got["prev"].tobytes() == last.tobytes() == level[:, -1].tobytes()
    # the twins of the level: the host conversion with the meter
    assert sc.input_convert_level_host(h, fmt, nch)[1].tobytes() == level.tobytes()


@pytest.mark.parametrize("mode", [sc.MODE_REFERENCE, sc.MODE_DEC752, sc.MODE_REFERENCE | sc.MODE_FFT_HUNT,
                                  sc.MODE_DEC752 | sc.MODE_FFT_HUNT])
def test_demod_records_squelch_fmt_in_every_mode(mode):
    fmt = sc.IN_ULAW | IL
    codes, y, d, level = format_case(sc.IN_ULAW, mode)
    exp, last = squelched_records(d, level, None, MIN_SUMSQ, sc.REC_BY_FRAME)
    rx = sc.Receiver(8, mode=mode)
    got = rx.demod_records_squelch_fmt(as_layout(codes, IL), fmt, MIN_SUMSQ, order=sc.REC_BY_FRAME, trace=True, soft=True)
    rx.close()
    _same(got, exp)
    assert got["level"].tobytes() == level.tobytes() and got["prev"].tobytes() == last.tobytes()


@pytest.mark.parametrize("fmt", FORMATS)
def test_split_calls_carry_prev(fmt):
    """1 + 3 + 4 frames with prev carried equal one call"""
    order = sc.REC_BY_CHANNEL
    codes, y, d, level = format_case(fmt & 0x0f, 0)
    whole, _ = squelched_records(d, level, None, MIN_SUMSQ, order)
    rx = sc.Receiver(8)
    parts, prev = [], None
    for a, e in ((0, 1), (1, 4), (4, 8)):
        g = rx.demod_records_squelch_fmt(as_layout(np.ascontiguousarray(codes[:, a:e]), fmt & 0x10), fmt, MIN_SUMSQ,
                                         prev=prev, order=order, trace=True, soft=True)
        prev = g["prev"]
        assert prev.tobytes() == level[:, e - 1].tobytes()
        assert g["level"].tobytes() == np.ascontiguousarray(level[:, a:e]).tobytes()
        g["rec"] = g["rec"].copy()
        g["rec"]["frame"] += a
        parts.append(g)
    rx.close()
    rec = np.concatenate([g["rec"] for g in parts])
    tr, so = np.concatenate([g["trace"] for g in parts]), np.concatenate([g["soft"] for g in parts])
    k = np.lexsort((rec["frame"], rec["channel"]))   # a channel's frames of the three calls side by side
    assert sum(g["count"] for g in parts) == whole["count"]
    assert rec[k].tobytes() == whole["rec"].tobytes()
    np.testing.assert_array_equal(tr[k], whole["trace"])
    assert so[k].tobytes() == whole["soft"].tobytes()


@pytest.mark.parametrize("fmt", FORMATS)
def test_silence_gives_no_record(fmt):
    """the quietest code in every sample: sumsq 0 for mu-law and int16, where
    min_sumsq = 1 squelches every frame; A-law has no zero (a frame of +8 has
    sumsq 1880 * 64), so its gate is the smallest value above that"""
    enc = fmt & 0x0f
    codes, y, d = silence_format_case(enc)
    idle = 0 if enc != sc.IN_ALAW else 1880 * 64
    assert int(sc.level_host(y)["sumsq"].max()) == idle and (d["valid"] != 0).any()
    rx = sc.Receiver(2)
    got = rx.demod_records_squelch_fmt(as_layout(codes, fmt & 0x10), fmt, idle + 1)
    assert got["count"] == 0 and len(got["rec"]) == 0 and not got["groups"].any()
    assert (got["level"]["sumsq"] == idle).all()
    rx.reset()
    got = rx.demod_records_squelch_fmt(as_layout(codes, fmt & 0x10), fmt, idle)   # at the level itself: kept
    rx.close()
    assert got["count"] == int((d["valid"] != 0).sum())


def _device_call(rx, dx, fmt, prev, order, S):
    o = rx.demod_records_squelch_device_fmt(dx, fmt, MIN_SUMSQ, prev=prev, order=order, trace=True, soft=True,
                                            stream=S)
    with torch.cuda.stream(S):
        c = {k: v.clone() for k, v in o.items()}
        dx.zero_()   # behind the clones: work that ran late computes from, or leaves, something else
        for k, v in o.items():
            if k != "prev":
                v.view(torch.uint8).fill_(SENT)
    return c


@pytest.mark.parametrize("fmt", [sc.IN_ALAW | IL, sc.IN_ULAW | PL])
def test_device_form_behind_a_delay(fmt):
    """on a caller's stream behind a delay kernel, the input copied in late and
    overwritten afterwards, prev carried on the device: nothing waits for the
    stream, and everything runs in its order"""
    order, enc, layout = sc.REC_BY_FRAME, fmt & 0x0f, fmt & 0x10
    codes, y, d, level = format_case(enc, 0)
    decoy = block(enc, 8, 8, seed=5)   # what the device buffers hold before the late copy
    cuts = ((0, 3), (3, 8))
    wants = [squelched_records({k: np.ascontiguousarray(v[:, a:e]) for k, v in d.items()},
                               np.ascontiguousarray(level[:, a:e]), None if a == 0 else level[:, a - 1].copy(),
                               MIN_SUMSQ, order)[0] for a, e in cuts]
    S = torch.cuda.Stream()
    rx = sc.Receiver(8)
    pins = [torch.from_numpy(as_layout(np.ascontiguousarray(codes[:, a:e]), layout)).pin_memory() for a, e in cuts]
    D = 100.0
    clones = running = delay = None
    for delay_ms in (None, D):   # the first pass is the warm-up: the delayed one grows and allocates nothing
        devs = [torch.from_numpy(as_layout(np.ascontiguousarray(decoy[:, a:e]), layout)).cuda() for a, e in cuts]
        with torch.cuda.stream(S):
            prev = torch.zeros((8, 2), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        delay = gpu_delay.put(S, delay_ms) if delay_ms else None
        with torch.cuda.stream(S):
            for dev, pin in zip(devs, pins):   # the input arrives late, behind the delay
                dev.copy_(pin, non_blocking=True)
        clones = [_device_call(rx, dx, fmt, prev, order, S) for dx in devs]
        running = delay.running() if delay else None
        S.synchronize()
        rx.sync()
        if delay is None:
            rx.reset()
            del clones, devs
    assert delay.ms() >= 0.9 * D
    assert running, "the delay had ended when the last enqueue returned: a call waited for the stream"
    rx.close()
    for c, want, (a, e) in zip(clones, wants, cuts):
        count = int(c["count"].cpu().numpy().view(np.uint32)[0])
        got = {"count": count, "groups": c["groups"].cpu().numpy().view(np.uint32),
               "rec": sc.rec_from_tensor(c["rec"], count), "trace": c["trace"][:count].cpu().numpy(),
               "soft": c["soft"][:count].cpu().numpy()}
        _same(got, want)
        assert sc.level_from_tensor(c["level"]).tobytes() == np.ascontiguousarray(level[:, a:e]).tobytes()
        assert sc.level_from_tensor(c["prev"]).tobytes() == level[:, e - 1].tobytes()


# ------------------------------------------------------------------ 4. streams
def _run_stream(st, src, nf, chunk, levels):
    """all chunks of src ([nch][T] or [T][nch]) through st: the records with the
    chunk's first frame added, and the levels"""
    inter = bool(st.fmt & 0x10)
    recs, lvs, k = [], [], 0
    for a in list(range(0, nf, chunk)) + [None] * st.nslot:
        if st.pending == st.nslot or (a is None and st.pending):
            g = st.retrieve_records(levels=levels)
            g["rec"]["frame"] += k * chunk
            recs.append(g)
            if levels:
                lvs.append(g["level"])
            k += 1
        if a is not None:
            buf = st.acquire_raw()
            buf[...] = src[a * N:(a + chunk) * N] if inter else src[:, a * N:(a + chunk) * N]
            st.submit()
    assert k == nf // chunk and st.pending == 0
    return recs, (np.concatenate(lvs, axis=1) if levels else None)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", [sc.IN_ALAW | IL, sc.IN_S16 | PL])
def test_squelch_stream(fmt, order):
    """8 ch x 8 frames as chunks of 2 frames in 3 slots: the stream carries the
    levels from chunk to chunk, from zero"""
    codes, y, d, level = format_case(fmt & 0x0f, 0)
    whole, _ = squelched_records(d, level, None, MIN_SUMSQ, order)
    src = as_layout(codes, fmt & 0x10)
    gc.collect()
    base = live_handles()
    st = sc.Stream(8, 2, nslot=3, fmt=fmt, records=True, order=order, min_sumsq=MIN_SUMSQ)
    assert live_handles() > base
    recs, lv = _run_stream(st, src, 8, 2, levels=True)
    # the dense retrieve is not this stream's
    st.acquire_raw()[...] = src[:2 * N] if fmt & 0x10 else src[:, :2 * N]
    st.submit()
    b, v = C.c_void_p(), C.c_void_p()
    assert sc.lib().qpsk_stream_retrieve(st._h, C.byref(b), C.byref(v)) == sc.QPSK_EINVAL
    assert st.retrieve_records()["count"] >= 0   # the plain record retrieve works on it as on any record stream
    st.close()
    assert live_handles() == base
    assert lv.tobytes() == level.tobytes()
    rec = np.concatenate([g["rec"] for g in recs])
    assert sum(g["count"] for g in recs) == whole["count"] == len(rec)
    if order == sc.REC_BY_CHANNEL:   # a channel's frames of all chunks side by side
        rec = rec[np.lexsort((rec["frame"], rec["channel"]))]
    assert rec.tobytes() == whole["rec"].tobytes()
    for g in recs:   # each chunk's groups are its own
        np.testing.assert_array_equal(np.diff(g["groups"].astype(np.int64)).sum(), g["count"])


def test_a_plain_record_stream_is_unaffected():
    """a record stream without squelch gives what the record call gives, and
    has no levels to retrieve"""
    fmt = sc.IN_ALAW | IL
    codes, y, d, level = format_case(sc.IN_ALAW, 0)
    want = sc.compact_host(d["bits"], d["valid"], order=sc.REC_BY_FRAME)
    st = sc.Stream(8, 2, nslot=3, fmt=fmt, records=True, order=sc.REC_BY_FRAME)
    recs, _ = _run_stream(st, as_layout(codes, IL), 8, 2, levels=False)
    st.acquire_raw()[...] = as_layout(codes, IL)[:2 * N]
    st.submit()
    with pytest.raises(sc.QpskError) as ei:
        st.retrieve_records(levels=True)
    assert ei.value.code == sc.QPSK_EINVAL
    st.close()
    rec = np.concatenate([g["rec"] for g in recs])
    assert rec.tobytes() == want["rec"].tobytes() and len(rec) > whole_count(d, level)


def whole_count(d, level):
    return squelched_records(d, level, None, MIN_SUMSQ, sc.REC_BY_FRAME)[0]["count"]


# ------------------------------------------------------------------ 5. refusals launch nothing
def test_refusals_launch_nothing():
    L = sc.lib()
    nch, nf, fmt = 3, 1, sc.IN_ALAW | IL
    x = block(sc.IN_ALAW, nch, nf, seed=2)
    d = _place(source(x, IL, nch), 0)
    need = sc.input_level_work_bytes(fmt, nch, nf, nch)
    wo, out = _sentinel(2 * nch * nf * N)
    wl, lv = _sentinel(16 * nch * nf)
    ww, work = _sentinel(need)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, o, l, w = d.data_ptr(), out.data_ptr(), lv.data_ptr(), work.data_ptr()
    gc.collect()
    base = live_handles()
    for args in ((fmt, p, nch, nch, nf, o, l + 4, w, need), (fmt, p, nch, nch, nf, o, l, w + 8, need),
                 (fmt, p, nch, nch, nf, o, l, w, need - 1), (fmt, p, nch, nch, nf, o, l, None, need),
                 (0x23, p, nch, nch, nf, o, l, w, need), (3 | IL, p, nch, nch, nf, o, l, w, need),
                 (fmt, p, nch, nch, nf, o, None, w, need), (fmt, p, nch - 1, nch, nf, o, l, w, need),
                 (fmt, p, nch, nch, nf, o + 8, l, w, need), (sc.IN_ALAW | PL, p, 0, nch, nf, o, l, w + 8, 0)):
        assert L.qpsk_input_convert_level_device(*args, s) == sc.QPSK_EINVAL, args
    assert L.qpsk_input_convert_level_device_grid(fmt, p, nch, nch, nf, o, l, w, need, s, 2, 0) == sc.QPSK_EINVAL
    assert L.qpsk_input_convert_level_device(fmt, None, nch, nch, 0, None, None, None, 0, s) == 0   # no frames
    torch.cuda.synchronize()
    assert live_handles() == base
    for whole in (wo, wl, ww):
        assert bool((whole == SENT).all())
    # the record calls: nothing is received when an argument is refused
    rx = sc.Receiver(nch)
    cnt = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    lvl = torch.zeros((nch + 1, 2), dtype=torch.int64, device="cuda")
    dx = torch.zeros((nf * N, nch), dtype=torch.int16, device="cuda")
    call = L.qpsk_rx_batch_records_squelch_device_fmt
    for d_in, f, ld, prev, level in ((p, 0x23, nch, None, None), (p, fmt, nch - 1, None, None),
                                     (None, fmt, nch, None, None), (p, fmt, nch, lvl.data_ptr() + 4, None),
                                     (p, fmt, nch, None, lvl.data_ptr() + 4),
                                     (dx.data_ptr() + 1, sc.IN_S16 | IL, nch, None, None)):
        assert call(rx._h, d_in, f, ld, nf, 1, prev, 0, 0, None, None, None, None, cnt.data_ptr(), level,
                    s) == sc.QPSK_EINVAL, (d_in, f, ld)
    n = C.c_uint32(5)
    h = source(x, IL, nch)
    host = L.qpsk_rx_batch_records_squelch_fmt
    assert host(rx._h, h.ctypes.data, 0x23, nch, nf, 1, None, 0, 0, None, None, None, None, C.addressof(n),
                None) == sc.QPSK_EINVAL
    assert host(rx._h, None, fmt, nch, nf, 1, None, 0, 0, None, None, None, None, C.addressof(n),
                None) == sc.QPSK_EINVAL
    torch.cuda.synchronize()
    assert rx.frames == 0 and int(cnt.cpu()[0]) == 77 and n.value == 5
    # a call of no frames is fine: an empty list, prev as it was
    got = rx.demod_records_squelch_fmt(np.zeros((0, nch), np.uint8), fmt, 5, prev=sc.level_host(decoded(x, 1))[:, 0])
    assert got["count"] == 0 and got["level"].shape == (nch, 0)
    assert got["prev"].tobytes() == sc.level_host(decoded(x, 1))[:, 0].tobytes()
    rx.close()
    # a stream: a format word or an order it does not know, and no handle is left
    err = C.c_int(0)
    for f, order in ((0x23, 0), (fmt, 2)):
        assert not L.qpsk_stream_create_records_squelch(0, nch, 2, 3, 0, f, order, 6, 1, C.byref(err))
        assert err.value == sc.QPSK_EINVAL
    assert live_handles() == base


# ------------------------------------------------------------------ 6. the examples
def _exe(name):
    exe = os.path.join(ROOT, "examples", name)
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.dirname(exe)], check=True)
    return exe


def test_example_raw_squelches_g711_files(tmp_path):
    """qpsk_rx_raw -b -f alaw -q DBFS: the files it gave when it expanded the
    codes on the host, which is what the host twins give"""
    codes, y, d, level = format_case(sc.IN_ALAW, 0)
    nch = 3
    paths = []
    for c in range(nch):
        codes[c].tofile(tmp_path / f"ch{c}.al")
        paths.append(str(tmp_path / f"ch{c}.al"))
    dd = {k: np.ascontiguousarray(v[:nch]) for k, v in d.items()}
    db = -50.0
    x = sc.input_convert_host(as_layout(np.ascontiguousarray(codes[:nch]), PL), sc.IN_ALAW, nch)   # the parent's logic
    s = sc.squelch_host(sc.level_host(x), dd["valid"], sc.sumsq_of_dbfs(db))
    assert 0 < s["valid"].sum() < (dd["valid"] != 0).sum()
    out = str(tmp_path / "q")
    r = subprocess.run([_exe("qpsk_rx_raw"), "-b", "-f", "alaw", "-q", str(db), *paths, "-o", out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for c in range(nch):
        assert open(f"{out}{c}.bin", "rb").read() == sc.records(dd["bits"][c], s["valid"][c]), c


def test_example_stream_squelch_option(tmp_path):
    """qpsk_rx_stream -i NCH -f alaw -p FILE -q DBFS: exactly the records of
    demod_records_squelch_fmt in by-frame order"""
    codes, y, d, level = format_case(sc.IN_ALAW, 0)
    nch, nf = 8, 8
    trunk = as_layout(codes, IL)
    trunk.tofile(tmp_path / "trunk.al")
    db = -50.0
    rx = sc.Receiver(nch)
    want = rx.demod_records_squelch_fmt(trunk, sc.IN_ALAW | IL, sc.sumsq_of_dbfs(db), order=sc.REC_BY_FRAME)
    rx.close()
    assert 0 < want["count"] < int((d["valid"] != 0).sum())
    for extra, ok in ((["-q", str(db)], True), ([], False)):
        out = str(tmp_path / ("q.rec" if ok else "p.rec"))
        r = subprocess.run([_exe("qpsk_rx_stream"), "-f", "2", "-f", "alaw", *extra, "-i", str(nch),
                            str(tmp_path / "trunk.al"), "-p", out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(out, sc.REC_DTYPE)
        assert (got.tobytes() == want["rec"].tobytes()) == ok
    # -q without -p is a usage error
    r = subprocess.run([_exe("qpsk_rx_stream"), "-q", "-50", "-i", "8", str(tmp_path / "trunk.al"), "-o",
                        str(tmp_path / "x")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
