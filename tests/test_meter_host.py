"""The conversion with the level meter in its pass on the host
(include/qpsk_input.h: qpsk_input_convert_level_host, the twin every GPU result
of tests/test_gpu_meter_fused.py is compared with), the size of the device
call's work area, and the refusals that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import singlecarrier_amd as sc
from level_cases import SENT, filled, restate_level
from meter_cases import LOUDEST, as_layout, block, decoded, source, tile_edges

ENCS = [sc.IN_S16, sc.IN_ALAW, sc.IN_ULAW]
LAYOUTS = [sc.IN_PLANAR, sc.IN_INTERLEAVED]


@pytest.mark.parametrize("nch,nf", [(1, 1), (8, 3), (65, 2), (5, 7)])
def test_host_twin_against_numpy(nch, nf):
    """the converted block is the decoded block by the tests' own G.711 tables,
    the levels are numpy's of it"""
    for enc in ENCS:
        x = block(enc, nch, nf, seed=nch * 10 + nf)
        y = decoded(x, enc)
        want = restate_level(y)
        for layout in LAYOUTS:
            out, level = sc.input_convert_level_host(as_layout(x, layout), enc | layout, nch)
            np.testing.assert_array_equal(out, y)
            assert level.tobytes() == want.tobytes(), (enc, layout)
            assert level.tobytes() == sc.level_host(sc.input_convert_host(as_layout(x, layout), enc | layout, nch)).tobytes()


def test_host_twin_on_a_wider_trunk_and_what_it_writes():
    """ld > nch: the columns past nch are loud and are not metered; the outputs
    are written exactly, between sentinels"""
    nch, nf, ld = 5, 2, 9
    L = sc.lib()
    for enc in ENCS:
        x = block(enc, nch, nf, seed=3)
        src = source(x, sc.IN_INTERLEAVED, ld)
        out = filled(nch * nf * sc.FRAME_SIZE + 16, np.int16)
        level = filled(nch * nf + 2, sc.LEVEL_DTYPE)
        assert L.qpsk_input_convert_level_host(enc | sc.IN_INTERLEAVED, src.ctypes.data, ld, nch, nf,
                                               out[8:].ctypes.data, level[1:].ctypes.data, 2) == 0
        y = decoded(x, enc)
        np.testing.assert_array_equal(out[8:-8].reshape(y.shape), y)
        assert level[1:-1].tobytes() == restate_level(y).tobytes()
        for guard in (out[:8], out[-8:], level[:1], level[-1:]):
            assert (guard.view(np.uint8) == SENT).all()


def test_the_cases_hold_what_they_claim():
    """the loudest rows reach 32256 / 32124 and never `clipped`; int16 rows do;
    the tile edges of a frame lie where the tiling puts them"""
    for enc in (sc.IN_ALAW, sc.IN_ULAW):
        lv = restate_level(decoded(block(enc, 8, 7, seed=1), enc))
        assert lv["peak"].max() == LOUDEST[enc] and lv["clipped"].max() == 0
        assert (lv["sumsq"] == 1880 * LOUDEST[enc] ** 2).any()
    assert restate_level(block(sc.IN_S16, 8, 7, seed=1))["clipped"].max() == 1880
    assert tile_edges(0)[:2] == [127, 128] and tile_edges(1)[:2] == [39, 40] and tile_edges(2)[:2] == [79, 80]
    assert tile_edges(3)[:2] == [119, 120] and tile_edges(16)[:2] == [127, 128]   # 16 * 1880 = 235 * 128
    assert (3 * 1880) % 128 == 8   # a frame boundary 8 samples into a tile


def test_work_bytes():
    """0 for planar blocks, for no frames and for refused arguments; for
    interleaved blocks 16 partial levels of 16 bytes a channel-frame, which
    grows with nch and nframes and does not depend on ld"""
    w = sc.input_level_work_bytes
    for enc in ENCS:
        assert w(enc | sc.IN_PLANAR, 8, 4) == 0
        fmt = enc | sc.IN_INTERLEAVED
        assert w(fmt, 8, 0, 8) == 0
        assert w(fmt, 8, 4, 7) == 0 and w(fmt, 0, 4, 8) == 0 and w(fmt, 8, -1, 8) == 0   # refused
        assert w(fmt, 1 << 14, 1 << 14, 1 << 14) == 0                                     # nch * nframes = 2^28
        assert w(fmt, 1, 1, 1) == 256
        assert w(fmt, 8, 4, 8) == w(fmt, 8, 4, 100) == 8 * 4 * 256
        prev = 0
        for nch, nf in ((1, 1), (1, 2), (2, 2), (63, 2), (64, 2), (65, 2), (65, 3), (129, 7), (65536, 32)):
            cur = w(fmt, nch, nf, nch)
            assert cur > prev and cur % 16 == 0
            prev = cur
    assert w(3, 8, 4, 8) == 0 and w(0x23, 8, 4, 8) == 0   # unknown format words


def test_refusals_of_the_host_twin():
    L = sc.lib()
    x = np.zeros(2 * sc.FRAME_SIZE, np.uint8)
    out = filled(2 * sc.FRAME_SIZE, np.int16)
    level = filled(2, sc.LEVEL_DTYPE)
    p, o, lv = x.ctypes.data, out.ctypes.data, level.ctypes.data
    for args in ((3, p, 2, 2, 1, o, lv), (sc.IN_ALAW | sc.IN_INTERLEAVED, p, 1, 2, 1, o, lv),
                 (sc.IN_ALAW, None, 0, 2, 1, o, lv), (sc.IN_ALAW, p, 0, 2, 1, None, lv),
                 (sc.IN_ALAW, p, 0, 2, 1, o, None), (sc.IN_ALAW, p, 0, 0, 1, o, lv), (sc.IN_ALAW, p, 0, 2, -1, o, lv)):
        assert L.qpsk_input_convert_level_host(*args, 1) == sc.QPSK_EINVAL, args
    assert (out.view(np.uint8) == SENT).all() and (level.view(np.uint8) == SENT).all()
    assert L.qpsk_input_convert_level_host(sc.IN_ALAW, None, 0, 2, 0, None, None, 1) == 0   # no frames: nothing to do


def test_refusals_of_the_device_call_that_need_no_gpu():
    """every argument check runs before any HIP call, so on a machine without a
    GPU the refusals are the same: the pointers are never followed"""
    L = sc.lib()
    fmt = sc.IN_ALAW | sc.IN_INTERLEAVED
    need = sc.input_level_work_bytes(fmt, 2, 1, 2)
    src, out, lv, work = 0x10000, 0x20000, 0x30000, 0x40000   # aligned addresses that are nobody's
    call = L.qpsk_input_convert_level_device
    for args in ((fmt, src, 2, 2, 1, out, None, work, need),          # a NULL d_level
                 (fmt, src, 2, 2, 1, out, lv + 4, work, need),        # d_level not 8-byte aligned
                 (fmt, src, 2, 2, 1, out, lv, work, need - 1),        # a short work area
                 (fmt, src, 2, 2, 1, out, lv, None, need),            # no work area where one is needed
                 (fmt, src, 2, 2, 1, out, lv, work + 8, need),        # a work area not 16-byte aligned
                 (sc.IN_ALAW, src, 0, 2, 1, out, lv, work + 8, 0),    # ... also where none is needed
                 (0x23, src, 2, 2, 1, out, lv, work, need),           # a bad format word
                 (fmt, src, 1, 2, 1, out, lv, work, need),            # ld < nch
                 (fmt, None, 2, 2, 1, out, lv, work, need), (fmt, src, 2, 2, 1, None, lv, work, need),
                 (fmt, src, 2, 2, 1, out + 8, lv, work, need),        # d_out not 16-byte aligned
                 (sc.IN_S16 | sc.IN_INTERLEAVED, src + 1, 2, 2, 1, out, lv, work, need)):
        assert call(*args, None) == sc.QPSK_EINVAL, args
    assert call(fmt, None, 2, 2, 0, None, None, None, 0, None) == 0   # no frames: QPSK_OK, nothing to do
    n = C.c_uint32(5)
    # the record calls: a format word they do not know, before anything else is touched
    assert L.qpsk_rx_batch_records_squelch_fmt(None, src, fmt, 2, 1, 1, None, 0, 0, None, None, None, None,
                                               C.addressof(n), None) == sc.QPSK_EINVAL   # no context
    assert n.value == 5
