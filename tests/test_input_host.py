"""The host twin of the input conversion (include/qpsk_input.h,
csrc/qpsk_input_host.c): G.711 expansion, interleaved and planar layouts,
sizes, refusals, threads, and the same code as a stand-alone program under
AddressSanitizer + UBSan.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import singlecarrier_amd as sc
from g711 import alaw_table, expand, ulaw_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "singlecarrier_amd", "csrc")
SHAPES = [(1, 1), (3, 7), (63, 63), (65, 80), (130, 131)]
ENCS = [sc.IN_S16, sc.IN_ALAW, sc.IN_ULAW]


def source(rng, enc, n, offset):
    """n random elements of the encoding's type in memory that starts `offset`
    bytes past an aligned address"""
    es = 2 if enc == sc.IN_S16 else 1
    raw = np.zeros(n * es + offset + 64, np.uint8)
    base = (-raw.ctypes.data) % 64 + offset
    view = raw[base:base + n * es]
    view[:] = rng.integers(0, 256, n * es, dtype=np.uint8)
    v = view.view(np.int16 if es == 2 else np.uint8)
    assert v.ctypes.data % 64 == offset % 64
    return v


def all_codes(fmt):
    x = np.zeros((1, sc.FRAME_SIZE), np.uint8)
    x[0, :256] = np.arange(256)
    return sc.input_convert_host(x, fmt, 1)[0, 0, :256].astype(np.int64)


def test_all_256_codes_equal_the_formulas_and_the_anchors():
    u, a = all_codes(sc.IN_ULAW), all_codes(sc.IN_ALAW)
    np.testing.assert_array_equal(u, ulaw_table())
    np.testing.assert_array_equal(a, alaw_table())
    assert [u[0x00], u[0x80], u[0x7F], u[0xFF]] == [-32124, 32124, 0, 0]
    assert [a[0x55], a[0xD5], a[0x2A], a[0xAA]] == [-8, 8, -32256, 32256]
    assert np.abs(u).sum() == 1532928 and np.abs(a).sum() == 1564672


def test_codes_equal_audioop_where_python_has_it():
    try:
        import audioop
    except ImportError:
        # (no skip: the formulas and anchors above are the check everywhere)
        return
    codes = bytes(range(256))
    np.testing.assert_array_equal(all_codes(sc.IN_ULAW), np.frombuffer(audioop.ulaw2lin(codes, 2), np.int16))
    np.testing.assert_array_equal(all_codes(sc.IN_ALAW), np.frombuffer(audioop.alaw2lin(codes, 2), np.int16))


@pytest.mark.parametrize("nframes", [1, 3])
@pytest.mark.parametrize("nch,ld", SHAPES)
def test_interleaved_equals_transpose_and_lookup(nch, ld, nframes):
    rng = np.random.default_rng(nch * 10 + nframes)
    T = nframes * sc.FRAME_SIZE
    for enc in ENCS:
        for offset in ((0, 2) if enc == sc.IN_S16 else (0, 1, 3)):
            n = (T - 1) * ld + nch
            flat = source(rng, enc, n, offset)
            # element (t, c) at flat[t * ld + c]: a strided view, no copy
            view = np.lib.stride_tricks.as_strided(flat, (T, nch), (ld * flat.itemsize, flat.itemsize))
            got = sc.input_convert_host(view, enc | sc.IN_INTERLEAVED, nch)
            assert got.shape == (nch, nframes, sc.FRAME_SIZE) and got.dtype == np.int16
            np.testing.assert_array_equal(got.reshape(nch, T), expand(view, enc).T)


@pytest.mark.parametrize("nch", [1, 3, 65])
def test_planar_equals_lookup(nch):
    rng = np.random.default_rng(nch)
    T = 3 * sc.FRAME_SIZE
    for enc in ENCS:
        for offset in ((0, 2) if enc == sc.IN_S16 else (0, 1, 3)):
            x = source(rng, enc, nch * T, offset).reshape(nch, T)
            got = sc.input_convert_host(x, enc | sc.IN_PLANAR, nch)
            np.testing.assert_array_equal(got.reshape(nch, T), expand(x, enc))


def test_input_bytes():
    T = 3 * 1880
    for enc, es in ((sc.IN_S16, 2), (sc.IN_ALAW, 1), (sc.IN_ULAW, 1)):
        assert sc.input_bytes(enc | sc.IN_PLANAR, 65, 3) == 65 * T * es
        assert sc.input_bytes(enc | sc.IN_PLANAR, 65, 3, 1) == 65 * T * es        # ld ignored
        assert sc.input_bytes(enc | sc.IN_INTERLEAVED, 65, 3, 80) == ((T - 1) * 80 + 65) * es
        assert sc.input_bytes(enc | sc.IN_INTERLEAVED, 65, 3, 65) == 65 * T * es
        assert sc.input_bytes(enc | sc.IN_INTERLEAVED, 65, 0, 80) == 0
        assert sc.input_bytes(enc | sc.IN_INTERLEAVED, 65, 3, 64) == 0           # refused
    assert sc.input_bytes(sc.IN_ALAW, 65536, 4095) == 65536 * 4095 * 1880         # past 2^32
    assert sc.input_bytes(3, 1, 1) == 0


def test_every_einval_case_is_refused():
    L = sc.lib()
    src = np.zeros(4 * 1880, np.uint8)
    out = np.full(4 * 1880 + 8, 0x5A5A, np.int16)
    s, o = src.ctypes.data, out.ctypes.data
    A, AI = sc.IN_ALAW, sc.IN_ALAW | sc.IN_INTERLEAVED
    cases = [(3, s, 1, 1, 1, o), (0x20, s, 1, 1, 1, o), (0x11 + 0x10, s, 1, 1, 1, o), (-1, s, 1, 1, 1, o),
             (AI, s, 1, 2, 1, o),                 # ld < nch
             (A, None, 1, 1, 1, o), (A, s, 1, 1, 1, None),
             (A, s, 1, 1, -1, o), (A, s, 1, 0, 1, o),
             (A, s, 1, 1 << 14, 1 << 14, o), (A, s, 1, 1, 1 << 28, o)]
    for fmt, sp, ld, nch, nf, op in cases:
        assert L.qpsk_input_convert_host(fmt, sp, ld, nch, nf, op, 2) == sc.QPSK_EINVAL, (fmt, ld, nch, nf)
    assert (out == 0x5A5A).all()
    assert L.qpsk_input_convert_host(A, None, 1, 1, 0, None, 2) == 0    # no frames: nothing to point at
    # the device entry points check their arguments before any HIP call: the
    # same refusals without a GPU (the pointers are never followed)
    for fmt, sp, ld, nch, nf, op in cases:
        assert L.qpsk_input_convert_device(fmt, sp, ld, nch, nf, op, None) == sc.QPSK_EINVAL
    assert L.qpsk_input_convert_device(A, s, 1, 1, 1, o + (2 if o % 16 == 0 else 0), None) == sc.QPSK_EINVAL   # d_out not 16-byte aligned
    for f in (L.qpsk_rx_batch_fmt, L.qpsk_rx_batch_device_fmt):
        tail = (None,) if f is L.qpsk_rx_batch_device_fmt else ()
        assert f(None, s, A, 1, 1, o, o, None, None, *tail) == sc.QPSK_EINVAL
    err = C.c_int(0)
    for fmt in (3, 0x20, -1):
        assert not L.qpsk_stream_create_fmt(0, 4, 2, 3, 0, fmt, C.byref(err)) and err.value == sc.QPSK_EINVAL
    assert not L.qpsk_stream_acquire_raw(None, C.byref(err)) and err.value == sc.QPSK_EINVAL
    # the Python mirror refuses an unknown format word with the same code
    with pytest.raises(sc.QpskError) as ei:
        sc.input_convert_host(np.zeros((1, 1880), np.uint8), 3, 1)
    assert ei.value.code == sc.QPSK_EINVAL


def test_thread_counts_give_equal_output():
    rng = np.random.default_rng(4)
    x = rng.integers(0, 256, (3 * 1880, 131), dtype=np.uint8)[:, :130]
    one = sc.input_convert_host(x, sc.IN_ULAW | sc.IN_INTERLEAVED, 130, threads=1)
    four = sc.input_convert_host(x, sc.IN_ULAW | sc.IN_INTERLEAVED, 130, threads=4)
    np.testing.assert_array_equal(one, four)
    np.testing.assert_array_equal(one.reshape(130, -1), expand(x, sc.IN_ULAW).T)


def test_host_twin_runs_clean_under_asan_and_ubsan(tmp_path):
    """tests/callers/input_caller.c + qpsk_input_host.c, nothing else, built
    with -fsanitize=address,undefined and run as a program of its own."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    exe = str(tmp_path / "input_caller")
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "callers", "input_caller.c"),
                    os.path.join(CSRC, "qpsk_input_host.c"), "-lpthread"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) >= 6 * 3 * 2 * 2 * 2
