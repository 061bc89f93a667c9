"""The host twin of the output conversion (include/qpsk_output.h,
csrc/qpsk_output_host.c): G.711 compression, planar and interleaved layouts,
untouched memory, sizes, refusals, threads, the same code as a stand-alone
program under AddressSanitizer + UBSan, and the example's options.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import singlecarrier_amd as sc
from g711 import ALL, CODES, TABLES, compress

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "singlecarrier_amd", "csrc")
ENCS = [sc.OUT_S16, sc.OUT_ALAW, sc.OUT_ULAW]
NCHS = [1, 63, 64, 65, 130]
NS = [1, 127, 128, 129, 2783]
SENTINEL = 0xC3


def lib_codes(enc):
    """the library's codes of all 65,536 samples"""
    return sc.output_convert_host(ALL.astype(np.int16)[None], enc | sc.OUT_PLANAR)[0]


def test_all_65536_inputs_equal_the_formulas_and_the_anchors():
    for enc in (sc.OUT_ALAW, sc.OUT_ULAW):
        np.testing.assert_array_equal(lib_codes(enc), CODES[enc])
    u, a = lib_codes(sc.OUT_ULAW), lib_codes(sc.OUT_ALAW)
    at = lambda t, x: int(t[x + 32768])
    assert [at(u, 0), at(u, -1), at(u, 32767), at(u, -32768)] == [0xFF, 0x7F, 0x80, 0x00]
    assert [at(a, 0), at(a, -1), at(a, 32767), at(a, -32768)] == [0xD5, 0x55, 0xAA, 0x2A]


def test_round_trip_monotonicity_and_error():
    k = np.arange(256)
    for enc, worst in ((sc.OUT_ALAW, 512), (sc.OUT_ULAW, 644)):
        back = sc.output_convert_host(TABLES[enc].astype(np.int16)[None], enc)[0]
        differ = np.nonzero(back != k)[0].tolist()
        # mu-law 0x7F expands to 0, which compresses to 0xFF
        assert differ == ([0x7F] if enc == sc.OUT_ULAW else [])
        if enc == sc.OUT_ULAW:
            assert back[0x7F] == 0xFF
        y = TABLES[enc][lib_codes(enc)]
        assert (np.diff(y) >= 0).all()
        assert int(np.abs(y - ALL).max()) == worst


def test_codes_equal_audioop_where_python_has_it():
    """A-law: audioop.lin2alaw is G.191's alaw_compress, equal on all 65,536
    inputs.  mu-law: audioop.lin2ulaw negates the 14-bit sample (-(x >> 2))
    where G.191's ulaw_compress takes its ones' complement ((~x) >> 2), so its
    magnitude is one step of 4 further out on every negative input: it equals
    this library on every x >= 0, and audioop(x) == library(x - 4) on every
    x < 0, which changes the code of 508 inputs (all negative).  The library
    follows G.191, the inverse of the expansion on every code (test above);
    the relation to audioop is asserted exactly, on every input."""
    audioop = pytest.importorskip("audioop")
    raw = ALL.astype("<i2").tobytes()
    np.testing.assert_array_equal(lib_codes(sc.OUT_ALAW), np.frombuffer(audioop.lin2alaw(raw, 2), np.uint8))
    u, ref = lib_codes(sc.OUT_ULAW), np.frombuffer(audioop.lin2ulaw(raw, 2), np.uint8)
    np.testing.assert_array_equal(u[32768:], ref[32768:])
    np.testing.assert_array_equal(u[np.maximum(np.arange(32768) - 4, 0)], ref[:32768])
    assert int((u != ref).sum()) == 508


def _placed(nbytes, offset, dtype):
    """a sentinel-filled array of nbytes that starts `offset` bytes past a
    64-byte boundary, with 64 guard bytes either side: (whole, view)"""
    raw = np.full(nbytes + offset + 192, SENTINEL, np.uint8)
    base = (-raw.ctypes.data) % 64 + 64 + offset
    return raw, raw[base:base + nbytes].view(dtype)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("nch", NCHS)
def test_layouts_equal_numpy_and_nothing_else_is_written(nch, n):
    """planar and interleaved, every encoding, ld = minimum, +1, +3, the source
    rows apart too; every byte outside the block's elements keeps its sentinel"""
    rng = np.random.default_rng(1000 * nch + n)
    L = sc.lib()
    for k, pad in enumerate((0, 1, 3)):
        src_ld = n + (3, 0, 1)[k]
        wide = rng.integers(-32768, 32768, (nch, src_ld), dtype=np.int16)
        wide[0, 0], wide[-1, n - 1] = -32768, 32767
        x = wide[:, :n]
        for enc in ENCS:
            es = 2 if enc == sc.OUT_S16 else 1
            dt = np.int16 if es == 2 else np.uint8
            for lay in (sc.OUT_PLANAR, sc.OUT_INTERLEAVED):
                fmt = enc | lay
                rows, cols = (n, nch) if lay else (nch, n)
                ld = cols + pad
                nbytes = sc.output_bytes(fmt, nch, n, ld)
                assert nbytes == ((rows - 1) * ld + cols) * es
                raw, flat = _placed(nbytes, (k * es) % 4 if es == 2 else k + (nch & 1), dt)
                assert L.qpsk_output_convert_host(fmt, x.ctypes.data, src_ld, nch, n, flat.ctypes.data, ld, 3) == 0
                full = np.full(rows * ld, SENTINEL * 0x0101 if es == 2 else SENTINEL, np.int64)
                full[:flat.size] = flat.view(np.uint16) if es == 2 else flat
                full = full.reshape(rows, ld)
                want = compress(x, enc)
                want = want.T if lay else want
                what = f"fmt {fmt:#x} nch {nch} n {n} ld {ld}"
                np.testing.assert_array_equal(full[:, :cols].astype(np.uint16 if es == 2 else np.uint8),
                                              want.view(np.uint16) if es == 2 else want, err_msg=what)
                assert (full[:, cols:] == (SENTINEL * 0x0101 if es == 2 else SENTINEL)).all(), what + ": gaps"
                lo = flat.ctypes.data - raw.ctypes.data
                assert (raw[:lo] == SENTINEL).all() and (raw[lo + nbytes:] == SENTINEL).all(), what + ": around"
                # the Python mirror gives the same block
                got = sc.output_convert_host(x, fmt, ld=ld)
                np.testing.assert_array_equal(got[:, :cols], want, err_msg=what)


def test_output_bytes():
    for enc, es in ((sc.OUT_S16, 2), (sc.OUT_ALAW, 1), (sc.OUT_ULAW, 1)):
        assert sc.output_bytes(enc | sc.OUT_PLANAR, 65, 2783, 2783) == 65 * 2783 * es
        assert sc.output_bytes(enc | sc.OUT_PLANAR, 65, 2783, 3000) == (64 * 3000 + 2783) * es
        assert sc.output_bytes(enc | sc.OUT_INTERLEAVED, 65, 2783, 80) == (2782 * 80 + 65) * es
        assert sc.output_bytes(enc | sc.OUT_INTERLEAVED, 65, 2783, 65) == 65 * 2783 * es
        assert sc.output_bytes(enc | sc.OUT_INTERLEAVED, 65, 0, 80) == 0
        assert sc.output_bytes(enc | sc.OUT_INTERLEAVED, 65, 5, 64) == 0      # refused
        assert sc.output_bytes(enc | sc.OUT_PLANAR, 65, 5, 4) == 0            # refused
    n = 4095 * 1880
    assert sc.output_bytes(sc.OUT_ALAW, 65536, n, n) == 65536 * n             # past 2^32
    assert sc.output_bytes(sc.OUT_ALAW, 1 << 14, (1 << 14) * 1880, (1 << 14) * 1880) == 0   # nch * n = 2^28 * 1880
    assert sc.output_bytes(sc.OUT_ALAW, 1 << 14, (1 << 14) * 1880 - 1, (1 << 14) * 1880) > 0
    assert sc.output_bytes(3, 1, 1, 1) == 0


def test_every_einval_case_is_refused():
    L = sc.lib()
    src = np.zeros(64, np.int16)
    dst = np.full(64, SENTINEL, np.uint8)
    s, d = src.ctypes.data, dst.ctypes.data
    A, AI = sc.OUT_ALAW, sc.OUT_ALAW | sc.OUT_INTERLEAVED
    big = (1 << 14) * 1880
    # (fmt, src, src_ld, nch, n, dst, ld)
    cases = [(3, s, 4, 2, 4, d, 4), (0x20, s, 4, 2, 4, d, 4), (0x21, s, 4, 2, 4, d, 4), (-1, s, 4, 2, 4, d, 4),
             (AI, s, 4, 3, 4, d, 2),               # interleaved ld < nch
             (A, s, 4, 2, 4, d, 3),                # planar ld < n
             (A, s, 3, 2, 4, d, 4),                # src_ld < n
             (A, None, 4, 2, 4, d, 4), (A, s, 4, 2, 4, None, 4),
             (A, s, 4, 0, 4, d, 4), (A, s, 4, 2, -1, d, 4),
             (A, s, big, 1 << 14, big, d, big)]    # nch * n >= 2^28 * 1880
    for fmt, sp, sld, nch, n, dp, ld in cases:
        assert L.qpsk_output_convert_host(fmt, sp, sld, nch, n, dp, ld, 2) == sc.QPSK_EINVAL, (fmt, sld, nch, n, ld)
    assert (dst == SENTINEL).all()
    assert L.qpsk_output_convert_host(A, None, 0, 1, 0, None, 0, 2) == 0    # nothing to convert, nothing to point at
    # the device entry points check their arguments before any HIP call: the
    # same refusals without a GPU (the pointers are never followed)
    for fmt, sp, sld, nch, n, dp, ld in cases:
        assert L.qpsk_output_convert_device(fmt, sp, sld, nch, n, dp, ld, None) == sc.QPSK_EINVAL
    assert L.qpsk_output_convert_device(A, None, 0, 1, 0, None, 0, None) == 0
    assert L.qpsk_output_convert_device(sc.OUT_S16 | sc.OUT_INTERLEAVED, s, 4, 2, 4, d + 1, 4, None) == sc.QPSK_EINVAL
    for f in (L.qpsk_tx_batch_fmt, L.qpsk_tx_batch_device_fmt):
        tail = (None,) if f is L.qpsk_tx_batch_device_fmt else ()
        assert f(None, s, 1, d, A, 4000, *tail) == sc.QPSK_EINVAL          # no context
        assert f(None, s, 1, d, sc.OUT_S16, 4000, *tail) == sc.QPSK_EINVAL   # the plain call's refusal
    # the Python mirror refuses an unknown format word and a short ld with the same code
    for fmt, ld in ((3, None), (AI, 1)):
        with pytest.raises(sc.QpskError) as ei:
            sc.output_convert_host(np.zeros((2, 4), np.int16), fmt, ld=ld)
        assert ei.value.code == sc.QPSK_EINVAL


def test_thread_counts_give_equal_output():
    rng = np.random.default_rng(4)
    x = rng.integers(-32768, 32768, (130, 2783), dtype=np.int16)
    for fmt in (sc.OUT_ULAW | sc.OUT_INTERLEAVED, sc.OUT_ALAW | sc.OUT_PLANAR, sc.OUT_S16 | sc.OUT_INTERLEAVED):
        one, two, five = (sc.output_convert_host(x, fmt, threads=t) for t in (1, 2, 5))
        np.testing.assert_array_equal(one, two)
        np.testing.assert_array_equal(one, five)
        want = compress(x, fmt & 0x0f)
        np.testing.assert_array_equal(one, want.T if fmt & 0x10 else want)


def test_host_twin_runs_clean_under_asan_and_ubsan(tmp_path):
    """tests/callers/output_caller.c + qpsk_output_host.c, nothing else, built
    with -fsanitize=address,undefined and run as a program of its own."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    exe = str(tmp_path / "output_caller")
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "callers", "output_caller.c"),
                    os.path.join(CSRC, "qpsk_output_host.c"), "-lpthread"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) == 5 * 5 * 3 * 2 * 3


def test_example_writes_the_host_twins_trunk(tmp_path):
    """examples/qpsk_tx_raw builds; -c -f alaw -i writes the trunk the host twin
    gives for the host transmitter's samples, -c -f ulaw one file of codes per
    channel"""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = os.path.join(ROOT, "examples", "qpsk_tx_raw")
    bits = np.random.default_rng(8).integers(0, 2, (3, 2, 8, 62), dtype=np.uint8)
    paths = []
    for c in range(3):
        paths.append(str(tmp_path / f"ch{c}.bits"))
        bits[c].tofile(paths[-1])
    x = sc.tx_batch_host(bits, gap=17)
    trunk = tmp_path / "trunk.al"
    r = subprocess.run([exe, "-b", "-c", "-f", "alaw", "-i", "-g", "17", *paths, "-o", str(trunk)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = sc.output_convert_host(x, sc.OUT_ALAW | sc.OUT_INTERLEAVED)
    assert want.shape == (2 * 1897, 3)
    np.testing.assert_array_equal(np.fromfile(trunk, np.uint8).reshape(-1, 3), want)
    np.testing.assert_array_equal(want, compress(x, sc.OUT_ALAW).T)
    pre = tmp_path / "u_"
    r = subprocess.run([exe, "-b", "-c", "-f", "ulaw", "-g", "17", *paths, "-o", str(pre)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for c in range(3):
        np.testing.assert_array_equal(np.fromfile(f"{pre}{c}.raw", np.uint8), compress(x[c], sc.OUT_ULAW))
