"""The host twin of the level meter and the squelch (include/qpsk_level.h,
csrc/qpsk_level_host.c) against numpy restatements written from the header
alone (tests/level_cases.py), on the oracle's outputs, and under ASan + UBSan.
No GPU."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import singlecarrier_amd as sc
from level_cases import (MIN_SUMSQ, SENT, SINGLE_AT, filled, oracle_case, oracle_classes, random_squelch_case,
                         restate_level, restate_squelch, rows, silence_case, special_rows, squelched_records)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "singlecarrier_amd", "csrc")
INC = os.path.join(ROOT, "include")
ORDERS = [sc.REC_BY_CHANNEL, sc.REC_BY_FRAME]
MODES = [0, 1, 2, 3]


# ------------------------------------------------------------------ 1. the meter
def test_level_of_the_special_rows():
    got = sc.level_host(special_rows())
    assert got.dtype == sc.LEVEL_DTYPE and sc.LEVEL_DTYPE.itemsize == 16
    assert got[0].tolist() == (1880 << 30, -61_603_840, 32768, 1880)        # all -32768
    assert got[1].tolist() == (1880 * 32767 ** 2, 1880 * 32767, 32767, 1880)   # all 32767
    assert got[2].tolist() == (1880 * 32767 ** 2, 0, 32767, 940)            # alternating +-32767
    for k, v in enumerate((-32768, 32767, -1, 1, 12345, -32767)):           # one sample, at SINGLE_AT[k]
        assert special_rows()[3 + k][SINGLE_AT[k]] == v
        assert got[3 + k].tolist() == (v * v, v, abs(v), int(v in (32767, -32768)))
    assert got[9].tolist() == (0, 0, 0, 0)
    assert got[10].tolist() == (940 * (32768 ** 2 + 32767 ** 2), -940, 32768, 1880)   # both rails
    np.testing.assert_array_equal(got, restate_level(special_rows()))


@pytest.mark.parametrize("n", [1, 3, 64, 257])
def test_level_against_numpy(n):
    x = rows(n, seed=n)
    got = sc.level_host(x)
    assert got.tobytes() == restate_level(x).tobytes()
    assert got[-1].tolist() == (1880 << 30, -61_603_840, 32768, 1880)   # rows() ends on a special row
    out = filled(n + 2, sc.LEVEL_DTYPE)   # nothing outside the n rows
    assert sc.lib().qpsk_level_host(x.ctypes.data, n, out[1:].ctypes.data) == 0
    assert out[1:n + 1].tobytes() == got.tobytes()
    assert (out[[0, -1]].view(np.uint8) == SENT).all()


def test_level_shapes_and_refusals():
    assert sc.level_host(np.zeros((3, 5, 1880), np.int16)).shape == (3, 5)
    assert sc.level_host(np.zeros((0, 1880), np.int16)).shape == (0,)
    with pytest.raises(ValueError):
        sc.level_host(np.zeros((3, 1879), np.int16))
    L = sc.lib()
    x, out = np.zeros(1880, np.int16), filled(1, sc.LEVEL_DTYPE)
    assert L.qpsk_level_host(None, 0, None) == 0
    assert L.qpsk_level_host(None, 1, out.ctypes.data) == sc.QPSK_EINVAL
    assert L.qpsk_level_host(x.ctypes.data, 1, None) == sc.QPSK_EINVAL
    assert L.qpsk_level_host(x.ctypes.data, 1 << 28, out.ctypes.data) == sc.QPSK_EINVAL
    assert (out.view(np.uint8) == SENT).all()
    assert sc.level_tiling()["rows_per_block"] >= 1


def test_expanded_g711_never_reaches_the_rails():
    """the header's note on `clipped`: no G.711 code expands to an int16 rail"""
    codes = np.tile(np.arange(256, dtype=np.uint8), 8)[None, :1880]
    for fmt, peak in ((sc.IN_ALAW, 32256), (sc.IN_ULAW, 32124)):
        x = sc.input_convert_host(codes, fmt | sc.IN_PLANAR, 1)
        lv = sc.level_host(x.reshape(1, 1880))
        assert lv["clipped"][0] == 0 and lv["peak"][0] == peak == -int(x.min())


# ------------------------------------------------------------------ 2. the squelch rule
def _squelch(level, prev, valid, bits, soft, min_sumsq, alias_valid=False, alias_last=False):
    """squelch_host on copies, against the restatement; returns the flags"""
    level, valid, bits, soft = level.copy(), valid.copy(), bits.copy(), soft.copy()
    prev = None if prev is None else prev.copy()
    ev, el, eb, es = restate_squelch(level, prev, min_sumsq, valid, bits, soft)
    got = sc.squelch_host(level, valid, min_sumsq, prev=prev, bits=bits, soft=soft,
                          valid_out=valid if alias_valid else None, last=prev if alias_last else None)
    assert (got["valid"] is valid) == alias_valid and (got["last"] is prev) == alias_last
    np.testing.assert_array_equal(got["valid"], ev)
    assert got["last"].tobytes() == el.tobytes()
    np.testing.assert_array_equal(bits, eb)
    assert soft.tobytes() == es.tobytes()
    return got["valid"]


@pytest.mark.parametrize("nch,nf", [(1, 1), (1, 9), (9, 1), (5, 7), (64, 9)])
def test_squelch_against_numpy(nch, nf):
    rng = np.random.default_rng(nch * 100 + nf)
    level, prev, valid, bits, soft = random_squelch_case(rng, nch, nf)
    for min_sumsq in (0, 1, MIN_SUMSQ, sc.FULL_SUMSQ, sc.FULL_SUMSQ + 1):
        for p in (None, prev):
            _squelch(level, p, valid, bits, soft, min_sumsq)
        _squelch(level, prev, valid, bits, soft, min_sumsq, alias_valid=True)
        _squelch(level, prev, valid, bits, soft, min_sumsq, alias_last=True)
        _squelch(level, prev, valid, bits, soft, min_sumsq, alias_valid=True, alias_last=True)


def _levels(sumsq):
    a = np.zeros(np.shape(sumsq), sc.LEVEL_DTYPE)
    a["sumsq"] = sumsq
    return a


def test_squelch_rule_case_by_case():
    one = np.ones((1, 4), np.uint8)
    lv = _levels([[0, 5, 0, 0]])
    # the f-1 term: frame 2 is kept because of frame 1, frame 3 is not
    assert sc.squelch_host(lv, one, 5)["valid"].tolist() == [[0, 1, 1, 0]]
    assert sc.squelch_host(lv, one, 6)["valid"].tolist() == [[0, 0, 0, 0]]
    # prev NULL is a prev of zeros; a loud prev keeps frame 0 only
    assert sc.squelch_host(lv, one, 5, prev=_levels([0]))["valid"].tolist() == [[0, 1, 1, 0]]
    assert sc.squelch_host(lv, one, 5, prev=_levels([5]))["valid"].tolist() == [[1, 1, 1, 0]]
    assert sc.squelch_host(lv, one, 5, prev=_levels([4]))["valid"].tolist() == [[0, 1, 1, 0]]
    # min_sumsq == 0 squelches nothing, silence included
    assert sc.squelch_host(_levels([[0, 0, 0, 0]]), one, 0)["valid"].tolist() == [[1, 1, 1, 1]]
    assert sc.squelch_host(_levels([[0, 0, 0, 0]]), one, 1)["valid"].tolist() == [[0, 0, 0, 0]]
    # flags of 2 and 3 are kept as they are; 0 stays 0
    flags = np.array([[2, 3, 0, 1]], np.uint8)
    assert sc.squelch_host(_levels([[9, 9, 9, 9]]), flags, 5)["valid"].tolist() == [[2, 3, 0, 1]]
    assert sc.squelch_host(_levels([[9, 0, 0, 0]]), flags, 5)["valid"].tolist() == [[2, 3, 0, 0]]
    # sumsq is compared in 64 bits
    big = _levels([[1 << 32, (1 << 32) + 1]])
    assert sc.squelch_host(big, np.ones((1, 2), np.uint8), (1 << 32) + 1)["valid"].tolist() == [[0, 1]]
    assert sc.squelch_host(_levels([[1, 0]]), np.ones((1, 2), np.uint8), 1 << 32)["valid"].tolist() == [[0, 0]]


def test_squelch_last_and_no_frames():
    rng = np.random.default_rng(4)
    level, prev, valid, _, _ = random_squelch_case(rng, 3, 5)
    got = sc.squelch_host(level, valid, MIN_SUMSQ, prev=prev)
    assert got["last"].tobytes() == level[:, -1].tobytes()
    empty = np.zeros((3, 0), np.uint8)
    no_level = np.zeros((3, 0), sc.LEVEL_DTYPE)
    assert sc.squelch_host(no_level, empty, MIN_SUMSQ, prev=prev)["last"].tobytes() == prev.tobytes()
    last = filled(3, sc.LEVEL_DTYPE)
    sc.squelch_host(no_level, empty, MIN_SUMSQ, last=last)
    assert last.tobytes() == bytes(48)   # no prev either: zero
    p = prev.copy()
    sc.squelch_host(no_level, empty, MIN_SUMSQ, prev=p, last=p)
    assert p.tobytes() == prev.tobytes()
    # every optional pointer NULL
    vo = filled((3, 5), np.uint8)
    assert sc.lib().qpsk_squelch_host(level.ctypes.data, None, 3, 5, MIN_SUMSQ, valid.ctypes.data, vo.ctypes.data,
                                      None, None, None) == 0
    np.testing.assert_array_equal(vo, restate_squelch(level, None, MIN_SUMSQ, valid)[0])


def test_squelch_leaves_other_rows_untouched():
    """sentinel rows: only the rows of frames that were valid and are squelched
    are written, and they are zero"""
    valid = np.array([[1, 1, 0, 0, 2, 1]], np.uint8)
    lv = _levels([[9, 0, 0, 0, 0, 0]])   # kept, kept by f-1, invalid, invalid, squelched, squelched
    bits, soft = filled((1, 6, 62), np.uint8), filled((1, 6, 31, 2), np.float32)
    got = sc.squelch_host(lv, valid, 5, bits=bits, soft=soft)
    assert got["valid"].tolist() == [[1, 1, 0, 0, 0, 0]]
    for f in range(6):
        want = 0 if f >= 4 else SENT
        assert (bits[0, f] == want).all() and (soft[0, f].view(np.uint8) == want).all(), f


def test_squelch_refusals():
    L = sc.lib()
    lv, v, vo = _levels([[1]]), np.ones((1, 1), np.uint8), filled((1, 1), np.uint8)
    a, b, c = lv.ctypes.data, v.ctypes.data, vo.ctypes.data

    def call(level=a, nch=1, nf=1, vin=b, vout=c):
        return L.qpsk_squelch_host(level, None, nch, nf, 0, vin, vout, None, None, None)

    assert call() == 0 and vo[0, 0] == 1
    vo[...] = SENT
    for kw in (dict(nch=-1), dict(nf=-1), dict(level=None), dict(vin=None), dict(vout=None),
               dict(nch=1 << 14, nf=1 << 14)):
        assert call(**kw) == sc.QPSK_EINVAL, kw
    assert vo[0, 0] == SENT
    assert call(nch=0, level=None, vin=None, vout=None) == 0
    # the device calls' checks come before any HIP call: no GPU is touched
    assert L.qpsk_level_device(None, 1, a, None) == sc.QPSK_EINVAL
    assert L.qpsk_level_device(a, 1, None, None) == sc.QPSK_EINVAL
    assert L.qpsk_level_device(a, 1 << 28, a, None) == sc.QPSK_EINVAL
    assert L.qpsk_level_device(a + 8, 1, a, None) == sc.QPSK_EINVAL   # d_in below 16 bytes
    assert L.qpsk_level_device(a, 1, a + 4, None) == sc.QPSK_EINVAL   # d_out below 8
    assert L.qpsk_level_device(None, 0, None, None) == 0
    assert L.qpsk_squelch_device(None, None, 1, 1, 0, b, c, None, None, None, None) == sc.QPSK_EINVAL
    assert L.qpsk_squelch_device(a, None, 1, -1, 0, b, c, None, None, None, None) == sc.QPSK_EINVAL
    assert L.qpsk_squelch_device(a + 4, None, 1, 1, 0, b, c, None, None, None, None) == sc.QPSK_EINVAL
    assert L.qpsk_squelch_device(a, a + 4, 1, 1, 0, b, c, None, None, None, None) == sc.QPSK_EINVAL
    assert L.qpsk_squelch_device(a, None, 1, 1, 0, b, c, a + 1, None, None, None) == sc.QPSK_EINVAL   # bits below 2
    assert L.qpsk_squelch_device(a, None, 1, 1, 0, b, c, None, a + 4, None, None) == sc.QPSK_EINVAL   # soft below 8
    assert L.qpsk_squelch_device(a, None, 1, 1, 0, b, c, None, None, a + 4, None) == sc.QPSK_EINVAL
    n = C.c_uint32(9)
    assert L.qpsk_rx_batch_records_squelch(None, b, 1, 0, None, 0, 0, None, None, None, None, C.addressof(n),
                                           None) == sc.QPSK_EINVAL
    assert L.qpsk_rx_batch_records_squelch_device(None, b, 1, 0, None, 0, 0, None, None, None, None, C.addressof(n),
                                                  None, None) == sc.QPSK_EINVAL
    assert n.value == 9


# ------------------------------------------------------------------ 3, 4. on the oracle
def _restate_records(d, valid, order):
    """(channel, frame, words, groups) of the list, in numpy"""
    if order == sc.REC_BY_FRAME:
        fc = np.argwhere(valid.T != 0)
        f, c = fc[:, 0], fc[:, 1]
        per = (valid != 0).sum(axis=0)
    else:
        cf = np.argwhere(valid != 0)
        c, f = cf[:, 0], cf[:, 1]
        per = (valid != 0).sum(axis=1)
    w = ((d["bits"][c, f] == 1).astype(np.uint64) << np.arange(62, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    return c, f, w, np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)


@pytest.mark.parametrize("mode", MODES)
def test_squelch_on_the_oracle(mode):
    x, d, level = oracle_case(mode)
    np.testing.assert_array_equal(sc.level_host(x), level)
    own, before, gone, invalid = oracle_classes(d, level)
    # a condition of the test, which the reference alone meets: all three classes of valid frames
    counts = [int(m.sum()) for m in (own, before, gone, invalid)]
    print(f"mode {mode}: kept on their own {counts[0]}, kept by the previous frame {counts[1]}, "
          f"squelched {counts[2]}, invalid {counts[3]}; smallest non-zero sumsq "
          f"{int(level['sumsq'][level['sumsq'] > 0].min())}")
    assert counts == [20, 18, 15, 11] and int((d["valid"] != 0).sum()) == 53
    assert level["sumsq"][level["sumsq"] > 0].min() > 2.5e10 > MIN_SUMSQ
    s = sc.squelch_host(level, d["valid"], MIN_SUMSQ)
    np.testing.assert_array_equal(s["valid"] != 0, own | before)
    for order in ORDERS:
        got = sc.compact_host(d["bits"], s["valid"], d["trace"], d["soft"], order=order)
        c, f, w, groups = _restate_records(d, np.where(own | before, d["valid"], 0), order)
        assert got["count"] == 38 == len(c)
        np.testing.assert_array_equal(got["rec"]["channel"], c)
        np.testing.assert_array_equal(got["rec"]["frame"], f)
        np.testing.assert_array_equal(got["rec"]["bits"], w)
        np.testing.assert_array_equal(got["groups"], groups)
        np.testing.assert_array_equal(got["trace"], d["trace"][c, f])
        assert got["soft"].tobytes() == d["soft"][c, f].tobytes()
        assert got["rec"].tobytes() == squelched_records(d, level, None, MIN_SUMSQ, order)[0]["rec"].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_silence_gives_no_records(mode):
    """the reference calls silence valid: 12 frames of 12, non-zero bits; a
    squelch at the lowest level there is leaves none of them"""
    x, d = silence_case(mode)
    assert int(d["valid"].sum()) == 12 and (d["trace"][..., 1] == 128).all() and d["bits"].any()
    level = sc.level_host(x)
    assert level.tobytes() == bytes(12 * 16)
    for order in ORDERS:
        assert squelched_records(d, level, None, 1, order)[0]["count"] == 0
        assert squelched_records(d, level, None, 0, order)[0]["count"] == 12
    bits, soft = d["bits"].copy(), d["soft"].copy()
    sc.squelch_host(level, d["valid"], 1, bits=bits, soft=soft)
    assert not bits.any() and soft.tobytes() == bytes(soft.nbytes)


# ------------------------------------------------------------------ 5. the dB helpers
def test_db_helpers():
    full = sc.FULL_SUMSQ
    assert full == 1880 << 30
    assert sc.level_dbfs([full])[0] == 0.0 and sc.sumsq_of_dbfs(0.0) == full
    assert sc.level_dbfs([0])[0] == -math.inf and sc.sumsq_of_dbfs(-math.inf) == 0
    assert sc.sumsq_of_dbfs(1.0) == full and sc.sumsq_of_dbfs(math.nan) == 0   # clamped; no level
    assert sc.sumsq_of_dbfs(-1000.0) == 1   # every finite level needs some energy
    assert sc.level_dbfs(sc.level_host(np.full((1, 1880), -32768, np.int16)))[0] == 0.0
    assert abs(sc.level_dbfs([full // 10])[0] + 10.0) < 1e-9 and abs(sc.level_dbfs([1])[0] + 123.05) < 0.01
    q = np.unique(np.concatenate([np.arange(1, 70), full - np.arange(0, 70), 10 ** np.arange(1, 13),
                                  np.random.default_rng(5).integers(1, full, 200)])).astype(np.uint64)
    db = sc.level_dbfs(q)
    assert (np.diff(db) > 0).all()   # strictly monotone on distinct sumsq
    # Round trip.  sumsq_of_dbfs(db) is by definition the smallest s with
    # level_dbfs(s) >= db, so with db = level_dbfs(q) it is at most q.  It is
    # also at least q: neighbouring sumsq differ in level by 10 / (ln 10 * q)
    # >= 2.1e-12 dB (q <= 2.02e12), a thousand times the double rounding of a
    # level of at most 124 dB in magnitude (2 ulp <= 2.9e-14), so level_dbfs(q - 1)
    # < level_dbfs(q) in double.  The bound is therefore equality.
    for s, d in zip(q.tolist(), db.tolist()):
        assert sc.sumsq_of_dbfs(d) == s
    # between two levels: the smallest sumsq at or above the threshold
    for d in (-3.0, -20.0, -47.5, -90.0):
        s = sc.sumsq_of_dbfs(d)
        assert sc.level_dbfs([s])[0] >= d > sc.level_dbfs([s - 1])[0]
        assert abs(s - full * 10 ** (d / 10)) <= 1 + 1e-9 * s
    assert sc.sumsq_of_dbfs(-20.0) <= sc.sumsq_of_dbfs(-19.0)


# ------------------------------------------------------------------ 6. sanitizers
def _read(buf, off, dtype, n):
    a = np.frombuffer(buf, dtype, n, off)
    return a.copy(), off + a.nbytes


def test_sanitized_host_twin(tmp_path):
    """csrc/qpsk_level_host.c driven by tests/sanitize/level_check.c (its own
    main, every array a heap block of exactly the stated size) under ASan +
    UBSan on the CPU: any report aborts the run, and what it computed is what
    the unsanitized library computes from the same inputs."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    exe = str(tmp_path / "level_check")
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I" + INC, "-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "sanitize", "level_check.c"),
                    os.path.join(CSRC, "qpsk_level_host.c"), "-lm"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(tmp_path)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    # the meter
    buf = (tmp_path / "level.bin").read_bytes()
    n = int(np.frombuffer(buf, np.int32, 1)[0])
    x, off = _read(buf, 4, np.int16, n * 1880)
    lv, off = _read(buf, off, sc.LEVEL_DTYPE, n)
    assert off == len(buf) and n == 17
    assert lv.tobytes() == sc.level_host(x.reshape(n, 1880)).tobytes() == restate_level(x.reshape(n, 1880)).tobytes()
    # the squelch, case by case with the same aliasing
    buf = (tmp_path / "squelch.bin").read_bytes()
    off = ncases = 0
    L = sc.lib()
    while off < len(buf):
        (nch, nf, hasprev, alias, _), off = _read(buf, off, np.int32, 5)
        (min_sumsq,), off = _read(buf, off, np.uint64, 1)
        cf = nch * nf
        level, off = _read(buf, off, sc.LEVEL_DTYPE, cf)
        prev, off = _read(buf, off, sc.LEVEL_DTYPE, nch)
        vin, off = _read(buf, off, np.uint8, cf)
        bits, off = _read(buf, off, np.uint8, cf * 62)
        soft, off = _read(buf, off, np.float32, cf * 62)
        want = []
        for dt, k in ((np.uint8, cf), (np.uint8, cf * 62), (np.float32, cf * 62), (sc.LEVEL_DTYPE, nch)):
            a, off = _read(buf, off, dt, k)
            want.append(a)
        vout = vin if alias & 1 else filled(cf, np.uint8)
        last = prev if alias & 2 else filled(nch, sc.LEVEL_DTYPE)
        bare = bool(alias & 4)
        assert L.qpsk_squelch_host(level.ctypes.data, prev.ctypes.data if hasprev else None, int(nch), int(nf),
                                   int(min_sumsq), vin.ctypes.data, vout.ctypes.data,
                                   None if bare else bits.ctypes.data, None if bare else soft.ctypes.data,
                                   None if bare else last.ctypes.data) == 0
        for got, w in zip((vout, bits, soft, last), want):
            assert got.tobytes() == w.tobytes(), (nch, nf, hasprev, alias, int(min_sumsq))
        ncases += 1
    assert f"{ncases} squelch cases" in r.stdout and ncases == 7 * 2 * 3 * 5


@pytest.mark.parametrize("cc,std", [("gcc", "-std=c99"), ("gcc", "-std=gnu11"), ("g++", "-std=c++17")])
def test_header_compiles_as_c_and_cxx(tmp_path, cc, std):
    src = tmp_path / ("t.c" if cc == "gcc" else "t.cc")
    src.write_text('#include "qpsk_level.h"\n'
                   "int main(void) { qpsk_frame_level q = {1, 2, 3, 4}; "
                   "return (int)sizeof q - 16 + (int)q.sumsq - 1 + q.clipped - 4; }\n")
    r = subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
