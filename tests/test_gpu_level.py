"""The level meter, the squelch and the record calls with squelch on the GPU
(include/qpsk_level.h) against the host twins and the oracle; cases of
tests/level_cases.py.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import gpu_delay
import singlecarrier_amd as sc
from level_cases import (MIN_SUMSQ, SENT, filled, oracle_case, oracle_classes, random_squelch_case, restate_level,
                         rows, silence_case, squelched_records)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ORDERS = [sc.REC_BY_CHANNEL, sc.REC_BY_FRAME]
R = sc.level_tiling()["rows_per_block"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(a, guard=1):
    """A numpy array [n][...] (uint8, float32 or LEVEL_DTYPE, n > 0) on the
    device between `guard` rows of sentinel bytes: (the whole buffer as bytes
    [n + 2 * guard][row bytes], the n rows as a tensor [n][row elements], a
    level row being two int64)"""
    a = np.ascontiguousarray(a)
    n = a.shape[0]
    raw = a.view(np.uint8).reshape(n, -1)
    whole = torch.full((n + 2 * guard, raw.shape[1]), SENT, dtype=torch.uint8, device="cuda")
    body = whole[guard:guard + n]
    body.copy_(torch.from_numpy(raw))
    dt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32, sc.LEVEL_DTYPE: torch.int64}[a.dtype]
    return whole, body.view(dt)


def _guards_intact(whole, guard=1):
    """the first and last `guard` rows of a tensor still hold the sentinel in every byte"""
    g = torch.cat([whole[:guard].reshape(-1).view(torch.uint8), whole[-guard:].reshape(-1).view(torch.uint8)])
    return bool((g == SENT).all())


# ------------------------------------------------------------------ 7. the meter at its tiling's edges
@pytest.mark.parametrize("nrows", sorted({1, max(R - 1, 1), R, R + 1, 3 * R + 1, 64 * R + 3}))
def test_level_device_equals_host(nrows):
    x = rows(nrows, seed=nrows)
    exp = sc.level_host(x)
    assert exp.tobytes() == restate_level(x).tobytes()
    xin = torch.full((nrows + 2, sc.FRAME_SIZE), 12345, dtype=torch.int16, device="cuda")   # loud rows around the block
    xin[1:nrows + 1].copy_(torch.from_numpy(x))
    out = torch.from_numpy(filled((nrows + 2, 2), np.int64)).cuda()
    got = sc.level_device(xin[1:nrows + 1], out=out[1:nrows + 1])
    torch.cuda.synchronize()
    assert sc.level_from_tensor(got).tobytes() == exp.tobytes()
    assert _guards_intact(out)   # nothing outside the nrows rows


# ------------------------------------------------------------------ 8. rows more than 2^32 bytes apart
def test_level_device_past_4_gib():
    n = 1_143_000
    assert n * sc.FRAME_SIZE * 2 > 2 ** 32 and n < 2 ** 28
    x = torch.randint(-32768, 32768, (n, sc.FRAME_SIZE), dtype=torch.int16, device="cuda")
    first_past = 2 ** 32 // (sc.FRAME_SIZE * 2) + 1   # the first row that lies wholly past 2^32 bytes
    assert first_past < n - 1
    x[first_past] = 32767
    x[first_past - 1] = torch.from_numpy(rows(13)[3]).cuda()
    x[n - 1] = -32768   # the last row: the largest sumsq there is
    out = sc.level_device(x)
    assert tuple(out.shape) == (n, 2)
    bad = 0
    for a in range(0, n, 100_000):   # torch's own int64 reductions, a slab at a time
        v = x[a:a + 100_000].to(torch.int64)
        sumsq, s = (v * v).sum(1), v.sum(1)
        peak = v.abs().amax(1)
        clipped = ((v == 32767) | (v == -32768)).sum(1)
        rest = (s & 0xFFFFFFFF) | (peak << 32) | (clipped << 48)
        bad += int(((out[a:a + 100_000, 0] != sumsq) | (out[a:a + 100_000, 1] != rest)).sum())
    assert bad == 0
    tail = sc.level_from_tensor(out[[first_past, n - 1]])
    assert tail[0].tolist() == (1880 * 32767 ** 2, 1880 * 32767, 32767, 1880)
    assert tail[1].tolist() == (1880 << 30, -61_603_840, 32768, 1880)


# ------------------------------------------------------------------ 9. the squelch
def _squelch_on_device(level, prev, valid, bits, soft, min_sumsq, alias_valid=False, alias_last=False):
    """squelch_device on guarded buffers against squelch_host on copies"""
    nch, nf = valid.shape
    hb, hs = bits.copy(), soft.copy()
    hp = None if prev is None else prev.copy()
    exp = sc.squelch_host(level, valid, min_sumsq, prev=hp, bits=hb, soft=hs)
    cf = nch * nf
    wl, dl = _guarded(level.reshape(cf))
    wv, dv = _guarded(valid.reshape(cf), guard=8)
    wb, db = _guarded(bits.reshape(cf, sc.NBITS))
    wso, dso = _guarded(soft.reshape(cf, 62))
    wo, do = _guarded(filled(cf, np.uint8), guard=8)
    wla, dla = _guarded(filled(nch, sc.LEVEL_DTYPE))
    wp, dp = _guarded(prev if prev is not None else np.zeros(nch, sc.LEVEL_DTYPE))
    got = sc.squelch_device(dl.view(nch, nf, 2), dv.view(nch, nf), min_sumsq, prev=None if prev is None else dp,
                            bits=db.view(nch, nf, sc.NBITS), soft=dso.view(nch, nf, 31, 2),
                            valid_out=dv.view(nch, nf) if alias_valid else do.view(nch, nf),
                            last=dp if alias_last else dla)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got["valid"].cpu().numpy(), exp["valid"])
    assert sc.level_from_tensor(got["last"]).tobytes() == exp["last"].tobytes()
    np.testing.assert_array_equal(db.cpu().numpy().reshape(bits.shape), hb)
    assert dso.cpu().numpy().tobytes() == hs.tobytes()
    # the inputs that are not outputs too, and every guard
    assert sc.level_from_tensor(dl).tobytes() == level.tobytes()
    if not alias_valid:
        np.testing.assert_array_equal(dv.cpu().numpy().reshape(valid.shape), valid)
    if prev is not None and not alias_last:
        assert sc.level_from_tensor(dp).tobytes() == prev.tobytes()
    for w, g in ((wl, 1), (wv, 8), (wb, 1), (wso, 1), (wo, 8), (wla, 1), (wp, 1)):
        assert _guards_intact(w, g)
    if alias_valid:
        assert bool((wo == SENT).all())
    if alias_last:
        assert bool((wla.view(torch.uint8) == SENT).all())


@pytest.mark.parametrize("nch,nf", [(1, 1), (5, 7), (64, 9), (300, 33)])
def test_squelch_device_equals_host(nch, nf):
    rng = np.random.default_rng(nch * 100 + nf)
    level, prev, valid, bits, soft = random_squelch_case(rng, nch, nf)
    for min_sumsq in (0, MIN_SUMSQ, sc.FULL_SUMSQ + 1):
        _squelch_on_device(level, None, valid, bits, soft, min_sumsq)
        _squelch_on_device(level, prev, valid, bits, soft, min_sumsq)
    _squelch_on_device(level, prev, valid, bits, soft, MIN_SUMSQ, alias_valid=True, alias_last=True)


def test_squelch_device_on_the_oracle_and_no_frames():
    x, d, level = oracle_case(0)
    own, before, gone, invalid = oracle_classes(d, level)
    assert own.any() and before.any() and gone.any() and invalid.any()
    _squelch_on_device(level.copy(), None, d["valid"].copy(), d["bits"].copy(), d["soft"].copy(), MIN_SUMSQ)
    # no frames: last is prev, or zero
    rng = np.random.default_rng(3)
    _, prev, _, _, _ = random_squelch_case(rng, 5, 1)
    e = torch.empty((5, 0), dtype=torch.uint8, device="cuda")
    lv = torch.empty((5, 0, 2), dtype=torch.int64, device="cuda")
    got = sc.squelch_device(lv, e, MIN_SUMSQ, prev=_dev(prev.view(np.int64).reshape(5, 2)), valid_out=e)
    assert sc.level_from_tensor(got["last"]).tobytes() == prev.tobytes()
    got = sc.squelch_device(lv, e, MIN_SUMSQ, valid_out=e)
    assert sc.level_from_tensor(got["last"]).tobytes() == bytes(5 * 16)


# ------------------------------------------------------------------ 10. records with squelch
def _same(got, exp, rows=True):
    assert got["count"] == exp["count"]
    np.testing.assert_array_equal(got["groups"], exp["groups"])
    assert got["rec"].tobytes() == exp["rec"].tobytes()
    if rows:
        np.testing.assert_array_equal(got["trace"], exp["trace"])
        assert got["soft"].tobytes() == exp["soft"].tobytes()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mode", [sc.MODE_REFERENCE, sc.MODE_DEC752])
@pytest.mark.parametrize("case", ["oracle", "silence"])
def test_demod_records_squelch(case, mode, order):
    if case == "oracle":
        x, d, level = oracle_case(mode)
        min_sumsq, count = MIN_SUMSQ, 38
    else:
        x, d = silence_case(mode)
        level = restate_level(x)
        min_sumsq, count = 1, 0
    nch, nf = d["valid"].shape
    plain = int((d["valid"] != 0).sum())
    assert plain in (53, 12)
    for cap in (None, max(count - 5, 0), count + 3):
        exp, last = squelched_records(d, level, None, min_sumsq, order, cap)
        assert exp["count"] == count
        rx = sc.Receiver(nch, mode=mode)
        got = rx.demod_records_squelch(x, min_sumsq, order=order, cap=cap, trace=True, soft=True)
        assert rx.frames == nf
        rx.close()
        assert len(got["rec"]) == min(count, nch * nf if cap is None else cap)
        _same(got, exp)
        assert got["level"].tobytes() == level.tobytes()
        assert got["prev"].tobytes() == last.tobytes() == level[:, -1].tobytes()
    # min_sumsq == 0: demod_records bit for bit
    for cap in (None, plain - 5):
        rx = sc.Receiver(nch, mode=mode)
        want = rx.demod_records(x, order=order, cap=cap, trace=True, soft=True)
        rx.close()
        rx = sc.Receiver(nch, mode=mode)
        got = rx.demod_records_squelch(x, 0, order=order, cap=cap, trace=True, soft=True)
        rx.close()
        assert want["count"] == plain
        _same(got, want)
        _same(got, sc.compact_host(d["bits"], d["valid"], d["trace"], d["soft"], order=order, cap=cap))
        assert got["level"].tobytes() == level.tobytes()


def test_demod_records_squelch_plain_outputs_and_many_channels():
    """without trace / soft rows, as a pure count, and on 300 channels (more
    than one workgroup of every pass) of which every third is idle"""
    nch, nf = 300, 12
    x = sc.synth_device(41, nch, nf, 5.0).cpu().numpy()
    x[::3] = 0
    x[1::3, 6:] = 0
    rx = sc.Receiver(nch)
    d = rx.demod(x, trace=True, soft=True)
    rx.close()
    level = sc.level_host(x)
    min_sumsq = sc.sumsq_of_dbfs(-60.0)
    for order in ORDERS:
        exp, last = squelched_records(d, level, None, min_sumsq, order)
        assert 0 < exp["count"] < int((d["valid"] != 0).sum())
        rx = sc.Receiver(nch)
        got = rx.demod_records_squelch(x, min_sumsq, order=order)
        assert "trace" not in got and "soft" not in got
        _same(got, exp, rows=False)
        assert got["level"].tobytes() == level.tobytes() and got["prev"].tobytes() == last.tobytes()
        rx.reset()
        got = rx.demod_records_squelch(x, min_sumsq, order=order, cap=0)
        rx.close()
        assert got["count"] == exp["count"] and len(got["rec"]) == 0
        np.testing.assert_array_equal(got["groups"], exp["groups"])


# ------------------------------------------------------------------ 11. split calls
@pytest.mark.parametrize("order", ORDERS)
def test_split_calls_carry_prev(order):
    x, d, level = oracle_case(0)
    whole, _ = squelched_records(d, level, None, MIN_SUMSQ, order)

    def two_calls(carry):
        rx = sc.Receiver(8)
        a = rx.demod_records_squelch(np.ascontiguousarray(x[:, :3]), MIN_SUMSQ, order=order, trace=True, soft=True)
        b = rx.demod_records_squelch(np.ascontiguousarray(x[:, 3:]), MIN_SUMSQ, prev=a["prev"] if carry else None,
                                     order=order, trace=True, soft=True)
        rx.close()
        assert a["prev"].tobytes() == level[:, 2].tobytes() and b["prev"].tobytes() == level[:, 7].tobytes()
        return a, b

    a, b = two_calls(True)
    rb = b["rec"].copy()
    rb["frame"] += 3
    rec = np.concatenate([a["rec"], rb])
    tr, so = np.concatenate([a["trace"], b["trace"]]), np.concatenate([a["soft"], b["soft"]])
    if order == sc.REC_BY_CHANNEL:   # a channel's frames of both calls side by side
        k = np.lexsort((rec["frame"], rec["channel"]))
        rec, tr, so = rec[k], tr[k], so[k]
    assert a["count"] + b["count"] == whole["count"] == 38
    assert rec.tobytes() == whole["rec"].tobytes()
    np.testing.assert_array_equal(tr, whole["trace"])
    assert so.tobytes() == whole["soft"].tobytes()
    # without the carry the second call starts a stream: exactly what the host twin says of it
    a2, b2 = two_calls(False)
    d2 = {k: np.ascontiguousarray(v[:, 3:]) for k, v in d.items()}
    fresh, _ = squelched_records(d2, np.ascontiguousarray(level[:, 3:]), None, MIN_SUMSQ, order)
    _same(a2, a)
    _same(b2, fresh)
    lost = (d["valid"][:, 3] != 0) & (level["sumsq"][:, 3] < MIN_SUMSQ) & (level["sumsq"][:, 2] >= MIN_SUMSQ)
    assert lost.any() and b["count"] - b2["count"] == int(lost.sum())


# ------------------------------------------------------------------ 12. the device form in stream order
def _device_call(rx, dx, prev, order, S):
    o = rx.demod_records_squelch_device(dx, MIN_SUMSQ, prev=prev, order=order, trace=True, soft=True, stream=S)
    with torch.cuda.stream(S):
        c = {k: v.clone() for k, v in o.items()}
        dx.zero_()   # behind the clones: work that ran late computes from, or leaves, something else
        for k, v in o.items():
            if k != "prev":
                v.view(torch.uint8).fill_(SENT)
    return c


@pytest.mark.parametrize("order", ORDERS)
def test_device_form_behind_a_delay(order):
    import oracle
    x, d, level = oracle_case(0)
    decoy = oracle.synth(9, 8, 8, 1000.0)   # another stream: a premature read gives plausible output
    exp, last = squelched_records(d, level, None, MIN_SUMSQ, order)
    first, _ = squelched_records({k: np.ascontiguousarray(v[:, :3]) for k, v in d.items()},
                                 np.ascontiguousarray(level[:, :3]), None, MIN_SUMSQ, order)
    second, _ = squelched_records({k: np.ascontiguousarray(v[:, 3:]) for k, v in d.items()},
                                  np.ascontiguousarray(level[:, 3:]), level[:, 2].copy(), MIN_SUMSQ, order)
    assert first["count"] + second["count"] == exp["count"]
    S = torch.cuda.Stream()
    rx = sc.Receiver(8)
    pins = [torch.from_numpy(np.ascontiguousarray(x[:, a:e])).pin_memory() for a, e in ((0, 3), (3, 8))]
    D = 100.0
    clones = running = delay = None
    for delay_ms in (None, D):   # the first pass is the warm-up: the delayed one grows and allocates nothing
        devs = [_dev(decoy[:, a:e]) for a, e in ((0, 3), (3, 8))]
        with torch.cuda.stream(S):
            prev = torch.zeros((8, 2), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        delay = gpu_delay.put(S, delay_ms) if delay_ms else None
        with torch.cuda.stream(S):
            for dev, pin in zip(devs, pins):   # the input arrives late, behind the delay
                dev.copy_(pin, non_blocking=True)
        clones = [_device_call(rx, dx, prev, order, S) for dx in devs]   # prev is carried on the device
        running = delay.running() if delay else None
        S.synchronize()
        rx.sync()
        if delay is None:
            rx.reset()
            del clones, devs
    assert delay.ms() >= 0.9 * D
    assert running, "the delay had ended when the last enqueue returned: a call waited for the stream"
    rx.close()
    for c, want, lv in zip(clones, (first, second), (level[:, :3], level[:, 3:])):
        count = int(c["count"].cpu().numpy().view(np.uint32)[0])
        got = {"count": count, "groups": c["groups"].cpu().numpy().view(np.uint32),
               "rec": sc.rec_from_tensor(c["rec"], count), "trace": c["trace"][:count].cpu().numpy(),
               "soft": c["soft"][:count].cpu().numpy()}
        _same(got, want)
        assert sc.level_from_tensor(c["level"]).tobytes() == np.ascontiguousarray(lv).tobytes()
    # prev as each call left it (cloned in stream order)
    assert sc.level_from_tensor(clones[0]["prev"]).tobytes() == level[:, 2].tobytes()
    assert sc.level_from_tensor(clones[1]["prev"]).tobytes() == level[:, 7].tobytes() == last.tobytes()


# ------------------------------------------------------------------ the C example
def test_example_squelch_option(tmp_path):
    """examples/qpsk_rx_raw -b -q DBFS: the idle channel's file is empty, the
    others hold the 496-byte records of their squelched frames; without -q the
    idle channel has a record per frame."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "qpsk_rx_raw")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.dirname(exe)], check=True)
    nch, nf = 3, 10
    x = sc.synth_device(45, nch, nf, 8.0).cpu().numpy()
    x[1] = 0
    x[2, 5:] = 0
    paths = []
    for i in range(nch):
        x[i].tofile(tmp_path / f"ch{i}.raw")
        paths.append(str(tmp_path / f"ch{i}.raw"))
    rx = sc.Receiver(nch)
    d = rx.demod(x)
    rx.close()
    assert d["valid"][1].all() and d["valid"][0].any()
    s = sc.squelch_host(sc.level_host(x), d["valid"], sc.sumsq_of_dbfs(-60.0))
    assert not s["valid"][1].any() and s["valid"][0].any() and s["valid"][2].sum() < d["valid"][2].sum()
    for opt, valid in (([], d["valid"]), (["-q", "-60"], s["valid"])):
        out = str(tmp_path / ("q" if opt else "p"))
        r = subprocess.run([exe, "-b", *opt, *paths, "-o", out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        for c in range(nch):
            assert open(f"{out}{c}.bin", "rb").read() == sc.records(d["bits"][c], valid[c]), (opt, c)


# ------------------------------------------------------------------ 13. refusals
def test_refusals_launch_nothing():
    L = sc.lib()
    x = torch.zeros(2 * sc.FRAME_SIZE + 8, dtype=torch.int16, device="cuda")
    x[:] = 1000
    out = torch.from_numpy(filled((4, 2), np.int64)).cuda()
    p, q, s = x.data_ptr(), out.data_ptr(), sc._stream(None, x.device)
    assert p % 16 == 0 and q % 16 == 0
    for d_in, d_out, n in ((p + 2, q, 1), (p + 8, q, 1), (p, q + 4, 1), (p, q + 2, 1), (None, q, 1), (p, None, 1),
                           (p, q, 1 << 28), (p, q, (1 << 64) - 1)):
        assert L.qpsk_level_device(d_in, n, d_out, s) == sc.QPSK_EINVAL, (d_in, d_out, n)
    assert L.qpsk_level_device(None, 0, None, s) == 0
    assert L.qpsk_level_device(p, 1, q + 8, s) == 0   # 8-byte alignment is enough for the output
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint8).reshape(-1)   # 64 bytes: the level at bytes 8 .. 24
    assert (o[:8] == SENT).all() and (o[24:] == SENT).all()
    assert o[8:24].tobytes() == sc.level_host(np.full((1, 1880), 1000, np.int16)).tobytes()
    # the squelch
    lv, v = out, torch.ones(2, dtype=torch.uint8, device="cuda")
    vo = torch.full((2,), SENT, dtype=torch.uint8, device="cuda")
    a, b, c = lv.data_ptr(), v.data_ptr(), vo.data_ptr()
    for args in ((None, None, 1, 2, 0, b, c, None, None, None), (a, None, 1, 2, 0, None, c, None, None, None),
                 (a, None, 1, 2, 0, b, None, None, None, None), (a + 4, None, 1, 2, 0, b, c, None, None, None),
                 (a, a + 4, 1, 2, 0, b, c, None, None, None), (a, None, 1, 2, 0, b, c, a + 1, None, None),
                 (a, None, 1, 2, 0, b, c, None, a + 4, None), (a, None, 1, 2, 0, b, c, None, None, a + 4),
                 (a, None, -1, 2, 0, b, c, None, None, None), (a, None, 1 << 14, 1 << 14, 0, b, c, None, None, None)):
        assert L.qpsk_squelch_device(*args, s) == sc.QPSK_EINVAL, args
    torch.cuda.synchronize()
    assert bool((vo == SENT).all())
    # the record call: nothing is received when a pointer is refused
    rx = sc.Receiver(2)
    dx = torch.zeros((2, 1, sc.FRAME_SIZE), dtype=torch.int16, device="cuda")
    cnt = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    lvl = torch.zeros((3, 2), dtype=torch.int64, device="cuda")
    for d_in, prev, level in ((dx.data_ptr() + 2, None, None), (dx.data_ptr(), lvl.data_ptr() + 4, None),
                              (dx.data_ptr(), None, lvl.data_ptr() + 4), (None, None, None)):
        assert L.qpsk_rx_batch_records_squelch_device(rx._h, d_in, 1, 1, prev, 0, 0, None, None, None, None,
                                                      cnt.data_ptr(), level, s) == sc.QPSK_EINVAL
    assert L.qpsk_rx_batch_records_squelch_device(rx._h, dx.data_ptr(), 1, 1, None, 2, 0, None, None, None, None,
                                                  cnt.data_ptr(), None, s) == sc.QPSK_EINVAL   # an unknown order
    n = C.c_uint32(5)
    hx = np.zeros((2, 1, sc.FRAME_SIZE), np.int16)
    assert L.qpsk_rx_batch_records_squelch(rx._h, hx.ctypes.data, 1, 1, None, 0, 1, None, None, None, None,
                                           C.addressof(n), None) == sc.QPSK_EINVAL   # cap without rec
    assert L.qpsk_rx_batch_records_squelch(rx._h, None, 1, 1, None, 0, 0, None, None, None, None, C.addressof(n),
                                           None) == sc.QPSK_EINVAL
    torch.cuda.synchronize()
    assert rx.frames == 0 and int(cnt.cpu()[0]) == 77 and n.value == 5
    # and a call of no frames is fine: an empty list, prev as it was
    got = rx.demod_records_squelch(np.zeros((2, 0, sc.FRAME_SIZE), np.int16), 5, prev=sc.level_host(hx)[:, 0])
    assert got["count"] == 0 and got["groups"].tolist() == [0, 0, 0] and got["level"].shape == (2, 0)
    assert got["prev"].tobytes() == bytes(32)
    rx.close()
