"""G.711 and timeslot-interleaved output on the GPU (include/qpsk_output.h): the
converter against its host twin, the transmitter in front of it against the
plain call, the loop back into the receive path with nothing but codes in
between, contexts, handles and the C examples.  Run with -m gpu."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

import oracle
import singlecarrier_amd as sc
from g711 import TABLES, compress
from rxcheck import assert_same, live_handles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xC3
GUARD = 64          # sentinel bytes between two blocks of an arena
PATH_PREPASS, PATH_FUSED = 0, 1   # csrc/qpsk_fmt_internal.h QPSK_OUT_PATH_*
PLANAR_CODES = [sc.OUT_ALAW | sc.OUT_PLANAR, sc.OUT_ULAW | sc.OUT_PLANAR]
INTERLEAVED = [sc.OUT_S16 | sc.OUT_INTERLEAVED, sc.OUT_ALAW | sc.OUT_INTERLEAVED, sc.OUT_ULAW | sc.OUT_INTERLEAVED]


def _es(fmt):
    return 2 if (fmt & 0x0f) == sc.OUT_S16 else 1


class Arena:
    """Destination blocks side by side in one sentinel-filled device buffer and
    in its host image.  A block is placed `offset` bytes past a 16-byte
    boundary with GUARD bytes of sentinel in front of it; the device side is
    written by the code under test, the host image by the expectation, and the
    two are compared whole: the guards, the row tails and the foreign columns
    are part of the comparison."""

    def __init__(self):
        self.size = GUARD
        self.dev = None

    def place(self, nbytes, offset):
        pos = (self.size + 15) // 16 * 16 + offset
        self.size = pos + nbytes + GUARD
        return pos

    def alloc(self):
        import torch
        self.dev = torch.full((self.size + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.base = (-self.dev.data_ptr()) % 16
        self.host = np.full(self.size, SENTINEL, np.uint8)

    def ptr(self, pos):
        return self.dev.data_ptr() + self.base + pos

    def view(self, pos, fmt, rows, cols, ld):
        """the block at pos as a strided torch tensor [rows][cols]"""
        import torch
        es = _es(fmt)
        n = ((rows - 1) * ld + cols) * es
        flat = self.dev[self.base + pos:self.base + pos + n]
        flat = flat.view(torch.int16) if es == 2 else flat
        return torch.as_strided(flat, (rows, cols), (ld, 1), flat.storage_offset())

    def expect(self, pos, fmt, want, ld):
        """want [rows][cols] elements at pos, rows ld apart, into the host image"""
        es = _es(fmt)
        rows, cols = want.shape
        raw = np.ascontiguousarray(want).view(np.uint8).reshape(rows, cols * es)
        n = ((rows - 1) * ld + cols) * es
        np.lib.stride_tricks.as_strided(self.host[pos:pos + n], (rows, cols * es), (ld * es, 1))[...] = raw

    def check(self, what=""):
        import torch
        torch.cuda.synchronize()
        got = self.dev[self.base:self.base + self.size].cpu().numpy()
        bad = np.nonzero(got != self.host)[0]
        assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at {int(bad[0])} of {self.size}"


def _ld_list(nch):
    """row strides of an interleaved block: the minimum, and one per store width
    16 / 8 / 4 / 2 / 1 of the kernel for codes at a 16-byte aligned address
    (16 / 16 / 8 / 4 / 2 for int16)"""
    r16 = (nch + 15) // 16 * 16
    return [nch, r16, r16 + 8, r16 + 4, r16 + 2, r16 + 1]


def _convert(fmt, d_src, src_ld, nch, n, dst_ptr, ld):
    import torch
    w = C.c_int(-1)
    s = torch.cuda.current_stream()
    sc._check(sc.lib().qpsk_output_convert_device_w(fmt, d_src.data_ptr(), src_ld, nch, n, dst_ptr, ld,
                                                    C.c_void_p(s.cuda_stream), C.byref(w)))
    return w.value


def _host_block(x, fmt, ld):
    """the host twin's block [rows][cols] of x [nch][n]"""
    nch, n = x.shape
    cols = nch if fmt & 0x10 else n
    return sc.output_convert_host(x, fmt, ld=ld)[:, :cols]


@pytest.mark.parametrize("n", [1, 127, 128, 129, 2 * 2783])
@pytest.mark.parametrize("nch", [1, 63, 64, 65, 130])
def test_converter_equals_the_host_twin(nch, n):
    """every format; source rows n, n + 1 and n + 5 apart; the destination at
    every byte offset 0..15 (codes) and 0, 2, 6 (int16) past a 16-byte
    boundary; planar ld = n and n + 3; interleaved ld = nch and one value per
    store width.  All five store widths run for codes, four for int16, in every
    case; nothing outside the blocks' elements changes."""
    import torch
    rng = np.random.default_rng(1000 * nch + n)
    x = rng.integers(-32768, 32768, (nch, n), dtype=np.int16)
    x[0, 0], x[-1, -1] = -32768, 32767
    srcs = {}
    for sld in (n, n + 1, n + 5):
        wide = rng.integers(-32768, 32768, (nch, sld), dtype=np.int16)
        wide[:, :n] = x
        srcs[sld] = torch.from_numpy(wide).cuda()
    slds = sorted(srcs)
    for fmt in PLANAR_CODES + INTERLEAVED:
        es, inter = _es(fmt), bool(fmt & 0x10)
        offsets = (0, 2, 6) if es == 2 else range(16)
        lds = _ld_list(nch) if inter else [n, n + 3]
        rows, cols = (n, nch) if inter else (nch, n)
        arena, jobs, widths = Arena(), [], set()
        blocks = {ld: _host_block(x, fmt, ld) for ld in lds}
        for k, off in enumerate(offsets):
            for j, ld in enumerate(lds):
                if inter and off and j >= 2:
                    continue   # every offset with the minimum and an aligned ld, the other strides at offset 0
                for sld in (slds if (not inter or off == 0) else [slds[(k + j) % 3]]):
                    jobs.append((arena.place(sc.output_bytes(fmt, nch, n, ld), off), ld, sld))
        arena.alloc()
        for pos, ld, sld in jobs:
            assert arena.ptr(pos) % 16 == (pos % 16)
            w = _convert(fmt, srcs[sld], sld, nch, n, arena.ptr(pos), ld)
            assert w == (sc.lib().qpsk_output_store_width(arena.ptr(pos), ld, es) if inter else 0)
            widths.add(w)
            arena.expect(pos, fmt, blocks[ld], ld)
        arena.check(f"fmt {fmt:#x} nch {nch} n {n}")
        assert widths == ({0} if not inter else {16, 8, 4, 2} if es == 2 else {16, 8, 4, 2, 1}), (hex(fmt), widths)


def test_every_store_width_of_the_interleaved_kernel():
    """the store width follows the alignment of the block and of its row
    stride; each width is a kernel of its own"""
    import torch
    rng = np.random.default_rng(5)
    nch, n = 65, 300
    x = rng.integers(-32768, 32768, (nch, n), dtype=np.int16)
    d = torch.from_numpy(x).cuda()
    seen = {1: set(), 2: set()}
    for fmt, ld, off, width in [(sc.OUT_ALAW, 80, 0, 16), (sc.OUT_ALAW, 72, 0, 8), (sc.OUT_ULAW, 300, 0, 4),
                                (sc.OUT_ULAW, 70, 0, 2), (sc.OUT_ALAW, 80, 8, 8), (sc.OUT_ALAW, 80, 3, 1),
                                (sc.OUT_ALAW, 131, 0, 1), (sc.OUT_S16, 80, 0, 16), (sc.OUT_S16, 300, 0, 8),
                                (sc.OUT_S16, 70, 0, 4), (sc.OUT_S16, 131, 0, 2), (sc.OUT_S16, 80, 2, 2)]:
        fmt |= sc.OUT_INTERLEAVED
        arena = Arena()
        pos = arena.place(sc.output_bytes(fmt, nch, n, ld), off)
        arena.alloc()
        assert _convert(fmt, d, n, nch, n, arena.ptr(pos), ld) == width
        arena.expect(pos, fmt, _host_block(x, fmt, ld), ld)
        arena.check(f"fmt {fmt:#x} ld {ld} offset {off}")
        seen[_es(fmt)].add(width)
    assert seen == {1: {16, 8, 4, 2, 1}, 2: {16, 8, 4, 2}}


def test_python_converter_into_a_column_range_on_a_stream():
    """sc.output_convert_device into timeslots 3..132 of a 140-wide trunk, on a
    stream of its own; planar int16 with rows apart is a strided copy"""
    import torch
    rng = np.random.default_rng(6)
    x = rng.integers(-32768, 32768, (130, 257), dtype=np.int16)
    d = torch.from_numpy(x).cuda()
    s = torch.cuda.Stream()
    trunk = torch.full((257, 140), SENTINEL, dtype=torch.uint8, device="cuda")
    rows = torch.full((130, 300), 0x5A5A, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    sc.output_convert_device(d, sc.OUT_ULAW | sc.OUT_INTERLEAVED, trunk[:, 3:133], stream=s)
    sc.output_convert_device(d, sc.OUT_S16 | sc.OUT_PLANAR, rows[:, :257], stream=s)
    s.synchronize()
    want = np.full((257, 140), SENTINEL, np.uint8)
    want[:, 3:133] = compress(x, sc.OUT_ULAW).T
    np.testing.assert_array_equal(trunk.cpu().numpy(), want)
    want = np.full((130, 300), 0x5A5A, np.int16)
    want[:, :257] = x
    np.testing.assert_array_equal(rows.cpu().numpy(), want)


# ------------------------------------------------------------------ the kernels' loops
@pytest.mark.parametrize("fmt", PLANAR_CODES)
def test_planar_kernel_loops_over_more_than_65535_rows(fmt):
    """65,537 rows of 40 samples, src_ld = 41 and ld = 43 (not flat, so rows stay
    rows): grid.y is capped at 65,535 and rows 65,535 and 65,536 are the second
    round of planar_kernel's row loop.  Destination 0 and 5 bytes past a 16-byte
    boundary; with ld = 43 the rows take every offset either way."""
    import torch
    nch, n, sld, ld = 65537, 40, 41, 43
    rng = np.random.default_rng(65537)
    wide = rng.integers(-32768, 32768, (nch, sld), dtype=np.int16)
    x = wide[:, :n]
    d = torch.from_numpy(wide).cuda()
    want = _host_block(x, fmt, ld)
    arena, jobs = Arena(), []
    for off in (0, 5):
        jobs.append(arena.place(sc.output_bytes(fmt, nch, n, ld), off))
    arena.alloc()
    for pos in jobs:
        assert _convert(fmt, d, sld, nch, n, arena.ptr(pos), ld) == 0
        arena.expect(pos, fmt, want, ld)
    arena.check(f"fmt {fmt:#x}: {nch} rows")


@pytest.mark.parametrize("fmt", [sc.OUT_ALAW | sc.OUT_INTERLEAVED, sc.OUT_S16 | sc.OUT_INTERLEAVED])
def test_interleaved_kernel_loops_over_more_than_2_to_20_tiles(fmt):
    """one channel, 128 * 2^20 + 129 samples: 2^20 + 2 tiles of 128 samples, the
    last of one sample, on a grid capped at 2^20 blocks, so blocks 0 and 1 take
    a second tile.  The source repeats a block of prime length, so a tile taken
    from the wrong place differs."""
    import torch
    n, L = 128 * 2**20 + 129, 1_000_003
    assert (n + 127) // 128 == 2**20 + 2
    block = np.random.default_rng(20).integers(-32768, 32768, L, dtype=np.int16)
    x = np.resize(block, n)[None]
    d = torch.from_numpy(x).cuda()
    arena = Arena()
    pos = arena.place(sc.output_bytes(fmt, 1, n, 1), 0)
    arena.alloc()
    assert _convert(fmt, d, n, 1, n, arena.ptr(pos), 1) == _es(fmt)   # ld = 1 element: the narrowest store
    arena.expect(pos, fmt, _host_block(x, fmt, 1), 1)
    arena.check(f"fmt {fmt:#x}: {n} samples of one channel")
    del d, arena
    torch.cuda.empty_cache()


def test_planar_kernel_loops_over_more_than_2_to_28_units():
    """one flat row of 2^32 + 4,103 samples: 2^28 + 257 units of 16 codes on a
    grid of 2^20 blocks x 256 lanes, so the lanes of the first two blocks take a
    second unit, at element indices past 2^32.  Source and expectation repeat a
    block of prime length on the device; the block's codes are the host twin's.
    The destination starts 5 bytes past a 16-byte boundary.  Needs about 17 GB
    of device memory: skipped below 24 GiB free, never shrunk (below 2^28 units
    the loop does not iterate)."""
    import torch
    fmt, n, L, off = sc.OUT_ALAW | sc.OUT_PLANAR, 2**32 + 4103, 1_000_003, 5
    assert (off + n + 15) // 16 > 2**28
    if torch.cuda.mem_get_info()[0] < 24 * 2**30:
        pytest.skip("needs about 17 GB of device memory")
    block = np.random.default_rng(28).integers(-32768, 32768, L, dtype=np.int16)
    codes = sc.output_convert_host(block[None], fmt)[0]
    src = full = blk = exp = out = None
    try:
        reps = -(-n // L)
        src = torch.from_numpy(block).cuda().repeat(reps)[:n].view(1, n)
        full = torch.full((GUARD + 16 + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        start = GUARD + (off - full.data_ptr() - GUARD) % 16
        out = full[start:start + n].view(1, n)
        assert out.data_ptr() % 16 == off
        sc.output_convert_device(src, fmt, out)
        torch.cuda.synchronize()
        assert bool((full[:start] == SENTINEL).all()) and bool((full[start + n:] == SENTINEL).all()), "wrote outside n"
        blk = torch.from_numpy(codes).cuda()
        step = 2**26
        for lo in range(0, n, step):
            hi = min(lo + step, n)
            exp = blk[torch.arange(lo, hi, device="cuda") % L]
            assert torch.equal(out[0, lo:hi], exp), f"codes [{lo}, {hi}) of {n} differ (units {lo // 16}..)"
    finally:
        del src, full, blk, exp, out
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ the transmitter in front of it
def _plain(tx, d_bits, N):
    """the plain call's block from the start state, as numpy [nch][N]"""
    import torch
    out = torch.zeros((tx.nch, N), dtype=torch.int16, device="cuda")
    tx.reset()
    tx.modulate_device(d_bits, out)
    tx.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("gap", [0, 1, 903])
@pytest.mark.parametrize("npk", [1, 3])
@pytest.mark.parametrize("nch", [1, 7, 9, 129, 300])
def test_modulate_device_fmt_equals_the_compressed_plain_call(nch, npk, gap):
    """planar codes with rows N, N + 1 and N + 5 apart at all 8 byte offsets of
    a row's alignment class, and the three interleaved formats, against this
    file's compression of modulate_device's samples"""
    import torch
    rng = np.random.default_rng(nch * 100 + npk * 10 + gap)
    bits = rng.integers(0, 2, (nch, npk, 8, 62), dtype=np.uint8)
    d_bits = torch.from_numpy(bits).cuda()
    N = npk * (1880 + gap)
    tx = sc.Transmitter(nch, gap=gap)
    x = _plain(tx, d_bits, N)
    np.testing.assert_array_equal(x, sc.tx_batch_host(bits, gap=gap))
    arena, jobs = Arena(), []
    for fmt in PLANAR_CODES:
        for off in range(8):
            for ld in (N, N + 1, N + 5):
                # the default (the fused store of tx_batch_kernel) and both paths by name
                for path in (None, PATH_PREPASS, PATH_FUSED):
                    jobs.append((fmt, arena.place(sc.output_bytes(fmt, nch, N, ld), off), ld, path))
    for fmt in INTERLEAVED:
        for ld, off in ((nch, 0), (nch + 4, 2)):
            jobs.append((fmt, arena.place(sc.output_bytes(fmt, nch, N, ld), off), ld, None))
    arena.alloc()
    s = torch.cuda.current_stream()
    for fmt, pos, ld, path in jobs:
        rows, cols = (N, nch) if fmt & 0x10 else (nch, N)
        want = compress(x, fmt & 0x0f)
        tx.reset()
        if path is None:
            tx.modulate_device_fmt(d_bits, arena.view(pos, fmt, rows, cols, ld), fmt, ld)
        else:
            sc._check(sc.lib().qpsk_tx_batch_device_fmt_path(tx._h, d_bits.data_ptr(), npk, arena.ptr(pos), fmt, ld,
                                                            C.c_void_p(s.cuda_stream), path))
        assert tx.packets() == npk
        arena.expect(pos, fmt, want.T if fmt & 0x10 else want, ld)
    # a path the format has not is refused
    for fmt in INTERLEAVED:
        assert sc.lib().qpsk_tx_batch_device_fmt_path(tx._h, d_bits.data_ptr(), npk, arena.ptr(jobs[0][1]), fmt, nch,
                                                      None, PATH_FUSED) == sc.QPSK_EINVAL
    tx.sync()
    arena.check(f"nch {nch} npk {npk} gap {gap}")
    tx.close()


@pytest.mark.parametrize("fmt", [sc.OUT_ALAW | sc.OUT_PLANAR, sc.OUT_ULAW | sc.OUT_INTERLEAVED,
                                 sc.OUT_S16 | sc.OUT_INTERLEAVED])
def test_calls_of_1_3_1_packets_equal_one_of_5(fmt):
    """the carried state advances as in the plain call; reset() gives the first
    call's block again; packets() counts"""
    import torch
    nch, gap = 9, 903
    P = 1880 + gap
    bits = np.random.default_rng(77).integers(0, 2, (nch, 5, 8, 62), dtype=np.uint8)
    inter = bool(fmt & 0x10)
    dt = torch.int16 if _es(fmt) == 2 else torch.uint8

    def run(tx, part):
        d_bits = torch.from_numpy(np.ascontiguousarray(part)).cuda()
        n = part.shape[1] * P
        out = torch.zeros((n, nch) if inter else (nch, n), dtype=dt, device="cuda")
        tx.modulate_device_fmt(d_bits, out, fmt)
        tx.sync()
        return out.cpu().numpy()

    tx = sc.Transmitter(nch, gap=gap)
    whole = run(tx, bits)
    assert tx.packets() == 5
    want = compress(sc.tx_batch_host(bits, gap=gap), fmt & 0x0f)
    np.testing.assert_array_equal(whole, want.T if inter else want)
    tx.reset()
    assert tx.packets() == 0
    parts, seen = [], []
    for lo, hi in ((0, 1), (1, 4), (4, 5)):
        parts.append(run(tx, bits[:, lo:hi]))
        seen.append(tx.packets())
    assert seen == [1, 4, 5]
    np.testing.assert_array_equal(np.concatenate(parts, axis=0 if inter else 1), whole)
    tx.reset()
    np.testing.assert_array_equal(run(tx, bits[:, :1]), parts[0])
    tx.close()


def test_modulate_fmt_equals_the_device_result_and_spares_foreign_columns():
    """the host call: every format against the compressed plain host call; an
    interleaved trunk of ld = nch + 4 keeps its 4 foreign columns, a planar
    block of ld = N + 3 its row tails"""
    nch, npk, gap = 37, 2, 903
    N = npk * (1880 + gap)
    bits = np.random.default_rng(12).integers(0, 2, (nch, npk, 8, 62), dtype=np.uint8)
    tx = sc.Transmitter(nch, gap=gap)
    x = tx.modulate(bits)
    for fmt in PLANAR_CODES + INTERLEAVED + [sc.OUT_S16 | sc.OUT_PLANAR]:
        inter, es = bool(fmt & 0x10), _es(fmt)
        want = compress(x, fmt & 0x0f)
        want = want.T if inter else want
        rows, cols = want.shape
        tx.reset()
        np.testing.assert_array_equal(tx.modulate_fmt(bits, fmt), want, err_msg=hex(fmt))
        ld = cols + (4 if inter else 3)
        fill = 0x5A5A if es == 2 else SENTINEL
        out = np.full((rows, ld), fill, np.int16 if es == 2 else np.uint8)
        tx.reset()
        assert tx.modulate_fmt(bits, fmt, ld=ld, out=out) is out
        np.testing.assert_array_equal(out[:, :cols], want, err_msg=hex(fmt))
        assert (out[:, cols:] == fill).all(), hex(fmt)
        assert tx.packets() == npk
    tx.close()


# ------------------------------------------------------------------ loopback
@pytest.fixture(scope="module")
def loop():
    """24 channels x 6 packets at the reference gap: the payload, the host
    twin's samples cut to 8 frames, and per G.711 encoding the oracle's receive
    of expand(compress(samples)) by this suite's own formulas and tables"""
    bits = np.random.default_rng(31).integers(0, 2, (24, 6, 8, 62), dtype=np.uint8)
    x = sc.tx_batch_host(bits, gap=903)[:, :8 * 1880]
    exp = {}
    for enc in (sc.OUT_ALAW, sc.OUT_ULAW):
        y = TABLES[enc][compress(x, enc)].astype(np.int16).reshape(24, 8, 1880)
        b, v, tr = oracle.cpu_rx(y, trace=True)
        # at least 48 of the 192 channel-frames valid: the comparison is not empty
        assert int(v.sum()) >= 48
        exp[enc] = (b, v, tr)
    return bits, exp


@pytest.mark.parametrize("enc", [sc.OUT_ALAW, sc.OUT_ULAW])
def test_loopback_through_an_interleaved_trunk_of_codes(loop, enc):
    """modulate_device_fmt into an interleaved device trunk, whose first
    8 x 1880 rows go to demod_device_fmt as they are"""
    import torch
    bits, exp = loop
    fmt = enc | sc.OUT_INTERLEAVED
    tx, rx = sc.Transmitter(24, gap=903), sc.Receiver(24)
    trunk = torch.zeros((6 * 2783, 24), dtype=torch.uint8, device="cuda")
    tx.modulate_device_fmt(torch.from_numpy(bits).cuda(), trunk, fmt)
    out = {"bits": torch.zeros((24, 8, sc.NBITS), dtype=torch.uint8, device="cuda"),
           "valid": torch.zeros((24, 8), dtype=torch.uint8, device="cuda"),
           "trace": torch.zeros((24, 8, 4), dtype=torch.int32, device="cuda"),
           "soft": torch.zeros((24, 8, sc.DATA_SYMBOLS, 2), dtype=torch.float32, device="cuda")}
    rx.demod_device_fmt(trunk[:8 * 1880], fmt, out["bits"], out["valid"], out["trace"], out["soft"])
    rx.sync()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert_same(out, exp[enc], hex(fmt))
    tx.close()
    rx.close()


# ------------------------------------------------------------------ other contexts
def test_two_contexts_on_two_streams_in_different_formats():
    import torch
    nch, gap, N = 70, 1, 3 * 1881
    rng = np.random.default_rng(3)
    b = [rng.integers(0, 2, (nch, 3, 8, 62), dtype=np.uint8) for _ in range(2)]
    fmts = [sc.OUT_ALAW | sc.OUT_INTERLEAVED, sc.OUT_ULAW | sc.OUT_PLANAR]
    txs = [sc.Transmitter(nch, gap=gap) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = [torch.zeros((N, nch), dtype=torch.uint8, device="cuda"),
            torch.zeros((nch, N), dtype=torch.uint8, device="cuda")]
    d = [torch.from_numpy(x).cuda() for x in b]
    torch.cuda.synchronize()
    for k in range(2):
        txs[k].modulate_device_fmt(d[k], outs[k], fmts[k], stream=streams[k])
    for k in range(2):
        txs[k].sync()
        want = compress(sc.tx_batch_host(b[k], gap=gap), fmts[k] & 0x0f)
        np.testing.assert_array_equal(outs[k].cpu().numpy(), want.T if fmts[k] & 0x10 else want)
        txs[k].close()


def test_default_format_calls_are_unaffected_and_handles_return():
    """a format call in front of plain calls changes nothing of them; a closed
    context that went through the format paths leaves no handle alive"""
    import torch
    nch, gap = 20, 903
    bits = np.random.default_rng(14).integers(0, 2, (nch, 3, 8, 62), dtype=np.uint8)
    want = sc.tx_batch_host(bits, gap=gap)
    gc.collect()
    base = live_handles()
    tx = sc.Transmitter(nch, gap=gap)
    first = tx.modulate_fmt(bits[:, :1], sc.OUT_ALAW | sc.OUT_INTERLEAVED)
    np.testing.assert_array_equal(first, compress(want[:, :2783], sc.OUT_ALAW).T)
    # the stream goes on in the plain calls, host and device
    np.testing.assert_array_equal(tx.modulate(bits[:, 1:2]), want[:, 2783:2 * 2783])
    out = torch.zeros((nch, 2783), dtype=torch.int16, device="cuda")
    tx.modulate_device(torch.from_numpy(np.ascontiguousarray(bits[:, 2:])).cuda(), out)
    tx.sync()
    np.testing.assert_array_equal(out.cpu().numpy(), want[:, 2 * 2783:])
    codes = torch.zeros((nch, 2783), dtype=torch.uint8, device="cuda")
    tx.reset()
    tx.modulate_device_fmt(torch.from_numpy(np.ascontiguousarray(bits[:, :1])).cuda(), codes, sc.OUT_ULAW)
    tx.sync()
    assert live_handles() > base
    tx.close()
    assert live_handles() == base


# ------------------------------------------------------------------ the C examples
def test_c_drivers_write_and_read_an_alaw_trunk(loop, tmp_path):
    """examples/qpsk_tx_raw -b -f alaw -i writes a trunk file of 24 timeslots;
    examples/qpsk_rx_stream -f alaw -i 24 reads it and gives the oracle's
    records of its first 8 frames"""
    bits, exp = loop
    want_bits, want_valid, _ = exp[sc.OUT_ALAW]
    paths = []
    for c in range(24):
        paths.append(str(tmp_path / f"ch{c}.bits"))
        bits[c].tofile(paths[-1])
    trunk = tmp_path / "trunk.al"
    r = subprocess.run([os.path.join(ROOT, "examples", "qpsk_tx_raw"), "-b", "-f", "alaw", "-i", *paths, "-o",
                        str(trunk)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(trunk, np.uint8).reshape(6 * 2783, 24)
    np.testing.assert_array_equal(got, compress(sc.tx_batch_host(bits, gap=903), sc.OUT_ALAW).T)
    pre = tmp_path / "r_"
    r = subprocess.run([os.path.join(ROOT, "examples", "qpsk_rx_stream"), "-f", "alaw", "-i", "24", str(trunk), "-o",
                        str(pre)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    total = 0
    for c in range(24):
        want = sc.records(want_bits[c], want_valid[c])
        total += len(want)
        assert open(f"{pre}{c}.bin", "rb").read() == want, c
    assert total >= 48 * 496
