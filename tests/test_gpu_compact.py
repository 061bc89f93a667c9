"""The record layer on the GPU (include/qpsk_compact.h, csrc/qpsk_compact.hip)
against its host twin, byte for byte: records, gathered trace and soft rows,
groups, count, and the sentinel fill past min(count, cap) rows.  The inputs are
synthetic dense arrays; no receive runs here.  Run with -m gpu.

The shapes sit at the edges of the kernels' tiling (csrc/qpsk_compact_tile.h,
read through sc.compact_tiling()): RUN items are one wave's run and one count
of the work area, BLOCK items one workgroup, and the scan's one workgroup takes
TRIP counts per trip of its loop.

The gather copies a soft row as 62 dwords and a trace row as 4, one lane each,
so the only alignment it asks for is the element's own 4 bytes; the alignment
cases place every row array at each of the four dword positions of a 16-byte
line."""
import numpy as np
import pytest

import singlecarrier_amd as sc
from compact_cases import SENT, filled, random_dense

pytestmark = pytest.mark.gpu

T = sc.compact_tiling()
RUN, BLOCK, TRIP = T["run_items"], T["block_items"], T["scan_trip"]
ORDERS = [sc.REC_BY_CHANNEL, sc.REC_BY_FRAME]


def _dev_bytes(nbytes, k=0):
    """nbytes of sentinel on the device, starting 4 * k bytes past a 16-byte line"""
    import torch
    buf = torch.full((nbytes + 32,), SENT, dtype=torch.uint8, device="cuda")
    base = (-buf.data_ptr()) % 16 + 4 * k
    return buf[base:base + nbytes]


def _dev_copy(a, k=0):
    """a numpy array on the device as bytes, starting 4 * k bytes past a 16-byte line"""
    import torch
    t = _dev_bytes(a.nbytes, k)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)))
    return t


class Dev:
    """The dense arrays of a case on the device, and its work area (poisoned)."""

    def __init__(self, d, offs=(0, 0)):
        import torch
        self.d = d
        bits, valid, trace, soft = d
        self.nch, self.nf = valid.shape
        self.bits, self.valid = _dev_copy(bits), _dev_copy(valid)
        self.trace, self.soft = _dev_copy(trace, offs[0]), _dev_copy(soft, offs[1])
        self.work = torch.full((sc.compact_work_bytes(self.nch, self.nf),), 0xFF, dtype=torch.uint8, device="cuda")


def _view(t, nch, nf):
    return t   # compact_device takes the pointers; the shape comes from valid


def run_case(dv, order, cap, rows=True, offs=(0, 0), groups=True):
    """One device call into sentinel-filled outputs, compared whole with the
    host twin's on the same fill.  Returns count."""
    import torch
    bits, valid, trace, soft = dv.d
    nch, nf = dv.nch, dv.nf
    G = nf if order == sc.REC_BY_FRAME else nch
    host = filled(cap, G)
    if not rows:
        del host["trace"], host["soft"]
    if not groups:
        del host["groups"]
    host = sc.compact_host(bits, valid, trace if rows else None, soft if rows else None, order=order, cap=cap,
                           out=host)
    rec = _dev_bytes(cap * 16)
    rtr = _dev_bytes(cap * 16, offs[0]) if rows else None
    rso = _dev_bytes(cap * 248, offs[1]) if rows else None
    grp = _dev_bytes((G + 1) * 4) if groups else None
    cnt = _dev_bytes(4)
    sc.compact_device(dv.bits, dv.valid.view(nch, nf), dv.trace if rows else None, dv.soft if rows else None,
                      order=order, cap=cap, rec=rec if cap else None, rec_trace=rtr, rec_soft=rso, groups=grp,
                      count=cnt, work=dv.work)
    torch.cuda.synchronize()
    count = int(cnt.cpu().numpy().view(np.uint32)[0])
    assert count == host["count"] == int((valid != 0).sum())
    np.testing.assert_array_equal(rec.cpu().numpy(), host["rec"].view(np.uint8).reshape(-1))
    if rows:
        np.testing.assert_array_equal(rtr.cpu().numpy(), host["trace"].view(np.uint8).reshape(-1))
        np.testing.assert_array_equal(rso.cpu().numpy(), host["soft"].view(np.uint8).reshape(-1))
    if groups:
        np.testing.assert_array_equal(grp.cpu().numpy().view(np.uint32), host["groups"])
    return count


def make(seed, nch, nf, pattern):
    rng = np.random.default_rng(seed)
    bits, valid, trace, soft = random_dense(rng, nch, nf, 0.2, odd_bytes=True)
    if pattern == "all":
        valid[:] = 1
    elif pattern == "none":
        valid[:] = 0
    elif pattern == "first":
        valid[:] = 0
        valid.reshape(-1)[0] = 1
    elif pattern == "last":
        valid[:] = 0
        valid.reshape(-1)[-1] = 1
    else:
        assert pattern == "random"
    return bits, valid, trace, soft


ITEMS = [1, 63, 64, 65, RUN - 1, RUN, RUN + 1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + RUN + 7]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n", ITEMS)
def test_item_counts_at_the_tiling_edges(n, order):
    """n items as one group of n and as n groups of one, 20 % valid; the work
    area is poisoned, and the second call runs on what the first left in it."""
    for nch, nf in ((1, n), (n, 1)):
        dv = Dev(make(n, nch, nf, "random"))
        count = run_case(dv, order, n)
        assert run_case(dv, order, n) == count


@pytest.mark.parametrize("order", ORDERS)
def test_one_more_count_than_a_scan_trip(order):
    """TRIP + 1 runs: the scan's workgroup goes round its loop twice, and the
    last run holds one item."""
    n = TRIP * RUN + 1
    assert sc.compact_work_bytes(n, 1) == 4 * (TRIP + 1)
    d = make(9, n, 1, "random")
    d[1].reshape(-1)[-1] = 1   # the lone item of the last run counts
    dv = Dev(d)
    count = run_case(dv, order, n, rows=False)
    assert run_case(dv, order, 100, rows=False) == count
    d = make(10, n, 1, "last")
    assert run_case(Dev(d), order, 4, rows=False) == 1


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("nf", [1, 2, 33])
@pytest.mark.parametrize("nch", [1, 63, 65, 257])
def test_ragged_channel_and_frame_counts(nch, nf, order):
    """by-frame order walks valid[c * nf + f] with c fastest: the strided walk
    over waves that end inside a frame's channels"""
    run_case(Dev(make(nch * 100 + nf, nch, nf, "random")), order, nch * nf)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("pattern", ["all", "none", "first", "last", "random"])
@pytest.mark.parametrize("nch,nf", [(65, 33), (BLOCK + 1, 1), (3, RUN + 1)])
def test_patterns_and_caps(nch, nf, pattern, order):
    dv = Dev(make(17, nch, nf, pattern))
    count = run_case(dv, order, nch * nf)
    for cap in sorted({0, max(count - 1, 0), count, count + 5}):
        assert run_case(dv, order, cap) == count


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("cap", [1, 10, 63])
def test_all_valid_with_cap_below_one_wave(cap, order):
    dv = Dev(make(3, 5, 40, "all"))
    assert run_case(dv, order, cap) == 200


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("k_soft", [0, 1, 2, 3])
@pytest.mark.parametrize("k_trace", [0, 1, 2, 3])
def test_rows_at_every_dword_alignment(k_trace, k_soft, order):
    """dense and gathered trace / soft arrays 4 * k bytes past a 16-byte line"""
    dv = Dev(make(21, 37, 9, "random"), offs=(k_trace, k_soft))
    run_case(dv, order, 37 * 9, offs=(k_soft, k_trace))   # the outputs the other way round


@pytest.mark.parametrize("order", ORDERS)
def test_pure_count_and_missing_outputs(order):
    import torch
    d = make(31, 70, 30, "random")
    dv = Dev(d)
    count = run_case(dv, order, 0, rows=False, groups=False)   # NULL records, NULL groups
    assert count == int((d[1] != 0).sum())
    run_case(dv, order, 0, rows=False)                         # groups alone
    run_case(dv, order, 70 * 30, rows=False)                   # records without rows
    # a gathered array without its dense source stays as it was
    rtr = _dev_bytes(70 * 30 * 16)
    sc.compact_device(dv.bits, dv.valid.view(70, 30), None, None, order=order, rec_trace=rtr, work=dv.work)
    torch.cuda.synchronize()
    assert bool((rtr == SENT).all())


def test_no_items():
    import torch
    for nch, nf in ((0, 5), (5, 0)):
        for order in ORDERS:
            G = nf if order == sc.REC_BY_FRAME else nch
            grp, cnt = _dev_bytes((G + 1) * 4), _dev_bytes(4)
            valid = torch.zeros((nch, nf), dtype=torch.uint8, device="cuda")
            bits = torch.zeros((nch, nf, 62), dtype=torch.uint8, device="cuda")
            sc.compact_device(bits, valid, order=order, cap=0, groups=grp, count=cnt,
                              work=torch.zeros(4, dtype=torch.uint8, device="cuda"))
            torch.cuda.synchronize()
            assert not bool(cnt.any()) and not bool(grp.any())


def test_pack_device_equals_the_host_packer():
    import torch
    rng = np.random.default_rng(4)
    for n in (1, 3, 4, 5, 1000, 4 * 4096 + 3):
        bits = rng.integers(0, 2, (n, 62), dtype=np.uint8)
        bits[rng.random(bits.shape) < 0.1] = 2
        bits[rng.random(bits.shape) < 0.1] = 255
        bits[0] = 0   # an invalid frame's row
        w = sc.pack_bits_device(torch.from_numpy(bits).cuda())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(w.cpu().numpy().view(np.uint64), sc.pack_bits(bits))
    assert sc.pack_bits_device(torch.zeros((0, 62), dtype=torch.uint8, device="cuda")).shape == (0,)


@pytest.mark.parametrize("n", [1, 5])
def test_pack_device_writes_its_words_and_nothing_else(n):
    """d_words 8 bytes past a 16-byte line (its stated alignment) inside a
    sentinel-filled buffer, 256 guard bytes on both sides: n words are written,
    the guards stay.  A pointer 4 bytes further is refused."""
    import torch
    guard = 256
    rng = np.random.default_rng(40 + n)
    bits = rng.integers(0, 2, (n, 62), dtype=np.uint8)
    d_bits = torch.from_numpy(bits).cuda()
    for fill in (SENT, SENT ^ 0xFF):
        raw = torch.full((2 * guard + 8 * n + 32,), fill, dtype=torch.uint8, device="cuda")
        base = (-raw.data_ptr()) % 16
        buf = raw[base:base + 2 * guard + 8 * n + 8]
        off = guard + 8
        assert (buf.data_ptr() + off) % 16 == 8
        img = np.full(buf.numel(), fill, np.uint8)
        rc = sc.lib().qpsk_bits_pack_device(d_bits.data_ptr(), n, buf.data_ptr() + off + 4, None)
        assert rc == sc.QPSK_EINVAL
        torch.cuda.synchronize()
        np.testing.assert_array_equal(buf.cpu().numpy(), img)
        sc.pack_bits_device(d_bits, out=buf[off:off + 8 * n].view(torch.int64))
        torch.cuda.synchronize()
        img[off:off + 8 * n] = sc.pack_bits(bits).view(np.uint8)
        np.testing.assert_array_equal(buf.cpu().numpy(), img)


@pytest.mark.parametrize("order", ORDERS)
def test_offsets_past_32_bits(order):
    """70 M items: an item's bits row starts past 2^32 bytes (62 * n = 4.3 GB).
    The expectation is torch's, on the device: nonzero for the order, the
    rows' (== 1) shifted and summed in int64."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip("needs 12 GiB of free device memory")
    nch, nf = 2187500, 32
    n = nch * nf
    assert n * 62 > 1 << 32 and n < 1 << 28
    g = torch.Generator(device="cuda").manual_seed(7)
    bits = torch.empty((nch, nf, 62), dtype=torch.uint8, device="cuda")
    flat = bits.view(-1)
    step = 1 << 28
    for o in range(0, flat.numel(), step):   # filled in pieces: no 4 GB temporary
        m = min(step, flat.numel() - o)
        flat[o:o + m] = torch.randint(0, 3, (m,), dtype=torch.uint8, device="cuda", generator=g)
    valid = (torch.rand((nch, nf), device="cuda", generator=g) < 0.005).to(torch.uint8)
    valid[-1, -1] = 1   # the very last item: the highest offset
    count = int(valid.sum())
    assert 0 < count < 1 << 20
    o = sc.compact_device(bits, valid, order=order, cap=count + 3)
    torch.cuda.synchronize()
    if order == sc.REC_BY_FRAME:
        fc = torch.nonzero(valid.t().contiguous())
        f, c = fc[:, 0], fc[:, 1]
        per = valid.sum(dim=0, dtype=torch.int64)
    else:
        cf = torch.nonzero(valid)
        c, f = cf[:, 0], cf[:, 1]
        per = valid.sum(dim=1, dtype=torch.int64)
    rows = bits.view(n, 62)[c * nf + f]
    words = ((rows == 1).to(torch.int64) << torch.arange(62, device="cuda", dtype=torch.int64)).sum(dim=1)
    assert int(o["count"].cpu().numpy().view(np.uint32)[0]) == count
    rec = sc.rec_from_tensor(o["rec"], count)
    np.testing.assert_array_equal(rec["channel"], c.cpu().numpy().astype(np.uint32))
    np.testing.assert_array_equal(rec["frame"], f.cpu().numpy().astype(np.uint32))
    np.testing.assert_array_equal(rec["bits"], words.cpu().numpy().view(np.uint64))
    assert (rec["channel"].astype(np.uint64) * 32 + rec["frame"]).max() * 62 > 1 << 32
    groups = o["groups"].cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(groups[1:], torch.cumsum(per, 0).cpu().numpy().astype(np.uint32))
    assert groups[0] == 0
