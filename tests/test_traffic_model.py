"""The traffic scripts of tests/traffic.py can see what they are meant to see:
shown on the CPU.

- Coverage of the committed seeds is asserted from the model alone.
- Observability is asserted from the oracle alone, per mode.
- A CPU stand-in receiver, built on the oracle's one-frame step (qc_rx_frame on a
  state per channel: an incremental receiver, where the model re-runs every life
  from its start) and the library's host twins (compact, level, squelch, input
  conversion), runs every committed script behind the runner's interface.  Clean
  it passes; with each planted fault some committed script catches it.
- The same on the transmit side: the real host twin qpsk_tx_batch_masked_host is
  the executor, and two planted faults are caught.

CPU only."""
import ctypes as C

import numpy as np
import pytest

import oracle
import rxcheck
import singlecarrier_amd as sc
import traffic
from tx_mask_cases import PACKET, snapshot, snapshot_fields

MODES = [sc.MODE_REFERENCE, sc.MODE_DEC752, sc.MODE_DEC752 | sc.MODE_FFT_HUNT]
MODE_IDS = ["reference", "dec752", "dec752_fft"]


@pytest.fixture(scope="module")
def scripts():
    return {seed: traffic.gen_rx(seed) for seed in traffic.RX_SEEDS}


def test_scripts_are_deterministic_and_within_bounds(scripts):
    traffic._gen_rx.cache_clear()               # generated again, not read back from the cache
    again = {seed: traffic.gen_rx(seed) for seed in traffic.RX_SEEDS}
    for seed, s in scripts.items():
        assert s == again[seed]
        assert len(s) <= 24 and sum(op[2] for op in s if op[0] == "rx") <= 40
        assert all(op[2] in traffic.FRAMES_PER_CALL for op in s if op[0] == "rx")
        assert all(op[2] in traffic.REINDEX for op in s if op[0] == "reindex")
    assert traffic.min_sumsq() == sc.sumsq_of_dbfs(traffic.SQUELCH_DBFS)


# ------------------------------------------------------------------------- coverage
def coverage(scripts):
    cover = {}
    for s in scripts.values():
        m = traffic.RxModel({"A": 130, "B": 40})
        for op in s:
            assert m.valid(op), op
            m.apply(op)
        for k, v in m.cover.items():
            if k[0] != "nth":
                cover[k] = cover.get(k, 0) + v
    return cover


def test_coverage_of_the_committed_seeds(scripts):
    cover = coverage(scripts)
    pairs = {(a, b) for a in traffic.RX_KINDS for b in traffic.RX_KINDS}
    missing = sorted(p for p in pairs if ("pair",) + p not in cover)
    assert not missing, f"op kinds never back to back on one channel: {missing}"
    for item in (("join distance", "odd"), ("join distance", "even"), ("reset distance", "odd"),
                 ("reset distance", "even"), ("join on a reset or joined channel",), ("mixed save",),
                 ("word passes 1057 in a call",), ("F0 after a reset",), ("join of a reindexed slot",)):
        assert cover.get(item), f"not covered: {item}"
    for form in ("dense", "rec", "sq", "alaw", "alaw_sq"):
        assert cover.get(("form", form)), form
    for order in traffic.ORDERS:                # plain record calls that return rows, F > 0
        for cap in (None, "count-1"):
            assert cover.get(("rec rows", order, cap)), f"no rec call with F > 0, order {order}, cap {cap}"
    for kind in ("inside one quad", "across a 64-lane boundary", "the last channel", "inside a range reset earlier"):
        assert cover.get(("range", kind)), f"no reset_channels range {kind}"
    for form in ("dense", "sq"):                # both forms right behind a lifecycle op, F > 0
        for where in ("host", "device"):
            assert cover.get((form + " after a lifecycle op", where)), (form, where)
    for form in ("rec", "sq", "alaw_sq"):
        assert cover.get(("records after a lifecycle op", form)), form
    for F in traffic.FRAMES_PER_CALL:
        assert cover.get(("F", F)), F
    for G in traffic.REINDEX:
        assert cover.get(("G", G)), G


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_every_op_kind_is_observed(scripts, mode):
    """Through a frame the oracle calls valid with fewer than 128 matches, on a
    channel of the op's range before its next start: 3 times per kind."""
    total = {}
    for seed, s in scripts.items():
        counts, _ = traffic.observe_script(s, mode, seed)
        for k, v in counts.items():
            total[k] = total.get(k, 0) + v
    print(total)
    for kind in traffic.RX_KINDS + ("reindex",):
        assert total.get(kind, 0) >= 3, f"{kind}: observed {total.get(kind, 0)} times"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_plain_record_calls_return_rows(scripts, mode):
    """Every rec call with F > 0 and a cap other than 0 returns rows (count - 1 > 0
    too), in both orders and with both caps, by the oracle."""
    rows = {}
    for seed, s in scripts.items():
        _, m = traffic.observe_script(s, mode, seed)
        for call in m.calls:
            form = call["form"]
            if form[0] == "rec" and call["F"] and form[2] != 0:
                n = len(call["rec"]["rec"])
                assert n > 0, f"seed {seed}, op {call['op']} {call['tuple']}: no rows"
                rows[form[1:]] = rows.get(form[1:], 0) + n
    print(rows)
    assert set(rows) == {(o, c) for o in traffic.ORDERS for c in (None, "count-1")}


@pytest.mark.parametrize("gap", [0, 903])
def test_the_exchange_is_observed(gap):
    plan = traffic.exchange_plan(traffic.EX_SEED, gap)
    _, stats = traffic.exchange_expected(plan)
    print(gap, stats)
    assert stats["observed"] >= 40
    assert stats["squelched"] > 0, "the gate never closes on a valid frame"


# ------------------------------------------------------------- the stand-in receiver
HDR = 64
FAULTS = ("join keeps the descrambler index", "reset one short at the low end", "reset one short at the high end",
          "join one channel off", "channel_frames not updated by a load", "record frame from the own index",
          "prev ignored at f == 0", "mixed save accepted")


def _einval():
    e = sc.QpskError("stand-in: QPSK_EINVAL")
    e.code = sc.QPSK_EINVAL
    return e


class CpuRx:
    """A receiver for the runner made of qc_rx_frame and the host twins.  `own` is
    what channel_frames reports, `key` what the descrambler uses."""

    def __init__(self, nch, mode, faults=()):
        self.lib = oracle.chan_lib()
        self.nch, self.mode, self.faults = nch, mode, set(faults)
        assert self.faults <= set(FAULTS)
        self.reset()

    def _fresh(self):
        ch = oracle.Chan()
        self.lib.qc_chan_init_mode(C.byref(ch), self.mode)
        return ch

    def reset(self):
        self.ch = [self._fresh() for _ in range(self.nch)]
        self.own, self.key, self.flip = [0] * self.nch, [0] * self.nch, [0] * self.nch
        self.frames, self.fresh, self.pending = 0, True, set()

    def close(self):
        pass

    def channel_frames(self):
        return np.array([self.frames if c in self.pending else self.own[c] for c in range(self.nch)], np.uint64)

    def reset_channels(self, c0, n):
        if self.pending:
            raise _einval()
        lo = c0 + ("reset one short at the low end" in self.faults)
        hi = c0 + n - ("reset one short at the high end" in self.faults)
        for c in range(lo, hi):
            self.ch[c], self.own[c], self.key[c], self.flip[c] = self._fresh(), 0, 0, 0
        self.fresh = False

    def state_save(self, c0, n):
        if self.pending or (len(set(self.own[c0:c0 + n])) > 1 and "mixed save accepted" not in self.faults):
            raise _einval()
        G = self.own[c0]
        hdr = bytearray(HDR)
        hdr[:8] = b"QPSKSTA1"
        hdr[16:24] = np.array([self.mode, n], "<i4").tobytes()
        hdr[24:32] = np.array([G], "<u8").tobytes()
        hdr[32] = self.key[c0] & 1                 # the parity the mixed state stands at
        body = b""
        for c in range(c0, c0 + n):
            ch = oracle.Chan.from_buffer_copy(self.ch[c])
            ch.frame = 0
            if self.flip[c]:                       # kept at the other parity: the snapshot is the index's own
                d = np.frombuffer(ch.dprev, np.float32)
                d[d != 0] *= -1
            body += bytes(ch)
        return bytes(hdr) + body

    def _put(self, snap, c0, index_of):
        n, G = int(np.frombuffer(snap[20:24], "<i4")[0]), traffic.frame_of(snap)
        size = C.sizeof(oracle.Chan)
        for i in range(n):
            ch = oracle.Chan.from_buffer_copy(snap[HDR + i * size:HDR + (i + 1) * size])
            self.ch[c0 + i] = ch
            self.flip[c0 + i] = (G ^ snap[32]) & 1   # the state stays at its parity; the mixer follows it
            index_of(c0 + i, G)
        self.fresh = False

    def state_join(self, snap, c0):
        if self.pending:
            raise _einval()
        n = int(np.frombuffer(snap[20:24], "<i4")[0])
        if "join one channel off" in self.faults:
            c0 = c0 + 1 if c0 + n < self.nch else c0 - 1

        def index_of(c, G):
            self.own[c] = G
            self.key[c] = self.frames if "join keeps the descrambler index" in self.faults else G
        self._put(snap, c0, index_of)

    def state_load(self, snap, c0):
        n, G = int(np.frombuffer(snap[20:24], "<i4")[0]), traffic.frame_of(snap)
        if self.fresh and not self.pending:
            self.frames = G
            if G and n < self.nch:
                self.pending = set(range(self.nch))
            for c in range(self.nch):
                self.key[c] = G
                if "channel_frames not updated by a load" not in self.faults:
                    self.own[c] = G
        elif G != self.frames:
            raise _einval()
        self.pending -= set(range(c0, c0 + n))

        def index_of(c, G):
            self.key[c] = G
            if "channel_frames not updated by a load" not in self.faults:
                self.own[c] = G
        self._put(snap, c0, index_of)

    def _step(self, x):
        nch, F = x.shape[:2]
        bits = np.zeros((nch, F, 62), np.uint8)
        valid = np.zeros((nch, F), np.uint8)
        tr = np.zeros((nch, F), oracle.TRACE_DTYPE)
        x = np.ascontiguousarray(x, np.int16)
        for c in range(nch):
            ch = self.ch[c]
            for f in range(F):
                v = self.key[c] % traffic.KS_FRAMES                  # the keystream word, at the state's parity
                v = v if (v ^ self.key[c] ^ self.flip[c]) & 1 == 0 else v + traffic.KS_FRAMES
                # (qc_rx_frame takes the history for zeros at frames 0 and 1: a channel with
                # history stays clear of them, one keystream period and mixer period up)
                ch.frame = v + 2 * traffic.KS_FRAMES if np.any(np.frombuffer(ch.hist, np.int16)) else v
                valid[c, f] = self.lib.qc_rx_frame(C.byref(ch), x[c, f].ctypes.data, bits[c, f].ctypes.data,
                                                   tr[c, f:f + 1].ctypes.data)
                self.key[c] += 1
                self.own[c] += 1
        self.frames += F
        self.fresh = self.fresh and F == 0
        return rxcheck.dense(bits, valid, tr)

    def run(self, form, x, codes, prev, cap):
        if self.pending:
            raise _einval()
        kind = form[0]
        if kind in ("alaw", "alaw_sq"):
            x = sc.input_convert_host(codes, traffic.ALAW_I, self.nch, threads=1)
        before = list(self.own)
        d = self._step(x)
        if kind in ("dense", "alaw"):
            return d
        order = form[1] if kind in ("rec", "alaw_sq") else form[2]
        valid, extra = d["valid"], {}
        if kind != "rec":
            level = sc.level_host(x)
            p = None if "prev ignored at f == 0" in self.faults else prev
            sq = sc.squelch_host(level, valid, sc.sumsq_of_dbfs(traffic.SQUELCH_DBFS), prev=p,
                                 bits=d["bits"], soft=d["soft"])
            valid = sq["valid"]
            extra = {"level": level, "last": sq["last"] if x.shape[1] else prev.copy()}
        r = sc.compact_host(d["bits"], valid, d["trace"], d["soft"], order=order, cap=cap)
        if "record frame from the own index" in self.faults:
            r["rec"]["frame"] += np.array(before, np.uint64)[r["rec"]["channel"]].astype(np.uint32)
        r.update(extra)
        return r


def _make(faults=()):
    return lambda nch, mode: CpuRx(nch, mode, faults)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_the_clean_stand_in_passes_every_script(scripts, mode):
    for seed, s in scripts.items():
        traffic.run_rx(s, _make(), mode, seed)


@pytest.mark.parametrize("fault", FAULTS)
def test_a_planted_fault_is_caught(scripts, fault):
    caught = []
    for seed, s in scripts.items():
        try:
            traffic.run_rx(s, _make([fault]), sc.MODE_REFERENCE, seed)
        except AssertionError as e:
            caught.append((seed, str(e)[:200]))
    print(fault, "->", caught)
    assert caught, f"no committed script catches: {fault}"
    assert all(f"seed {seed}" in msg for seed, msg in caught)


def test_a_prefix_replays_to_the_same_difference(scripts):
    """The message's seed and op index are enough: the prefix up to that op shows the difference."""
    fault = "join keeps the descrambler index"
    for seed, s in scripts.items():
        try:
            traffic.run_rx(s, _make([fault]), sc.MODE_REFERENCE, seed)
        except AssertionError as e:
            msg = str(e)
            k = int(msg.split("op ")[1].split(" ")[0])
            with pytest.raises(AssertionError) as ei:
                traffic.replay(s[:k + 1], "rx", sc.MODE_REFERENCE, seed, make=_make([fault]))
            assert f"op {k} " in str(ei.value)
            return
    pytest.fail("the fault was not caught")


# ---------------------------------------------------------------- the transmit side
TX_FAULTS = ("load forgets the last dibits", "an idle slot advances the index")


class CpuTx:
    """The host twin qpsk_tx_batch_masked_host behind the runner's interface.  A
    snapshot is the header's: index and last 9 dibits; a load rebuilds the
    channel as the header says it behaves, a fresh run of the transmitter fed
    `index` packets of which the last ends in those dibits."""

    def __init__(self, nch, gap, faults=()):
        self.nch, self.gap, self.faults = nch, gap, set(faults)
        self.st = sc.tx_states(nch)
        self.idx, self.word, self.slots = np.zeros(nch, np.uint64), np.zeros(nch, np.uint32), 0

    def close(self):
        pass

    def packets(self):
        return self.slots

    def channel_packets(self):
        return self.idx.copy()

    def reset_channels(self, c0, n):
        self.st[c0:c0 + n] = sc.tx_states(n)
        self.idx[c0:c0 + n], self.word[c0:c0 + n] = 0, 0

    def state_save(self, c0, n):
        return snapshot(self.idx[c0:c0 + n], self.word[c0:c0 + n])

    def state_load(self, snap, c0):
        n, idx, words = snapshot_fields(snap)
        for i in range(n):
            k, w = int(idx[i]), int(words[i])
            if "load forgets the last dibits" in self.faults:
                w = 0
            st = sc.tx_states(1)
            if k:
                bits = np.zeros((1, k, 8, 62), np.uint8)
                for j in range(9):
                    fr, s = divmod(239 + j, 31)
                    bits[0, -1, fr, 2 * s + 1], bits[0, -1, fr, 2 * s] = (w >> j) & 1, (w >> (16 + j)) & 1
                sc.tx_batch_host(bits, gap=0, states=st, threads=1)
            self.st[c0 + i], self.idx[c0 + i], self.word[c0 + i] = st[0], k, words[i]

    def run(self, form, bits, mask):
        nch, npk = bits.shape[:2]
        y = sc.tx_batch_host(bits, gap=self.gap, states=self.st, active=mask, threads=1)
        for c in range(nch):
            k = np.arange(npk) if mask is None else np.flatnonzero(mask[c])
            if k.size:
                self.word[c] = traffic.last_dibits(bits[c, k[-1]])
            self.idx[c] += np.uint64(k.size)
            idle = npk - k.size
            if idle and "an idle slot advances the index" in self.faults:
                st = self.st[c:c + 1].copy()                 # the carrier of `idle` more packets
                sc.tx_batch_host(np.zeros((1, idle, 8, 62), np.uint8), gap=0, states=st, threads=1)
                self.st[c, -8:] = st[0, -8:]
                self.idx[c] += np.uint64(idle)
        self.slots += npk
        return y if form == "s16_device" else sc.output_convert_host(y, traffic.TX_FMT[form])


def test_transmit_scripts_cover_the_ops_and_forms():
    ops = [op for seed in traffic.TX_SEEDS for op in traffic.gen_tx(seed)]
    assert {op[0] for op in ops} == {"tx", "reset_channels", "save", "load"}
    assert {op[4] for op in ops if op[0] == "tx"} == set(traffic.TX_FORMS)
    for seed in traffic.TX_SEEDS:
        s = traffic.gen_tx(seed)
        assert s == traffic.gen_tx(seed) and sum(op[2] for op in s if op[0] == "tx") <= 30
    for seed in traffic.TX_SEEDS:        # a load into a context of another gap than the save's
        s = traffic.gen_tx(seed)
        saved = {op[4]: op[1] for op in s if op[0] == "save"}
        if any(op[0] == "load" and saved[op[2]] != op[1] for op in s):
            return
    pytest.fail("no snapshot moves to a context of another gap")


@pytest.mark.parametrize("seed", traffic.TX_SEEDS)
def test_the_real_host_twin_passes_the_transmit_scripts(seed):
    traffic.run_tx(traffic.gen_tx(seed), CpuTx, seed)


@pytest.mark.parametrize("fault", TX_FAULTS)
def test_a_planted_transmit_fault_is_caught(fault):
    caught = []
    for seed in traffic.TX_SEEDS:
        try:
            traffic.run_tx(traffic.gen_tx(seed), lambda nch, gap: CpuTx(nch, gap, [fault]), seed)
        except AssertionError as e:
            caught.append((seed, str(e)[:160]))
    print(fault, "->", caught)
    assert caught, f"no committed transmit script catches: {fault}"


def test_mask_rows_are_call_traffic():
    m = traffic.call_mask(3, 64, 30) != 0
    for row in m:
        runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], row.astype(np.int8), [0]]))))
        active, idle = runs[::2], runs[1::2]
        assert (active <= 5).all() and (idle >= 1).all() and (idle <= 3).all()
        inner = active[1:-1] if row[0] and row[-1] else active[1:] if row[0] else active[:-1] if row[-1] else active
        assert (inner >= 2).all()
    assert PACKET == 1880
