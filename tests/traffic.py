"""Random call traffic over the lifecycle calls: seeded scripts, a model written
from the headers alone, and a runner that compares every output with the oracle.

Plain module like tests/spacing.py: no GPU import at module level (torch is
imported inside the GPU adapters).  Everything the model knows comes from
include/qpsk_batch.h, qpsk_compact.h, qpsk_level.h, qpsk_input.h and qpsk_tx.h;
nothing here knows how the library keeps a channel's index.

Receive model.  A channel is a *life*: the frames it was fed since its latest
start and its own index at that start (RxModel).  The spec sentence is the whole
model: every channel behaves exactly like a fresh run of the reference receiver
fed that channel's stream from its start.  So the dense outputs of a call are
oracle.cpu_rx on each life from its first frame, sliced to the call; where a
life's own index is not its frame count, the bits of valid frames move from the
keystream words of the life's frames to those of the own index.  Records, levels
and the squelch gate are restated here in numpy from the header text.  Lives of
equal length share one oracle run, and the model is evaluated once, at the end
of a script (a record call with cap = count - 1 evaluates its own context when
it is made, to know the count).

Scripts.  gen_rx(seed) / gen_tx(seed) return lists of plain tuples that print
and replay; replay(script[:k], ...) runs a prefix.  Receive ops, on two contexts
"A" and "B" of one mode and different channel counts:
    ("rx", ctx, F, form)            form: ("dense", "host" | "device"),
                                    ("rec", order, cap), ("sq", "host" | "device", order, cap),
                                    ("alaw",), ("alaw_sq", order);
                                    cap: None, "count-1" or 0
    ("reset_channels", ctx, c0, n)
    ("save", ctx, c0, n, slot)      QPSK_EINVAL predicted when the range holds two indices
    ("join", ctx, slot, c0)
    ("load", ctx, slot, c0)         into a context that is fresh, assembling, or at the slot's index
    ("reset", ctx)
    ("reindex", slot, G)            the snapshot's header edited to own index G
Transmit ops, on contexts "T0", "T1", "T2" of gaps 0, 1, 903:
    ("tx", ctx, npk, mask_seed, form)   form: "s16_device", "alaw", "ulaw_i"
    ("reset_channels", ctx, c0, n), ("save", ctx, c0, n, slot), ("load", ctx, slot, c0)

One place knows more than the headers say in so many words: _compare_snapshots
starts its plain receiver at the life's start index, because qpsk_batch.h promises
equal bytes for channels "fed the same frames", and a life whose snapshot was
edited to another index is a run from that index; where that start would be
negative it takes the index mod 2 * 1057, which rests on the state depending on
the index's parity and keystream word alone (tests/test_channel_index.py B pins
that on the oracle).

An executor is anything with the adapters' interface (GpuRx / GpuTx here, the
CPU stand-ins of tests/test_traffic_model.py).  A failure names the seed, the op
index, the op tuple, the output and the first differing (channel, frame).
"""
import functools
import math

import numpy as np

import g711
import oracle
import rxcheck
import singlecarrier_amd as sc
from tx_mask_cases import PACKET, Restated, last_dibits, payload, snapshot_fields

FRAME = sc.FRAME_SIZE
KS_FRAMES = 1057                      # 62 * 1057 = 2 * 32767: the keystream's period in frames
ALAW_I = sc.IN_ALAW | sc.IN_INTERLEAVED
REINDEX = (1, 1055, 1056, 2113, 2**32 + 5)
FRAMES_PER_CALL = (0, 1, 2, 3, 5)
RX_KINDS = ("rx", "reset_channels", "save", "join", "load", "reset")   # the kinds that touch channels
SQUELCH_DBFS = -60.0
# The committed seeds: tests/test_traffic_model.py asserts what they cover and observe.  A committed
# seed's script goes for what the seeds in front of it in this tuple left uncovered, so "seed 189"
# means its script under this order: reordering or editing the tuple changes the scripts behind the
# edit (gen_rx(seed) of a seed that is not in the tuple depends on nothing but the seed).
RX_SEEDS = (205, 174, 375, 350)
TX_SEEDS = (1, 2, 3)
EX_SEED = 7


# ------------------------------------------------------- snapshot header, keystream
def frame_of(snap):
    """StateHdr.frame of a receive snapshot."""
    return int(np.frombuffer(snap[24:32], "<u8")[0])


def at_frame(snap, old, G):
    """The one header edit: StateHdr.frame of a receive snapshot from `old` to G."""
    assert snap[:8] == b"QPSKSTA1" and len(snap) >= 64 and frame_of(snap) == old, "StateHdr layout changed"
    return snap[:24] + np.array([G], "<u8").tobytes() + snap[32:]


def keywords(first, nf):
    """The 62 keystream bits of frames first .. first + nf - 1 (any 64-bit first)."""
    ks = oracle.keystream(32767)
    words = np.array([(int(first) + k) % KS_FRAMES for k in range(nf)], np.int64)
    idx = (62 * words[:, None] + np.arange(62)[None, :]) % 32767
    return ks[idx]


# --------------------------------------------- numpy restatements of the header text
def min_sumsq(db=SQUELCH_DBFS):
    """qpsk_level.h: the smallest sumsq whose level 10 log10(sumsq / (1880 * 2^30)) is at least db."""
    full = FRAME << 30
    s = max(int(math.ceil(full * 10.0 ** (db / 10.0))), 1)
    while s > 1 and 10.0 * math.log10((s - 1) / full) >= db:
        s -= 1
    while 10.0 * math.log10(s / full) < db:
        s += 1
    return s


def levels_np(x):
    """qpsk_frame_level of every frame of int16 [...][1880]."""
    v = np.asarray(x).astype(np.int64)
    out = np.zeros(v.shape[:-1], sc.LEVEL_DTYPE)
    out["sumsq"] = (v * v).sum(-1)
    out["sum"] = v.sum(-1)
    out["peak"] = np.abs(v).max(-1) if v.shape[-1] else 0
    out["clipped"] = ((v == 32767) | (v == -32768)).sum(-1)
    return out


def gate_np(level, prev, valid, floor):
    """valid_out of the squelch: w = max(sumsq[f], sumsq[f - 1] or prev) >= floor ? valid : 0."""
    s = level["sumsq"].astype(np.uint64)
    p = np.concatenate([prev["sumsq"].astype(np.uint64)[:, None], s[:, :-1]], axis=1) if s.shape[1] else s
    return np.where(np.maximum(s, p) >= np.uint64(floor), valid, 0).astype(np.uint8)


def records_np(dense, valid, order, cap):
    """The records of a call from its dense outputs, ranked by `valid`:
    {"rec", "count", "groups", "trace", "soft"}, rows trimmed to min(count, cap)."""
    v = valid != 0
    if order == sc.REC_BY_CHANNEL:
        at = np.argwhere(v)
        per = v.sum(axis=1)
    else:
        at = np.argwhere(v.T)[:, ::-1]
        per = v.sum(axis=0)
    ch, fr = at[:, 0], at[:, 1]
    count = len(ch)
    m = count if cap is None else min(count, cap)
    rec = np.zeros(m, sc.REC_DTYPE)
    rec["channel"], rec["frame"] = ch[:m], fr[:m]
    ones = (dense["bits"][ch[:m], fr[:m]] == 1).astype(np.uint64)
    rec["bits"] = (ones << np.arange(62, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    groups = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    return {"rec": rec, "count": count, "groups": groups,
            "trace": dense["trace"][ch[:m], fr[:m]], "soft": dense["soft"][ch[:m], fr[:m]]}


def dense_zeros(nch, nf):
    """The dense outputs of a call (qpsk_batch.h's layouts), all zero."""
    return {"bits": np.zeros((nch, nf, 62), np.uint8), "valid": np.zeros((nch, nf), np.uint8),
            "trace": np.zeros((nch, nf, 4), np.int32), "soft": np.zeros((nch, nf, 31, 2), np.float32)}


def quantize_alaw(x):
    """int16 samples as an A-law line carries them, and the codes."""
    codes = g711.compress(x, sc.OUT_ALAW)
    return g711.expand(codes, sc.IN_ALAW), codes


# ------------------------------------------------------------------ source streams
def sources(seed, nrows, nframes):
    """int16 [nrows][nframes][1880], read-only: noiseless oracle.synth streams; on
    every second row the line goes silent for 1-2 frames after every 3-6 (call
    traffic for the squelch: the receiver calls silence valid)."""
    x = oracle.synth(1000 + seed, nrows, nframes, 1000.0)
    rng = np.random.default_rng([seed, 77])
    for r in range(1, nrows, 2):
        f = int(rng.integers(2, 6))
        while f < nframes:
            k = int(rng.integers(1, 3))
            x[r, f:f + k] = 0
            f += k + int(rng.integers(3, 7))
    x.setflags(write=False)
    return x


# --------------------------------------------------------------------- receive model
class Life:
    """A channel since its latest start: the frames fed (chunks [k][1880]), their
    count n, and own0 = own index - n (not 0 after a reindex)."""
    __slots__ = ("chunks", "n", "own0", "touched")

    def __init__(self, chunks=(), n=0, own0=0, touched=False):
        self.chunks, self.n, self.own0, self.touched = list(chunks), n, own0, touched

    def copy(self):
        return Life(self.chunks, self.n, self.own0, self.touched)

    @property
    def own(self):
        return self.own0 + self.n

    def samples(self):
        return np.concatenate(self.chunks) if self.chunks else np.zeros((0, FRAME), np.int16)


def range_kinds(lo, hi, nch, earlier):
    """The kinds of range the issue names that [lo, hi) is."""
    kinds = []
    if hi - lo < 4 and lo // 4 == (hi - 1) // 4:
        kinds.append("inside one quad")
    if lo // 64 != (hi - 1) // 64:
        kinds.append("across a 64-lane boundary")
    if lo == nch - 1:
        kinds.append("the last channel")
    if any(a <= lo and hi <= b and (hi - lo) < (b - a) for a, b in earlier):
        kinds.append("inside a range reset earlier")
    return kinds


class _Ctx:
    def __init__(self, nch, row0):
        self.resets = []                                    # the ranges reset since create / reset
        self.nch, self.frames, self.fresh, self.pending = nch, 0, True, set()
        self.life = [Life() for _ in range(nch)]
        self.src = [[row0 + c, 0] for c in range(nch)]      # [source row, cursor]
        self.last = ["create"] * nch                        # the latest op kind on the channel
        self.reidx = [False] * nch


class RxModel:
    """The receive model and the coverage it has seen.  src None: bookkeeping
    only (the script generator)."""

    def __init__(self, nchs, src=None):
        self.src = src
        self.ctx, row = {}, 0
        for name, n in nchs.items():
            self.ctx[name] = _Ctx(n, row)
            row += n
        self.slots, self.calls, self.cover = {}, [], {}

    # -- coverage: what an op exercises, from the model alone
    def items(self, op):
        kind = op[0]
        it = []
        if kind == "reindex":
            return [("G", op[2])]
        cx = self.ctx[op[1]]
        lo, hi = self.range_of(op)
        it += [("pair", cx.last[c], kind) for c in range(lo, hi) if cx.last[c] != "create"]
        if kind == "rx":
            F, form = op[2], op[3]
            it.append(("form", form[0]))
            it.append(("F", F))
            after = any(k not in ("rx", "create") for k in cx.last)     # right behind a lifecycle op
            if F and form[0] == "rec" and form[2] != 0:
                it.append(("rec rows", form[1], form[2]))
            if F and after and form[0] in ("dense", "sq"):
                it.append((form[0] + " after a lifecycle op", form[1]))
            if F and after and form[0] in ("rec", "sq", "alaw_sq"):
                it.append(("records after a lifecycle op", form[0]))
            if F == 0 and any(k in ("reset", "reset_channels") for k in cx.last):
                it.append(("F0 after a reset",))
            if any(cx.reidx[c] and cx.life[c].own % KS_FRAMES + F > KS_FRAMES for c in range(cx.nch)):
                it.append(("word passes 1057 in a call",))
        elif kind == "reset_channels":
            it.append(("reset distance", "odd" if cx.frames & 1 else "even"))
            it += [("range", k) for k in range_kinds(lo, hi, cx.nch, cx.resets)]
        elif kind == "save":
            if len({cx.life[c].own for c in range(lo, hi)}) > 1:
                it.append(("mixed save",))
        elif kind in ("join", "load"):
            s = self.slots[op[2]]
            if kind == "join":
                it.append(("join distance", "odd" if (s["own"] - cx.frames) & 1 else "even"))
                if any(cx.life[c].touched for c in range(lo, hi)):
                    it.append(("join on a reset or joined channel",))
            if s["reidx"]:
                it.append((kind + " of a reindexed slot",))
        return it

    def gain(self, op):
        return len({i for i in self.items(op) if i not in self.cover})

    def range_of(self, op):
        kind = op[0]
        cx = self.ctx[op[1]]
        if kind in ("rx", "reset"):
            return 0, cx.nch
        if kind in ("reset_channels", "save"):
            return op[2], op[2] + op[3]
        return op[3], op[3] + self.slots[op[2]]["n"]

    def valid(self, op):
        """May the script hold this op here?  (What the headers allow and what the model can predict.)"""
        kind = op[0]
        if kind == "reindex":
            return op[1] in self.slots
        cx = self.ctx[op[1]]
        if kind in ("join", "load") and op[2] not in self.slots:
            return False
        lo, hi = self.range_of(op)
        if not (0 <= lo < hi <= cx.nch):
            return False
        if kind == "reset":
            return True
        if kind == "load":
            G = self.slots[op[2]]["own"]
            return (cx.fresh and not cx.pending) or G == cx.frames
        return not cx.pending

    def apply(self, op, opi=None):
        """Advances the model; returns what the runner needs of the op."""
        for i in self.items(op):
            self.cover[i] = self.cover.get(i, 0) + 1
        kind = op[0]
        if kind == "reindex":
            s = self.slots[op[1]]
            s["own"], s["reidx"] = op[2], True
            for life, _ in s["chan"]:
                life.own0 = op[2] - life.n
            return None
        cx = self.ctx[op[1]]
        lo, hi = self.range_of(op)
        res = None
        if kind == "rx":
            res = self._feed(op, opi)
        elif kind == "reset_channels":
            for c in range(lo, hi):
                cx.life[c] = Life(touched=True)
                cx.reidx[c] = False
            cx.fresh = False
            cx.resets.append((lo, hi))
        elif kind == "save":
            owns = {cx.life[c].own for c in range(lo, hi)}
            res = len(owns) == 1
            if res:
                self.slots[op[4]] = {"n": hi - lo, "own": owns.pop(), "reidx": False,
                                     "chan": [(cx.life[c].copy(), list(cx.src[c])) for c in range(lo, hi)]}
        elif kind in ("join", "load"):
            s = self.slots[op[2]]
            if kind == "load":
                if cx.fresh and not cx.pending:
                    cx.frames = s["own"]
                    if s["own"] != 0 and s["n"] < cx.nch:
                        cx.pending = set(range(cx.nch))
                cx.pending -= set(range(lo, hi))
            for i, c in enumerate(range(lo, hi)):
                life, src = s["chan"][i]
                cx.life[c], cx.src[c] = life.copy(), list(src)
                cx.life[c].touched = kind == "join"
                cx.reidx[c] = s["reidx"]
            cx.fresh = False
        elif kind == "reset":
            cx.life = [Life() for _ in range(cx.nch)]
            cx.reidx = [False] * cx.nch
            cx.frames, cx.fresh, cx.pending, cx.resets = 0, True, set(), []
        for c in range(lo, hi):
            cx.last[c] = kind
        return res

    def _feed(self, op, opi):
        _, name, F, form = op
        cx = self.ctx[name]
        call = {"op": opi, "tuple": op, "ctx": name, "F": F, "form": form,
                "life": list(cx.life), "k0": [l.n for l in cx.life], "own": [l.own for l in cx.life]}
        if self.src is not None:
            x = np.stack([self.src[r, cur:cur + F] for r, cur in cx.src])
            assert x.shape == (cx.nch, F, FRAME), "a cursor ran past the source streams"
            if form[0] in ("alaw", "alaw_sq"):
                x, codes = quantize_alaw(x)
                call["codes"] = np.ascontiguousarray(codes.reshape(cx.nch, F * FRAME).T)   # [T][nch]
            call["x"] = x
        for c, life in enumerate(cx.life):
            if self.src is not None and F:
                life.chunks.append(call["x"][c])
            life.n += F
            cx.src[c][1] += F
        cx.frames += F
        cx.fresh = cx.fresh and F == 0
        self.calls.append(call)
        return call

    def frames(self, name):
        return self.ctx[name].frames

    def channel_frames(self, name):
        cx = self.ctx[name]
        return np.array([cx.frames if c in cx.pending else cx.life[c].own for c in range(cx.nch)], np.uint64)

    def prev(self, name, lo, hi):
        """The level the caller carries for channels [lo, hi): that of the frame in
        front of the next one on the channel's stream, zero at its start."""
        out = np.zeros(hi - lo, sc.LEVEL_DTYPE)
        for i, c in enumerate(range(lo, hi)):
            life = self.ctx[name].life[c]
            if life.n:
                out[i] = levels_np(life.chunks[-1][-1])
        return out

    # -- evaluation
    def evaluate(self, mode, calls=None):
        """Fills call["exp"] (the dense outputs) and, for record forms, call["rec"]
        for the given calls (default: all)."""
        calls = self.calls if calls is None else calls
        lives = {}
        for call in calls:
            for life in call["life"]:
                lives[id(life)] = life
        by_len = {}
        for life in lives.values():
            by_len.setdefault(life.n, []).append(life)
        runs = {}
        for n, group in by_len.items():
            if n:
                e = rxcheck.expected(np.stack([l.samples() for l in group]), mode)
                for i, life in enumerate(group):
                    runs[id(life)] = (e, i)
        for call in calls:
            self._expect(call, runs)

    def _expect(self, call, runs):
        nch, F = len(call["life"]), call["F"]
        exp = dense_zeros(nch, F)
        lvl_prev = np.zeros(nch, sc.LEVEL_DTYPE)
        for c, life in enumerate(call["life"]):
            k0, own = call["k0"][c], call["own"][c]
            if F:
                e, i = runs[id(life)]
                for k in rxcheck.KEYS:
                    exp[k][c] = e[k][i, k0:k0 + F]
                if own != k0:
                    vm = exp["valid"][c].astype(bool)
                    exp["bits"][c] = np.where(vm[:, None], exp["bits"][c] ^ keywords(k0, F) ^ keywords(own, F), 0)
            if k0:
                lvl_prev[c] = levels_np(life.samples()[k0 - 1])
        call["exp"] = exp
        call["observed"] = ((exp["valid"] != 0) & (exp["trace"][..., 1] < 128)) if F else np.zeros((nch, 0), bool)
        form = call["form"]
        if form[0] in ("rec", "sq", "alaw_sq"):
            order, cap = (form[1], None) if form[0] == "alaw_sq" else form[-2:]
            valid = exp["valid"]
            r = {}
            if form[0] != "rec":
                level = levels_np(call["x"])
                valid = gate_np(level, lvl_prev, valid, min_sumsq())
                r["level"] = level
                r["last"] = level[:, -1].copy() if F else lvl_prev
                call["squelched"] = int(((exp["valid"] != 0) & (valid == 0)).sum())
            count = int((valid != 0).sum())
            call["cap"] = max(count - 1, 0) if cap == "count-1" else cap
            r.update(records_np(exp, valid, order, call["cap"]))
            call["rec"] = r


# ------------------------------------------------------------- the receive scripts
ORDERS = (sc.REC_BY_CHANNEL, sc.REC_BY_FRAME)
CAPS = (None, "count-1", 0)


def _forms(rng):
    o, cap = ORDERS[int(rng.integers(2))], CAPS[int(rng.integers(3))]
    where = ("host", "device")[int(rng.integers(2))]
    return [("dense", where), ("rec", o, cap), ("sq", where, o, cap), ("alaw",), ("alaw_sq", o)]


def _a_range(rng, nch, earlier):
    """A channel range of one of the kinds the lifecycle calls go wrong at."""
    k = int(rng.integers(6))
    if k == 0:                                   # inside one quad
        q = int(rng.integers(nch // 4))
        return 4 * q + 1, 2
    if k == 1 and nch > 70:                      # across a 64-lane boundary
        c0 = int(rng.integers(58, 64))
        return c0, int(rng.integers(64 - c0 + 1, nch - c0 + 1))
    if k == 2:                                   # the last channel
        return nch - 1, 1
    if k == 3 and earlier:                       # inside a range reset earlier
        c0, n = earlier[int(rng.integers(len(earlier)))]
        if n > 2:
            return c0 + 1, n - 2
    c0 = int(rng.integers(nch))
    return c0, int(rng.integers(1, min(nch - c0, 48) + 1))


@functools.lru_cache(maxsize=None)
def _gen_rx(seed):
    nchs = {"A": 130, "B": 40}
    m = RxModel(nchs)
    if seed in RX_SEEDS and RX_SEEDS.index(seed):     # a committed seed goes for what those before it left
        m.cover = {k: v for k, v in _gen_rx(RX_SEEDS[RX_SEEDS.index(seed) - 1])[1].items() if k[0] != "nth"}
    script = _gen_rx_from(seed, m, nchs, 40, 24)
    return tuple(script), m.cover


def gen_rx(seed):
    """The receive script of a seed: greedy over what the model (and, for a
    committed seed, the committed seeds before it) has not covered yet, a
    receive call every third op, one on each context at the end.  130 and 40
    channels, at most 40 frames and 24 ops."""
    return list(_gen_rx(seed)[0])


def _gen_rx_from(seed, m, nchs, max_frames, max_ops):
    names = list(nchs)
    rng = np.random.default_rng([seed, 1])
    script, resets, nslot = [], {n: [] for n in names}, 0
    tail = 3 * len(names)
    left = max_frames - tail

    def put(op):
        nonlocal left
        assert m.valid(op), op
        m.apply(op)
        kind_n = ("nth", op[0], sum(1 for o in script if o[0] == op[0]))
        m.cover[kind_n] = 1
        script.append(op)
        if op[0] == "rx":
            left -= op[2]
        if op[0] == "reset_channels":
            resets[op[1]].append((op[2], op[3]))

    def rx_ops():
        out = []
        for name in names:
            for form in _forms(rng):
                F = int(rng.choice([f for f in FRAMES_PER_CALL if f <= left]))
                out.append(("rx", name, F, form))
        return out

    def score(op):
        nth = sum(1 for o in script if o[0] == op[0])
        return 10 * m.gain(op) + (15 if nth < 2 else 0) + 5 * float(rng.random())

    put(("rx", names[0], 3, ("dense", "host")))
    put(("rx", names[1], 2, ("dense", "device")))
    must_rx = None
    while len(script) < max_ops - len(names):
        room = max_ops - len(names) - len(script)
        since = next(i for i, o in enumerate(reversed(script)) if o[0] == "rx")
        if since < 3:
            cand = []
            for name in names:
                nch = nchs[name]
                cand += [("reset_channels", name) + _a_range(rng, nch, resets[name]) for _ in range(4)]
                cand += [("save", name) + _a_range(rng, nch, resets[name]) + (nslot,) for _ in range(2)]
                for _ in range(4):                     # saves that succeed: inside one index
                    c = int(rng.integers(nch))
                    own = m.ctx[name].life[c].own
                    hi = c + 1
                    while hi < nch and hi - c < 40 and m.ctx[name].life[hi].own == own:
                        hi += 1
                    cand.append(("save", name, c, int(rng.integers(1, hi - c + 1)), nslot))
                cand.append(("reset", name))
                for s, slot in m.slots.items():
                    if slot["n"] <= nch:
                        for _ in range(3):
                            c0 = int(rng.integers(nch - slot["n"] + 1))
                            cand.append(("join", name, s, c0))
                            cand.append(("load", name, s, c0))
                        same = [o for o in script if o[0] == "save" and o[4] == s and o[1] == name]
                        if same:                          # onto the range it was saved from
                            cand.append(("load", name, s, same[0][2]))
                prev_op = script[-1]
                if prev_op[0] in RX_KINDS[1:] and prev_op[1] == name:   # onto the channels of the op before
                    lo, hi = m.range_of(prev_op)
                    cand.append(("reset_channels", name, lo, (hi - lo + 1) // 2))
                    k = 1
                    while lo + k < hi and k < 40 and m.ctx[name].life[lo + k].own == m.ctx[name].life[lo].own:
                        k += 1
                    cand.append(("save", name, lo, k, nslot))
                    for s, slot in m.slots.items():
                        if slot["n"] <= nch:
                            c0 = min(lo, nch - slot["n"])
                            cand += [("join", name, s, c0), ("load", name, s, c0)]
            if script[-1][0] != "reindex" and room > 2:
                cand += [("reindex", s, REINDEX[int(rng.integers(len(REINDEX)))]) for s in m.slots]
            cand = [op for op in cand if m.valid(op)]
        if since == 2:        # a third op in a row only for a pair with a load that is still missing
            cand = [op for op in cand if op[0] != "reindex" and
                    any(i[0] == "pair" and "load" in i and i not in m.cover for i in m.items(op))]
        if since >= 3 or not cand:
            cand = rx_ops()
        if must_rx:           # a load or a reindexed join is received before anything starts its channels again
            cand = [op for op in rx_ops() if op[1] == must_rx and (op[2] or not left)]
            must_rx = None
        for best in sorted(cand, key=score, reverse=True):
            if best[0] == "load":
                cx, s = m.ctx[best[1]], m.slots[best[2]]
                if cx.fresh and s["own"] != 0 and s["n"] < cx.nch:    # an assembly: load every channel
                    c0s = list(range(0, cx.nch - s["n"], s["n"])) + [cx.nch - s["n"]]
                    if len(c0s) > min(room, 4):
                        continue
                    for c0 in c0s:
                        put(("load", best[1], best[2], c0))
                    must_rx = best[1]
                    break
            put(best)
            nload = sum(1 for o in script if o[0] == "load")
            if (best[0] == "load" and nload % 2) or (best[0] == "join" and m.slots[best[2]]["reidx"] and
                                                     ("pair", "join", "join") in m.cover):
                must_rx = best[1]
            if best[0] == "save" and best[4] in m.slots:
                nslot += 1
            break
        else:
            put(rx_ops()[0])
    left += tail
    for name in names:
        put(("rx", name, 3, ("dense", "host") if name == names[0] else ("sq", "device", sc.REC_BY_FRAME, None)))
    return script


# --------------------------------------------------------------- the receive runner
def _fail(seed, call, what):
    raise AssertionError(f"seed {seed}, op {call['op']} {call['tuple']}: {what}")


def _rows_differ(got, exp):
    """(count, first) of the differing rows of two arrays of rows, bit for bit"""
    g = np.ascontiguousarray(got).reshape(len(got), -1)
    e = np.ascontiguousarray(exp).reshape(len(exp), -1)
    if g.dtype.kind == "f":
        g, e = g.view(np.uint32), e.view(np.uint32)
    elif g.dtype.names:
        g, e = g.view(np.uint8).reshape(len(got), -1), e.view(np.uint8).reshape(len(exp), -1)
    bad = np.flatnonzero((g != e).any(axis=1))
    return len(bad), (int(bad[0]) if len(bad) else None)


def compare_call(seed, call, got):
    """One call's outputs against the model's; raises with the seed, the op, the
    output's name and the first differing (channel, frame)."""
    if "rec" not in call:
        if call["F"] == 0:
            for k in rxcheck.KEYS:
                if got[k].shape != call["exp"][k].shape:
                    _fail(seed, call, f"{k}: shape {got[k].shape}, expected {call['exp'][k].shape}")
            return
        bad = rxcheck.differences(got, call["exp"])
        if bad:
            _fail(seed, call, f"{bad}  (output: (channel-frames, first (channel, frame)))")
        return
    exp, form = call["rec"], call["form"]
    order = form[1] if form[0] == "alaw_sq" else form[-2]
    if got["count"] != exp["count"]:
        _fail(seed, call, f"count {got['count']}, expected {exp['count']}")
    for name in ("groups", "rec", "trace", "soft", "level", "last"):
        if name not in exp:
            continue
        g, e = got[name], exp[name]
        if name == "level":
            g, e = g.reshape(-1), e.reshape(-1)
        if len(e) == 0 and (g is None or len(g) == 0):
            continue
        if g.shape != e.shape:
            _fail(seed, call, f"{name}: shape {g.shape}, expected {e.shape}")
        n, first = _rows_differ(g, e)
        if n:
            if name in ("rec", "trace", "soft"):
                at = (int(exp["rec"]["channel"][first]), int(exp["rec"]["frame"][first]))
            elif name == "level":
                at = divmod(first, call["F"])
            else:
                at = (first, None) if name == "last" or order == sc.REC_BY_CHANNEL else (None, first)
            _fail(seed, call, f"{name} differs in {n} rows, first at row {first}, (channel, frame) {at}: "
                              f"got {g[first]}, expected {e[first]}")


def run_rx(script, make, mode, seed=None, nchs=None, snapshots=True):
    """Runs a receive script on executors made by make(nch, mode) and compares
    everything with the model.  Returns the evaluated model."""
    nchs = nchs or {"A": 130, "B": 40}
    src = sources(0 if seed is None else seed, sum(nchs.values()), 40)
    m = RxModel(nchs, src)
    rx = {name: make(n, mode) for name, n in nchs.items()}
    prev = {name: np.zeros(n, sc.LEVEL_DTYPE) for name, n in nchs.items()}
    snaps, results = {}, []
    try:
        for i, op in enumerate(script):
            where = f"seed {seed}, op {i} {op}"
            assert m.valid(op), f"{where}: the script does not fit the model"
            kind = op[0]
            if kind == "reindex":
                snaps[op[1]] = at_frame(snaps[op[1]], m.slots[op[1]]["own"], op[2])
                m.apply(op, i)
                continue
            name = op[1]
            r = rx[name]
            if kind == "rx":
                call = m.apply(op, i)
                form, cap = op[3], None
                if form[0] in ("rec", "sq"):
                    cap = form[-1]
                    if cap == "count-1":
                        m.evaluate(mode, [call])
                        cap = call["cap"]
                got = r.run(form, call["x"], call.get("codes"), prev[name], cap)
                if "last" in got:
                    prev[name] = got["last"].copy()
                elif op[2]:
                    prev[name] = levels_np(call["x"][:, -1])
                results.append((call, got))
            elif kind == "save":
                ok = m.apply(op, i)
                try:
                    snap = r.state_save(op[2], op[3])
                except sc.QpskError as e:
                    assert not ok and e.code == sc.QPSK_EINVAL, f"{where}: {e}, the model expects a snapshot"
                else:
                    assert ok, f"{where}: a range with two indices was saved; QPSK_EINVAL expected"
                    snaps[op[4]] = snap
                    assert frame_of(snap) == m.slots[op[4]]["own"], \
                        f"{where}: the snapshot is at {frame_of(snap)}, the model at {m.slots[op[4]]['own']}"
            else:
                if kind == "reset_channels":
                    r.reset_channels(op[2], op[3])
                elif kind == "join":
                    r.state_join(snaps[op[2]], op[3])
                elif kind == "load":
                    r.state_load(snaps[op[2]], op[3])
                else:
                    r.reset()
                m.apply(op, i)
                lo, hi = m.range_of(op)
                prev[name][lo:hi] = m.prev(name, lo, hi)   # zero after a reset or a fresh join
            assert r.frames == m.frames(name), f"{where}: frames {r.frames}, model {m.frames(name)}"
            got, want = r.channel_frames(), m.channel_frames(name)
            if not np.array_equal(got, want):
                c = int(np.flatnonzero(got != want)[0])
                raise AssertionError(f"{where}: channel_frames differs first at channel {c}: {got[c]}, model {want[c]}")
        m.evaluate(mode)
        for call, got in results:
            compare_call(seed, call, got)
        if snapshots:
            _compare_snapshots(seed, m, rx, make, mode)
    finally:
        for r in rx.values():
            r.close()
    return m


def _compare_snapshots(seed, m, rx, make, mode):
    """Every maximal range of one index and one age against a plain receiver fed
    those channels' frames from their start (at their start's index: the state
    of a run from another index differs by that index's parity alone)."""
    for name, cx in m.ctx.items():
        if cx.pending:
            continue
        c = 0
        while c < cx.nch:
            hi = c + 1
            while hi < cx.nch and (cx.life[hi].own, cx.life[hi].n) == (cx.life[c].own, cx.life[c].n):
                hi += 1
            life = cx.life[c]
            got = rx[name].state_save(c, hi - c)
            plain = make(hi - c, mode)
            base = life.own0 % (2 * KS_FRAMES) if life.own0 < 0 else life.own0
            if base:
                plain.state_load(at_frame(plain.state_save(0, hi - c), 0, base), 0)
            if life.n:
                plain.run(("dense", "host"), np.stack([cx.life[k].samples() for k in range(c, hi)]), None, None, None)
            want = plain.state_save(0, hi - c)
            plain.close()
            if base + life.n != life.own:
                want = at_frame(want, base + life.n, life.own)
            if got != want:
                d = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
                raise AssertionError(f"seed {seed}, end of script: the snapshot of {name}[{c}, {hi}) (own index "
                                     f"{life.own}, {life.n} frames) differs from a plain receiver's in {len(d)} "
                                     f"bytes, first at byte {int(d[0])}")
            c = hi


# ------------------------------------------------------------------ what was observed
def observed(m):
    """{op index: True/False} for the ops of an evaluated model: some channel of
    the op's range has, before its next start, a frame the oracle calls valid
    with fewer than 128 matches.  A reindex is observed through a join or load
    of its slot; a save through its channels going on, or through such a join."""
    seen = {}                                  # id(life) -> frames (life positions) that are observed
    for call in m.calls:
        for c, life in enumerate(call["life"]):
            ks = np.flatnonzero(call["observed"][c])
            if len(ks):
                seen.setdefault(id(life), []).extend((call["k0"][c] + ks).tolist())
    return seen


def observe_script(script, mode, seed, nchs=None):
    """Runs the model alone (no executor) over a script and returns {kind: the
    number of its ops that are observed} and the evaluated model."""
    nchs = nchs or {"A": 130, "B": 40}
    m = RxModel(nchs, sources(seed, sum(nchs.values()), 40))
    marks = []                                 # (kind, [(life, frames it had when the op ran)])
    by_slot = {}
    for i, op in enumerate(script):
        if op[0] == "reindex":
            m.apply(op, i)
            marks.append(("reindex", []))
            by_slot.setdefault(op[1], []).append(len(marks) - 1)
            continue
        res = m.apply(op, i)
        cx = m.ctx[op[1]]
        lo, hi = m.range_of(op)
        if op[0] == "rx":
            marks.append(("rx", [(l, k0) for l, k0 in zip(res["life"], res["k0"])]))
        else:
            marks.append((op[0], [(cx.life[c], cx.life[c].n) for c in range(lo, hi)]))
        if op[0] == "save" and res:
            by_slot[op[4]] = [len(marks) - 1]
        if op[0] in ("join", "load"):
            for j in by_slot.get(op[2], []):
                marks[j][1].extend(marks[-1][1])
    m.evaluate(mode)
    seen = observed(m)
    counts = {}
    for kind, lives in marks:
        hit = any(any(k >= n for k in seen.get(id(l), ())) for l, n in lives)
        counts[kind] = counts.get(kind, 0) + int(hit)
    return counts, m


# ------------------------------------------------------------------ the GPU executor
class GpuRx:
    """sc.Receiver behind the runner's interface."""

    def __init__(self, nch, mode):
        self.rx = sc.Receiver(nch, mode=mode)
        self.nch = nch
        for k in ("reset", "reset_channels", "state_join", "state_load", "channel_frames", "close"):
            setattr(self, k, getattr(self.rx, k))

    def state_save(self, c0, n):
        return self.rx.state_save(c0, n)

    @property
    def frames(self):
        return self.rx.frames

    def run(self, form, x, codes, prev, cap):
        import torch
        rx, kind = self.rx, form[0]
        floor = min_sumsq()
        if kind == "dense" and form[1] == "host":
            return rx.demod(x, trace=True, soft=True)
        if kind == "dense":
            F = x.shape[1]
            o = {k: torch.empty(v.shape, dtype=getattr(torch, v.dtype.name), device="cuda")
                 for k, v in dense_zeros(self.nch, F).items()}
            rx.demod_device(torch.from_numpy(np.ascontiguousarray(x)).cuda(), o["bits"], o["valid"], o["trace"], o["soft"])
            rx.sync()
            return {k: v.cpu().numpy() for k, v in o.items()}
        if kind == "alaw":
            return rx.demod_fmt(codes, ALAW_I, trace=True, soft=True)
        if kind == "rec":
            return rx.demod_records(x, order=form[1], cap=cap, trace=True, soft=True)
        if kind == "alaw_sq":
            r = rx.demod_records_squelch_fmt(codes, ALAW_I, floor, prev=prev, order=form[1], trace=True, soft=True)
        elif form[1] == "host":
            r = rx.demod_records_squelch(x, floor, prev=prev, order=form[2], cap=cap, trace=True, soft=True)
        else:
            d_prev = torch.from_numpy(prev.copy().view(np.int64).reshape(self.nch, 2)).cuda()
            r = rx.demod_records_squelch_device(torch.from_numpy(np.ascontiguousarray(x)).cuda(), floor, prev=d_prev,
                                                order=form[2], cap=cap, trace=True, soft=True)
            rx.sync()
            return records_from_device(r)
        r["last"] = r.pop("prev")
        return r


def records_from_device(r):
    """The tensors of a device record call as the host forms return them."""
    count = int(r["count"].cpu().numpy().view(np.uint32)[0])
    cap = 0 if r["rec"] is None else r["rec"].shape[0]
    k = min(count, cap)
    out = {"count": count, "groups": r["groups"].cpu().numpy().view(np.uint32),
           "rec": sc.rec_from_tensor(r["rec"], k) if cap else np.zeros(0, sc.REC_DTYPE),
           "trace": r["trace"][:k].cpu().numpy(), "soft": r["soft"][:k].cpu().numpy()}
    if r.get("level") is not None:
        out["level"] = sc.level_from_tensor(r["level"])
        out["last"] = sc.level_from_tensor(r["prev"])
    return out


# ------------------------------------------------------------------ transmit scripts
TX_GAPS = {"T0": 0, "T1": 1, "T2": 903}
TX_FORMS = ("s16_device", "alaw", "ulaw_i")
TX_FMT = {"s16_device": sc.OUT_S16 | sc.OUT_PLANAR, "alaw": sc.OUT_ALAW | sc.OUT_PLANAR,
          "ulaw_i": sc.OUT_ULAW | sc.OUT_INTERLEAVED}


def call_mask(seed, nch, npk):
    """Mask rows drawn as call traffic: runs of 2-5 active slots separated by 1-3
    idle ones, from a random phase; nonzero values other than 1 among them."""
    rng = np.random.default_rng([seed, 5])
    m = np.zeros((nch, npk), np.uint8)
    for c in range(nch):
        s = -int(rng.integers(0, 6))
        while s < npk:
            run = int(rng.integers(2, 6))
            m[c, max(s, 0):max(s + run, 0)] = 1
            s += run + int(rng.integers(1, 4))
    return m * rng.choice(np.array([1, 2, 0x80, 0xFF], np.uint8), m.shape)


def call_starts(mask):
    """[nch][npk] bool: the first slot of each run of active slots."""
    a = mask != 0
    return a & ~np.concatenate([np.zeros((a.shape[0], 1), bool), a[:, :-1]], axis=1)


class TxModel:
    """Restated per context, with the index and last-dibits word of every channel."""

    def __init__(self, nch, gaps=None):
        self.gaps = dict(gaps or TX_GAPS)
        self.nch = nch
        self.r = {k: Restated(nch) for k in self.gaps}
        self.word = {k: np.zeros(nch, np.uint32) for k in self.gaps}
        self.slots_sent = {k: 0 for k in self.gaps}
        self.slots = {}

    def apply(self, op):
        kind, name = op[0], op[1]
        r = self.r[name]
        if kind == "tx":
            _, _, npk, mseed, form = op
            bits = payload(mseed, self.nch, npk)
            mask = None if mseed % 4 == 0 else call_mask(mseed, self.nch, npk)
            y = r.call(bits, self.gaps[name], mask)
            for c in range(self.nch):
                k = np.arange(npk) if mask is None else np.flatnonzero(mask[c])
                if k.size:
                    self.word[name][c] = last_dibits(bits[c, k[-1]])
            self.slots_sent[name] += npk
            return bits, mask, y
        if kind == "reset_channels":
            r.reset(op[2], op[3])
            self.word[name][op[2]:op[2] + op[3]] = 0
        elif kind == "save":
            lo, hi = op[2], op[2] + op[3]
            self.slots[op[4]] = (r.st[lo:hi].copy(), r.sent[lo:hi].copy(), self.word[name][lo:hi].copy())
        elif kind == "load":
            st, sent, word = self.slots[op[2]]
            lo, hi = op[3], op[3] + len(sent)
            r.st[lo:hi], r.sent[lo:hi], self.word[name][lo:hi] = st, sent, word
        return None


def gen_tx(seed, nch=24, max_slots=30, max_ops=20):
    rng = np.random.default_rng([seed, 2])
    names = list(TX_GAPS)
    script, nslot, left = [], 0, max_slots - 2 * len(names)
    sizes = {}
    for i in range(max_ops - len(names)):
        k = int(rng.integers(5)) if i % 2 else 0
        name = names[int(rng.integers(len(names)))]
        if k == 0 or (k >= 3 and not sizes):
            npk = int(rng.integers(1, 5))
            if npk > left:
                continue
            left -= npk
            script.append(("tx", name, npk, int(rng.integers(1, 1 << 20)), TX_FORMS[int(rng.integers(3))]))
        elif k == 1:
            c0 = int(rng.integers(nch))
            script.append(("reset_channels", name, c0, int(rng.integers(1, nch - c0 + 1))))
        elif k == 2:
            c0 = int(rng.integers(nch))
            sizes[nslot] = int(rng.integers(1, nch - c0 + 1))
            script.append(("save", name, c0, sizes[nslot], nslot))
            nslot += 1
        else:
            s = int(rng.integers(nslot))
            script.append(("load", name, s, int(rng.integers(nch - sizes[s] + 1))))
    for j, name in enumerate(names):
        script.append(("tx", name, 2, int(rng.integers(1, 1 << 20)) | 1, TX_FORMS[j]))
    return script


def run_tx(script, make, seed=None, nch=24):
    """Runs a transmit script on executors made by make(nch, gap); every call's
    block sample for sample against Restated, the counts after every op."""
    m = TxModel(nch)
    tx = {name: make(nch, gap) for name, gap in TX_GAPS.items()}
    snaps = {}
    try:
        for i, op in enumerate(script):
            where = f"seed {seed}, op {i} {op}"
            kind, name = op[0], op[1]
            t = tx[name]
            if kind == "tx":
                bits, mask, y = m.apply(op)
                got = t.run(op[4], bits, mask)
                exp = y if op[4] == "s16_device" else sc.output_convert_host(y, TX_FMT[op[4]])
                if op[4] != "s16_device":      # the tables of tests/g711.py, not the library's
                    enc = g711.compress(y, TX_FMT[op[4]] & 0x0f)
                    assert np.array_equal(exp, enc.T if op[4] == "ulaw_i" else enc), f"{where}: host conversion"
                if not np.array_equal(got, exp):
                    d = np.argwhere(got != exp)[0]
                    c, s = (d[1], d[0]) if op[4] == "ulaw_i" else (d[0], d[1])
                    P = PACKET + TX_GAPS[name]
                    raise AssertionError(f"{where}: samples differ, first at (channel, slot) ({int(c)}, {int(s) // P}), "
                                         f"sample {int(s) % P}: got {got[tuple(d)]}, expected {exp[tuple(d)]}")
            elif kind == "reset_channels":
                t.reset_channels(op[2], op[3])
                m.apply(op)
            elif kind == "save":
                m.apply(op)
                snaps[op[4]] = t.state_save(op[2], op[3])
                n, idx, words = snapshot_fields(snaps[op[4]])
                _, sent, word = m.slots[op[4]]
                assert n == op[3] and np.array_equal(idx, sent), f"{where}: snapshot indices {idx}, model {sent}"
                assert np.array_equal(words, word), f"{where}: snapshot dibits {words}, model {word}"
            else:
                t.state_load(snaps[op[2]], op[3])
                m.apply(op)
            assert t.packets() == m.slots_sent[name], f"{where}: packets {t.packets()}, model {m.slots_sent[name]}"
            got, want = t.channel_packets(), m.r[name].sent
            assert np.array_equal(got, want), f"{where}: channel_packets {got}, model {want}"
    finally:
        for t in tx.values():
            t.close()
    return m


class GpuTx:
    """sc.Transmitter behind the runner's interface: every form through the device entry points."""

    def __init__(self, nch, gap):
        self.tx = sc.Transmitter(nch, gap=gap)
        self.nch, self.gap = nch, gap
        for k in ("reset_channels", "state_save", "state_load", "packets", "channel_packets", "close"):
            setattr(self, k, getattr(self.tx, k))

    def run(self, form, bits, mask):
        import torch
        n = bits.shape[1] * (PACKET + self.gap)
        d_bits = torch.from_numpy(np.array(bits)).cuda()
        d_m = None if mask is None else torch.from_numpy(np.array(mask)).cuda()
        if form == "s16_device":
            out = torch.zeros((self.nch, n), dtype=torch.int16, device="cuda")
            self.tx.modulate_device(d_bits, out, active=d_m)
        else:
            shape = (n, self.nch) if form == "ulaw_i" else (self.nch, n)
            out = torch.zeros(shape, dtype=torch.uint8, device="cuda")
            self.tx.modulate_device_fmt(d_bits, out, TX_FMT[form], active=d_m)
        self.tx.sync()
        return out.cpu().numpy()


# ------------------------------------------------------------------------ the exchange
EX_NCH, EX_SLOTS, EX_LD = 32, 14, 48


def exchange_plan(seed, gap):
    """The composite case, from the host side alone: a masked transmitter writes
    an A-law trunk, a receiver restarts its channels where the calls start.
    Returns the mask, payload, the line as the receiver decodes it
    [nch][frames][1880], the receive calls' frame cuts and per cut the channels
    that restart there."""
    P = PACKET + gap
    mask, bits = call_mask(seed, EX_NCH, EX_SLOTS), payload(seed + 1, EX_NCH, EX_SLOTS)
    starts = call_starts(mask)
    r = Restated(EX_NCH)
    rows = []
    for s in range(EX_SLOTS):
        for c in np.flatnonzero(starts[:, s]):
            r.reset(int(c), 1)
        rows.append(r.call(bits[:, s:s + 1], gap, mask[:, s:s + 1]))
    line, _ = quantize_alaw(np.concatenate(rows, axis=1))
    nf = EX_SLOTS * P // FRAME
    line = line[:, :nf * FRAME].reshape(EX_NCH, nf, FRAME)
    restart = {}                                # frame -> channels that restart in front of it
    for c, s in np.argwhere(starts):
        f = P * int(s) // FRAME
        if f < nf:
            restart.setdefault(f, set()).add(int(c))
    cuts = sorted(set(restart) | {0, nf})
    return {"mask": mask, "bits": bits, "starts": starts, "line": line, "nf": nf, "cuts": cuts,
            "restart": {f: sorted(v) for f, v in restart.items()}}


def exchange_expected(plan, mode=0):
    """Per receive call (f0, f1): the records, levels and `last` the header text
    gives, from the oracle on every channel's segment; and the observed calls."""
    nf, line = plan["nf"], plan["line"]
    seg0 = np.zeros((EX_NCH, nf), np.int64)     # the frame each channel's current segment started at
    for c in range(EX_NCH):
        st = sorted({0} | {f for f, cs in plan["restart"].items() if c in cs})
        for a, b in zip(st, st[1:] + [nf]):
            seg0[c, a:b] = a
    dense = dense_zeros(EX_NCH, nf)
    by_len, calls_seen, ncalls = {}, 0, 0
    for c in range(EX_NCH):
        for a in np.unique(seg0[c]):
            b = int(np.flatnonzero(seg0[c] == a)[-1]) + 1
            by_len.setdefault(b - int(a), []).append((c, int(a), b))
    for n, segs in by_len.items():
        e = rxcheck.expected(np.stack([line[c, a:b] for c, a, b in segs]), mode)
        for i, (c, a, b) in enumerate(segs):
            for k in rxcheck.KEYS:
                dense[k][c, a:b] = e[k][i]
            if a or 0 in plan["restart"] and c in plan["restart"][0]:
                ncalls += 1
                calls_seen += int(((e["valid"][i] != 0) & (e["trace"][i, :, 1] < 128)).any())
    level = levels_np(line)
    out = []
    for f0, f1 in zip(plan["cuts"][:-1], plan["cuts"][1:]):
        prev = np.zeros(EX_NCH, sc.LEVEL_DTYPE)
        if f0:
            prev = level[:, f0 - 1].copy()
            prev[plan["restart"].get(f0, [])] = 0
        d = {k: v[:, f0:f1] for k, v in dense.items()}
        valid = gate_np(level[:, f0:f1], prev, d["valid"], min_sumsq())
        r = records_np(d, valid, sc.REC_BY_FRAME, None)
        r["level"], r["last"] = level[:, f0:f1], level[:, f1 - 1]
        out.append(r)
    gated = gate_np(level, np.zeros(EX_NCH, sc.LEVEL_DTYPE), dense["valid"], min_sumsq())
    stats = {"calls": ncalls, "observed": calls_seen, "valid": int((dense["valid"] != 0).sum()),
             "below the gate": int(((dense["valid"] != 0) & (level["sumsq"] < min_sumsq())).sum()),
             "squelched": int(((dense["valid"] != 0) & (gated == 0)).sum())}
    return out, stats


def run_exchange(seed, gap, mode=0):
    """The exchange on the GPU: one device buffer, written by Transmitter.modulate_device_fmt
    slot by slot and read by Receiver.demod_records_squelch_device_fmt call by call.
    ld = 48: a trunk wider than the 32 channels; 8-bit codes may lie at any
    address, so every frame row [1880 f][0..32) meets the receive call's contract."""
    import torch
    plan = exchange_plan(seed, gap)
    exp, stats = exchange_expected(plan, mode)
    P, fmt = PACKET + gap, sc.OUT_ALAW | sc.OUT_INTERLEAVED
    trunk = torch.full((EX_SLOTS * P, EX_LD), 0x5A, dtype=torch.uint8, device="cuda")
    tx = sc.Transmitter(EX_NCH, gap=gap)
    d_bits, d_mask = torch.from_numpy(plan["bits"]).cuda(), torch.from_numpy(plan["mask"]).cuda()
    for s in range(EX_SLOTS):
        for c in np.flatnonzero(plan["starts"][:, s]):
            tx.reset_channels(int(c), 1)
        tx.modulate_device_fmt(d_bits[:, s:s + 1].contiguous(), trunk[s * P:(s + 1) * P, :EX_NCH], fmt,
                               active=d_mask[:, s:s + 1].contiguous())
    tx.sync()
    assert (trunk[:, EX_NCH:] == 0x5A).all(), "the transmitter wrote outside its 32 columns"
    rx = sc.Receiver(EX_NCH, mode=mode)
    d_prev = torch.zeros((EX_NCH, 2), dtype=torch.int64, device="cuda")
    try:
        for j, (f0, f1) in enumerate(zip(plan["cuts"][:-1], plan["cuts"][1:])):
            for c in plan["restart"].get(f0, []):
                rx.reset_channels(c, 1)
                d_prev[c] = 0
            r = rx.demod_records_squelch_device_fmt(trunk[f0 * FRAME:f1 * FRAME, :EX_NCH], ALAW_I, min_sumsq(),
                                                    prev=d_prev, order=sc.REC_BY_FRAME, trace=True, soft=True)
            rx.sync()
            call = {"op": j, "tuple": ("exchange", gap, f0, f1), "rec": exp[j], "F": f1 - f0,
                    "form": ("sq", "device", sc.REC_BY_FRAME, None)}
            compare_call(seed, call, records_from_device(r))
    finally:
        rx.close()
        tx.close()
    return stats


# -------------------------------------------------------------------------- replay
def replay(script, side="rx", mode=0, seed=None, make=None):
    """Runs a script, or a prefix script[:k] of one, as the tests do (on the GPU
    unless `make` gives another executor): the same difference, the same message."""
    if side == "rx":
        return run_rx(script, make or GpuRx, mode, seed, snapshots=True)
    return run_tx(script, make or GpuTx, seed)
