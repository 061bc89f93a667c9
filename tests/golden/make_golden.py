"""Generate the golden fixtures in tests/golden/ from the UNMODIFIED reference.

Runs in the build container only (needs /root/reference and oracle/_ref, built
by `make -C oracle ref`).  Inputs are either the reference's own data file
(preamble_qpsk_8k.raw, copied here as a data fixture) or synthetic channel
streams regenerated from a seed by the oracle's TX restatement (the input's
sha256 is stored so the generator itself is pinned).  Every expected output
below comes from oracle/_ref/libqpsk_ref.so, i.e. the reference's own code.

    python tests/golden/make_golden.py            # everything
    python tests/golden/make_golden.py --dec752   # only the dec752-mode fixtures
    python tests/golden/make_golden.py --hostile  # only hostile_ref.npz
    python tests/golden/make_golden.py --hostile-sweep   # re-choose hostile_params.json, then --hostile
    python tests/golden/make_golden.py --spacing  # only spacing_ref.json

The dec752 fixtures ("intended semantics"; NOT reference
parity) come from oracle/_ref/libqpsk_ref752.so: the same unmodified reference
sources, linked so that decimated_frame owns the 752 entries its decimation
loop writes (oracle/ref/dec752.ld).
"""
import hashlib
import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import oracle  # noqa: E402

SYNTH_CASES = [  # (name, seed, nch, nframes, ebn0_db)
    ("synth_s1_clean", 1, 64, 16, 1000.0),
    ("synth_s2_eb8", 2, 64, 16, 8.0),
    ("synth_s3_eb4", 3, 64, 16, 4.0),
    ("synth_s4_eb0", 4, 64, 16, 0.0),
]


# src/constants.c:25-42
PREAMBLE = [-1, 1, 1, -1, -1, 1, 1, 1, -1, 1, -1, -1, 1, 1, -1, -1, 1, 1, -1, 1, -1, -1, 1, -1,
            1, -1, 1, -1, 1, -1, 1, 1, 1, -1, 1, 1, 1, 1, -1, -1, 1, -1, -1, 1, 1, -1, 1, -1,
            1, 1, -1, 1, -1, -1, 1, -1, -1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, -1, -1, 1, 1, -1,
            1, 1, -1, -1, 1, 1, -1, 1, 1, -1, 1, 1, -1, -1, -1, 1, -1, 1, -1, 1, -1, -1, -1, 1,
            -1, -1, 1, -1, 1, 1, -1, -1, -1, -1, -1, 1, 1, 1, -1, 1, 1, -1, 1, 1, -1, -1, 1, 1,
            -1, 1, -1, 1, -1, -1, -1, 1]


DEC752_CASES = [  # (name, seed, nch, nframes, ebn0_db)
    ("synth_d752_s1_clean", 11, 48, 16, 1000.0),
    ("synth_d752_s2_eb4", 12, 48, 16, 4.0),
]


def bitstr(b):
    return "".join(str(int(v)) for v in b)


def _synth_golden(name, seed, nch, nfr, eb, mode):
    xs = oracle.synth(seed, nch, nfr, eb)
    b, v, t = oracle.ref_rx(xs, trace=True, mode=mode)
    soft = np.where(v[..., None, None].astype(bool), t["soft"], 0).astype(np.float32)
    np.savez_compressed(
        os.path.join(HERE, name + ".npz"), seed=seed, nch=nch, nframes=nfr, ebn0_db=eb,
        mode=mode, input_sha256=hashlib.sha256(xs.tobytes()).hexdigest(),
        bits=np.packbits(b, axis=-1), valid=v, max_index=t["max_index"],
        matches=t["matches"], rx_timing=t["rx_timing"], soft=soft)
    print(name, "valid frac %.3f" % v.mean())


def dec752():
    """Fixtures of the dec752 mode from the layout-padded reference build."""
    assert oracle.ref_available(oracle.MODE_DEC752)
    raw = np.fromfile(os.path.join(HERE, "preamble_qpsk_8k.raw"), np.int16)
    nf = raw.size // oracle.FRAME
    x = raw[: nf * oracle.FRAME].reshape(1, nf, oracle.FRAME)
    bits, valid, tr = oracle.ref_rx(x, trace=True, mode=oracle.MODE_DEC752)
    recs = b"".join(np.concatenate([bits[0, n], np.zeros(496 - 62, np.uint8)]).tobytes()
                    for n in range(nf) if valid[0, n])
    exp = {
        "mode": "dec752 (decimated_frame[752]; not reference parity)",
        "input": "preamble_qpsk_8k.raw",
        "input_md5": hashlib.md5(raw.tobytes()).hexdigest(),
        "frames": int(nf),
        "output_bytes": len(recs),
        "output_md5": hashlib.md5(recs).hexdigest(),
        "trace": [{k: int(tr[0, n][k]) for k in ("max_index", "matches", "valid", "rx_timing")}
                  for n in range(nf)],
        "soft": {str(n): tr[0, n]["soft"].tolist() for n in range(nf) if valid[0, n]},
    }
    with open(os.path.join(HERE, "sample_expected_dec752.json"), "w") as f:
        json.dump(exp, f, indent=1)
    for name, seed, nch, nfr, eb in DEC752_CASES:
        _synth_golden(name, seed, nch, nfr, eb, oracle.MODE_DEC752)
    print("sample (dec752):", exp["output_md5"], exp["output_bytes"], "B")


# ------------------------------------------------------------ hostile corpus
# tests/hostile.py's parameter table and its reference-made golden.
HOSTILE_AMPS = [32767, 30000, 20000, 10000, 3000]
HOSTILE_GOLDEN = (32, 8)   # channels x frames of hostile_ref.npz (the table's first rows)


def _hostile_candidates(n, seed):
    """n candidate wave rows: every second one a single triangle (the family
    with the most channels on which the Annex G recovery is observable), the
    others cycling through squares, two-wave sums and gated triangles."""
    rng = np.random.default_rng(seed)

    def one(kind):
        return {"kind": kind, "k": int(rng.integers(800, 32001)),
                "p": int(rng.integers(0, 65536)), "a": int(rng.choice(HOSTILE_AMPS))}

    rows = []
    for i in range(n):
        kind = ["tri", "square", "tri2", "sq2", "sqtri", "gated"][i % 6] if i % 2 else "tri"
        if kind in ("tri", "square"):
            r = one(kind)
        elif kind == "gated":
            r = dict(one("tri"), gate=int(rng.integers(4, 40)))
        else:
            r = {"sum": [one({"tri2": "tri", "sq2": "square", "sqtri": "square"}[kind]),
                         one("square" if kind == "sq2" else "tri")]}
        rows.append(r)
    return rows


def _differs(a, b):
    """[nch][nframes] mask: any documented output differs (soft: valid frames, bitwise)."""
    (b1, v1, t1), (b2, v2, t2) = a, b
    m = (v1 != v2) | (b1 != b2).any(-1)
    for k in ("max_index", "matches", "rx_timing"):
        m |= t1[k] != t2[k]
    soft = (t1["soft"].view(np.uint32) != t2["soft"].view(np.uint32)).any((-1, -2))
    return m | (v1.astype(bool) & v2.astype(bool) & soft)


def _hostile_impaired():
    rows = []
    for i, (d, num) in enumerate((d, num) for d in (3, 7, 25, 60) for num in (2, -2, 1)):
        rows.append({"kind": "echo", "seed": 301, "c": i, "d": d, "num": num})
    for i, g in enumerate((4, 100, 4, 100, 4, 100)):
        rows.append({"kind": "gain", "seed": 302, "c": i, "g": g})
    for i, o in enumerate((5000, -5000, 12000, -12000, 20000, -20000)):
        rows.append({"kind": "dc", "seed": 303, "c": i, "o": o})
    for i, at in enumerate((2000, 3000, 5000, 7000, 9400, 11000, 13000, 15000)):
        rows.append({"kind": "step", "seed": 304, "c": i, "at": at, "sh": 10})
    return rows


def hostile_sweep(ncand=6144, seed=20):
    """Choose the rows of tests/golden/hostile_params.json.  Every measurement
    below is on the unmodified reference (oracle/_ref) and on the restatement
    with qc_naive_cmul set, never on the code under test:
      sensitive channel-frame: the naive-product restatement departs from the
        reference there (reference mode, or dec752 for the second set);
      non-finite valid frame: the reference calls it valid and its soft
        symbols hold an inf or a NaN."""
    import ctypes
    sys.path.insert(0, os.path.dirname(HERE))
    import hostile
    assert oracle.ref_available() and oracle.ref_available(oracle.MODE_DEC752)
    flag = ctypes.c_int.in_dll(oracle.cpu_lib(), "qc_naive_cmul")
    rows = _hostile_candidates(ncand, seed)
    x = hostile.waves(rows)
    sens = {}
    for mode in (oracle.MODE_REF, oracle.MODE_DEC752):
        ref = oracle.ref_rx(x, trace=True, mode=mode)
        flag.value = 1
        try:
            naive = oracle.cpu_rx(x, trace=True, mode=mode)
        finally:
            flag.value = 0
        sens[mode] = _differs(naive, ref)
        if mode == oracle.MODE_REF:
            nonfin = ref[1].astype(bool) & ~np.isfinite(ref[2]["soft"]).all((-1, -2))
    s0, s1 = sens[oracle.MODE_REF], sens[oracle.MODE_DEC752]
    gch, gfr = HOSTILE_GOLDEN
    chosen = []

    def take(mask, n, exact=True):
        """Append up to n not yet chosen candidates of mask; the rows whose
        position the tests rely on must all be found (exact)."""
        got = 0
        for c in np.where(mask)[0]:
            if got == n:
                break
            if c not in chosen:
                chosen.append(int(c))
                got += 1
        assert got == n or not exact, (got, n)
        return got

    take(s0[:, :4].any(1), 8)             # rows 0..7: the tiny host call (4 frames)
    take(s0[:, :gfr].any(1), 12)          # the golden's sensitive channels ...
    nsens = len(chosen)                   # rows 0..nsens-1: sensitive inside the golden's frames
    assert s0[chosen, :gfr].any(1).all() and s0[chosen[:8], :4].any(1).all()
    take(nonfin[:, :gfr].any(1), 8)       # ... its non-finite valid ones ...
    take(s1[:, :gfr].any(1), 4)           # ... and dec752-only ones: 32 rows
    assert len(chosen) == gch
    take(s0.any(1), 36)
    take(nonfin.any(1), 16, exact=False)  # all there are
    take(s1.any(1), 28)
    take(np.ones(len(rows), bool), 160 - len(chosen))   # the rest: the families as they come
    assert len(chosen) == 160
    out = {"nframes": hostile.NFRAMES,
           "golden": {"channels": gch, "frames": gfr, "sensitive": nsens},
           "wave": [rows[c] for c in chosen], "impaired": _hostile_impaired()}
    with open(hostile.PARAMS, "w") as f:
        f.write("{\n")
        for k in ("nframes", "golden"):
            f.write(' "%s": %s,\n' % (k, json.dumps(out[k])))
        for k in ("wave", "impaired"):
            f.write(' "%s": [\n  ' % k + ",\n  ".join(json.dumps(r) for r in out[k])
                    + ("\n ],\n" if k == "wave" else "\n ]\n"))
        f.write("}\n")
    print("hostile sweep: %d candidates, sensitive cf %d / ch %d (ref), %d / %d (dec752), "
          "non-finite valid frames %d in %d ch" % (ncand, s0.sum(), s0.any(1).sum(), s1.sum(),
                                                   s1.any(1).sum(), nonfin.sum(), nonfin.any(1).sum()))
    print("chosen: sensitive cf %d / ch %d, non-finite valid %d / ch %d" % (
        s0[chosen].sum(), s0[chosen].any(1).sum(), nonfin[chosen].sum(), nonfin[chosen].any(1).sum()))


def hostile_golden():
    """tests/golden/hostile_ref.npz: the reference's outputs (both builds) on
    the first rows and frames of the corpus, soft symbols of valid frames only."""
    sys.path.insert(0, os.path.dirname(HERE))
    import hostile
    gch, gfr = HOSTILE_GOLDEN
    x = np.ascontiguousarray(hostile.waves(hostile.params()["wave"][:gch], gfr))
    out = {"input_sha256": hashlib.sha256(x.tobytes()).hexdigest()}
    for tag, mode in (("ref", oracle.MODE_REF), ("d752", oracle.MODE_DEC752)):
        b, v, t = oracle.ref_rx(x, trace=True, mode=mode)
        vm = v.astype(bool)
        out.update({tag + "_bits": np.packbits(b, axis=-1), tag + "_valid": v,
                    tag + "_max_index": t["max_index"].astype(np.int16),
                    tag + "_matches": t["matches"].astype(np.int16),
                    tag + "_rx_timing": t["rx_timing"].astype(np.int16),
                    tag + "_soft": t["soft"][vm].view(np.uint32)})   # bit patterns: NaNs kept
        print("hostile golden", tag, "valid", int(vm.sum()), "non-finite valid",
              int((~np.isfinite(t["soft"][vm]).all((-1, -2))).sum()))
    np.savez_compressed(os.path.join(HERE, "hostile_ref.npz"), **out)


def spacing_golden():
    """tests/golden/spacing_ref.json: sha256 digests of the reference's outputs
    (both builds) over the whole corpus of tests/spacing.py, soft symbols of
    invalid frames zeroed, and of the corpus's samples."""
    sys.path.insert(0, os.path.dirname(HERE))
    import spacing
    x = spacing.corpus()
    out = {"channels": int(x.shape[0]), "frames": int(x.shape[1]),
           "input_sha256": hashlib.sha256(x.tobytes()).hexdigest(), "modes": {}}
    for mode in (oracle.MODE_REF, oracle.MODE_DEC752):
        assert oracle.ref_available(mode)
        b, v, t = oracle.ref_rx(x, trace=True, mode=mode)
        out["modes"][str(mode)] = spacing.digests(b, v, t)
        print("spacing golden mode", mode, "valid", int(v.sum()), "of", v.size)
    with open(os.path.join(HERE, "spacing_ref.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    oracle.build(ref=True)
    if "--spacing" in sys.argv[1:]:
        return spacing_golden()
    if "--hostile-sweep" in sys.argv[1:]:
        hostile_sweep()
        return hostile_golden()
    if "--hostile" in sys.argv[1:]:
        return hostile_golden()
    if "--dec752" in sys.argv[1:]:
        return dec752()
    assert oracle.ref_available()
    # 1. the reference's sample capture, through the reference driver semantics
    src = "/root/reference/preamble_qpsk_8k.raw"
    dst = os.path.join(HERE, "preamble_qpsk_8k.raw")
    shutil.copyfile(src, dst)
    raw = np.fromfile(dst, np.int16)
    nf = raw.size // oracle.FRAME
    x = raw[: nf * oracle.FRAME].reshape(1, nf, oracle.FRAME)
    bits, valid, tr, log = oracle.ref_rx(x, trace=True, log=True)
    recs = b"".join(np.concatenate([bits[0, n], np.zeros(496 - 62, np.uint8)]).tobytes()
                    for n in range(nf) if valid[0, n])
    dec, mixed, _, _ = oracle.ref_stages(x)
    exp = {
        "input": "preamble_qpsk_8k.raw",
        "input_md5": hashlib.md5(raw.tobytes()).hexdigest(),
        "frames": int(nf),
        "output_bytes": len(recs),
        "output_md5": hashlib.md5(recs).hexdigest(),
        "trace": [{k: int(tr[0, n][k]) for k in ("max_index", "matches", "valid", "rx_timing")}
                  for n in range(nf)],
        "valid_bits": {str(n): bitstr(bits[0, n]) for n in range(nf) if valid[0, n]},
        "debug2": log.splitlines(),
    }
    with open(os.path.join(HERE, "sample_expected.json"), "w") as f:
        json.dump(exp, f, indent=1)
    np.savez_compressed(os.path.join(HERE, "sample_stages.npz"), dec=dec,
                        soft=tr[0]["soft"], valid=valid[0])

    # 2. KATs straight from the reference: mixer table and keystream
    ones = np.full((1, 2, oracle.FRAME), 16384, np.int16)   # x/16384 == 1
    _, mixed1, _, _ = oracle.ref_stages(ones)
    nz = 530                                                 # 530*62 > 32767 + 62
    zb, zv, _ = oracle.ref_rx(np.zeros((1, nz, oracle.FRAME), np.int16))
    assert zv.all(), "all-zero frames are always valid (matches == 128)"
    np.savez_compressed(os.path.join(HERE, "kat.npz"), mixer_frame0=mixed1[0],
                        mixer_frame1=mixed1[1], keystream=zb[0].reshape(-1))

    # 3. seeded synthetic channels (noiseless and AWGN)
    for name, seed, nch, nfr, eb in SYNTH_CASES:
        _synth_golden(name, seed, nch, nfr, eb, oracle.MODE_REF)
    # 4. reference transmitter (src/qpsk.c:278-342): 3 packets, seeded dibits
    pre = np.array([complex(p, p) for p in PREAMBLE], np.complex64)
    rng = np.random.default_rng(42)
    syms = []
    for _ in range(3):
        syms.append((pre, True))
        for _ in range(8):
            d = rng.integers(0, 4, 31)
            syms.append((np.array([complex(-1 if v >> 1 else 1, -1 if v & 1 else 1) for v in d],
                                  np.complex64), False))
    out = oracle.ref_tx(syms)
    np.savez_compressed(os.path.join(HERE, "tx_golden.npz"),
                        symbols=np.concatenate([s for s, _ in syms]),
                        preamble=np.array([p for _, p in syms]),
                        lengths=np.array([len(s) for s, _ in syms]), samples=np.concatenate(out))
    print("sample:", exp["output_md5"], exp["output_bytes"], "B")
    dec752()
    hostile_golden()
    spacing_golden()


if __name__ == "__main__":
    main()
