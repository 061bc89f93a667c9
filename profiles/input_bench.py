#!/usr/bin/env python3
"""The input conversion (include/qpsk_input.h) against the copy ceiling, and
the streaming rate of 8-bit interleaved input against planar int16, in one
process on one GPU.  Prints one JSON line and writes it to --out (a copy is
committed as profiles/input_bench.json and cited by README.md and DESIGN.md).

    python profiles/input_bench.py [--channels 65536] [--frames 32] [--steps 10] [--warmup 2]
                                   [--stream-frames 4] [--stream-chunks 30] [--rounds 3]
                                   [--out profiles/input_bench.json]

Converter: each of the five formats that are not the receive path's own
(planar A-law and mu-law, interleaved int16, A-law and mu-law; ld = channels),
G.711 with both decoders (the integer expansion and the LDS table), timed with
HIP events around the enqueue, alternated step by step after a warm-up; beside
them a hipMemcpyAsync device-to-device of the int16 output block, the
practical ceiling of moving its bytes once.  GB/s counts the bytes read plus
the bytes written.

Streaming: channels x stream-frames per chunk, 3 slots, the planar int16
stream (qpsk_stream_create_mode) and the interleaved A-law stream
(qpsk_stream_create_fmt), `rounds` times one after the other on the same box.
A round submits stream-chunks chunks whose pinned slots were filled once
(filling them is the caller's work in both cases and is left out) and is timed
by the host clock from the first submit to the last retrieve.  There is no CPU
fallback: without a GPU this fails.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hip_runtime():
    """The HIP runtime this process already has loaded (torch's)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def fill_random(t):
    """random bytes into a uint8 cuda tensor of any size, 2^30 at a time"""
    flat = t.view(-1)
    for i in range(0, flat.numel(), 1 << 30):
        flat[i:i + (1 << 30)].random_(0, 256)


def converter(args, sc, torch, hip):
    nch, nf = args.channels, args.frames
    T = nf * sc.FRAME_SIZE
    n = nch * T
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    L = sc.lib()
    out = torch.empty(n, dtype=torch.int16, device=dev)
    src = torch.empty(2 * n, dtype=torch.uint8, device=dev)   # n int16 or n codes
    fill_random(src)
    legs = {}

    def conv(fmt, dec):
        def run():
            sc._check(L.qpsk_input_convert_device_dec(fmt, src.data_ptr(), nch, nch, nf, out.data_ptr(), sp, dec))
        return run

    names = {sc.IN_ALAW: "alaw", sc.IN_ULAW: "ulaw", sc.IN_S16: "s16"}
    for lay, lname in ((sc.IN_PLANAR, "planar"), (sc.IN_INTERLEAVED, "interleaved")):
        for enc in (sc.IN_S16, sc.IN_ALAW, sc.IN_ULAW):
            if enc == sc.IN_S16 and lay == sc.IN_PLANAR:
                continue
            for dec, dname in ((0, "arith"), (1, "table")):
                if enc == sc.IN_S16 and dec:
                    continue
                key = f"{names[enc]}_{lname}" + ("" if enc == sc.IN_S16 else f"_{dname}")
                legs[key] = (conv(enc | lay, dec), n * (2 if enc == sc.IN_S16 else 1) + 2 * n)

    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    def memcpy():
        rc = hip.hipMemcpyAsync(out.data_ptr(), src.data_ptr(), 2 * n, 3, sp)   # hipMemcpyDeviceToDevice
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync: {rc}")

    legs["memcpy_d2d"] = (memcpy, 4 * n)
    ms = {k: [] for k in legs}
    for step in range(args.warmup + args.steps):
        for name, (fn, _) in legs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            if step >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))
    ceiling = statistics.median(ms["memcpy_d2d"])
    res = {}
    for name, (_, nbytes) in legs.items():
        med = statistics.median(ms[name])
        res[name] = {"ms": spread(ms[name]), "bytes_moved": nbytes, "gb_per_s": nbytes / (med * 1e-3) / 1e9,
                     "ms_over_memcpy_ms": med / ceiling}
    del out, src
    torch.cuda.empty_cache()
    return {"channels": nch, "frames": nf, "samples": n, "output_bytes": 2 * n, "steps": args.steps,
            "warmup": args.warmup, "legs": res}


def stream_round(sc, st, nchunk, filled, fill):
    """Msamples/s of nchunk chunks through the stream st"""
    import numpy as np  # noqa: F401
    per_chunk = st.nch * st.frames * sc.FRAME_SIZE
    # warm-up: every slot once (and filled, the first time round)
    for k in range(st.nslot):
        buf = st.acquire_raw()
        if k not in filled:
            fill(buf)
            filled.add(k)
        st.submit()
    while st.pending:
        st.retrieve(copy=False)
    t0 = time.perf_counter()
    for _ in range(nchunk):
        if st.pending == st.nslot:
            st.retrieve(copy=False)
        st.acquire_raw()
        st.submit()
    while st.pending:
        st.retrieve(copy=False)
    dt = time.perf_counter() - t0
    return nchunk * per_chunk / dt / 1e6


def streaming(args, sc, torch):
    import numpy as np
    nch, nf = args.channels, args.stream_frames
    small = 64
    assert nch % small == 0
    x = sc.synth(3, small, nf, 8.0)                                    # [64][nf][1880]
    tab = np.array([sc.input_convert_host(np.full((1, sc.FRAME_SIZE), c, np.uint8), sc.IN_ALAW, 1)[0, 0, 0]
                    for c in range(256)], np.int64)
    order = np.argsort(tab, kind="stable")
    vals = tab[order]
    flat = x.reshape(small, -1).astype(np.int64)
    i = np.clip(np.searchsorted(vals, flat), 1, 255)
    i = np.where(np.abs(vals[i - 1] - flat) <= np.abs(vals[i] - flat), i - 1, i)
    codes_t = np.ascontiguousarray(order[i].astype(np.uint8).T)        # [T][64]

    def fill_s16(buf):   # [nch][T]
        buf.reshape(nch // small, small, -1)[...] = x.reshape(1, small, -1)

    def fill_alaw(buf):  # [T][nch]
        buf.reshape(buf.shape[0], nch // small, small)[...] = codes_t[:, None, :]

    fmt = sc.IN_ALAW | sc.IN_INTERLEAVED
    streams = {"s16_planar": (sc.Stream(nch, nf, nslot=3), fill_s16, set()),
               "alaw_interleaved": (sc.Stream(nch, nf, nslot=3, fmt=fmt), fill_alaw, set())}
    rates = {k: [] for k in streams}
    for _ in range(args.rounds):
        for name, (st, fill, filled) in streams.items():
            rates[name].append(stream_round(sc, st, args.stream_chunks, filled, fill))
    for st, _, _ in streams.values():
        st.close()
    faster = [a > s for a, s in zip(rates["alaw_interleaved"], rates["s16_planar"])]
    return {"channels": nch, "frames_per_chunk": nf, "slots": 3, "chunks_per_round": args.stream_chunks,
            "rounds": args.rounds, "msamples_per_s": rates,
            "pcie_bytes_per_sample": {"s16_planar": 2, "alaw_interleaved": 1},
            "alaw_over_s16": [a / s for a, s in zip(rates["alaw_interleaved"], rates["s16_planar"])],
            "alaw_faster_in_every_round": all(faster)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stream-frames", type=int, default=4)
    ap.add_argument("--stream-chunks", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_bench.json"))
    args = ap.parse_args()

    import torch

    import singlecarrier_amd as sc

    if not torch.cuda.is_available():
        raise SystemExit("input_bench: no GPU")
    hip = hip_runtime()
    res = {"bench": "input_formats", "device": torch.cuda.get_device_name(0), "kernel_hash": sc.kernel_hash(),
           "converter": converter(args, sc, torch, hip), "streaming": streaming(args, sc, torch)}
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
