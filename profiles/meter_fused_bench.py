#!/usr/bin/env python3
"""The level meter inside the input conversion (qpsk_input_convert_level_device,
include/qpsk_input.h) against the two passes it replaces, in one process on one
GPU.  Prints one JSON line and writes it to --out (a copy is committed as
profiles/meter_fused_bench.json and cited by DESIGN.md).

    python profiles/meter_fused_bench.py [--channels 65536] [--frames 32] [--steps 7] [--warmup 2] [--rounds 3]
                                         [--stream-frames 4] [--stream-chunks 12] [--squelch-db -60]
                                         [--out profiles/meter_fused_bench.json]

The input is the benchmark's (synth_device(seed 3), noiseless), compressed on
the device to each format: planar A-law, interleaved A-law, interleaved int16.
Per format, timed with HIP events around the enqueue and alternated step by
step after a warm-up; `rounds` rounds, the median of each:
  convert          (a) qpsk_input_convert_device alone: the control against
                   profiles/input_bench.json
  convert_meter    (b) (a) followed by qpsk_level_device: today's composition
  fused            (c) qpsk_input_convert_level_device, its fold launch included
  records_two      convert + qpsk_rx_batch_records_squelch_device
  records_fmt      qpsk_rx_batch_records_squelch_device_fmt
`fused_below_composition_every_round` is the condition under which a format's
fused kernel stays the default of the squelched calls.

Streams: a plain record stream and a squelch record stream, both interleaved
A-law with 3 slots, `stream-chunks` chunks of `stream-frames` frames through
each by the host clock (PCIe inbound binds both).
There is no CPU fallback: without a GPU this fails.
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


def rounds_of(legs, rounds, warmup, steps, timed):
    """{leg: [the median ms of each round]}; the legs alternate step by step"""
    out = {k: [] for k in legs}
    for _ in range(rounds):
        ms = {k: [] for k in legs}
        for step in range(warmup + steps):
            for name, fn in legs.items():
                t = timed(fn)
                if step >= warmup:
                    ms[name].append(t)
        for k in legs:
            out[k].append(statistics.median(ms[k]))
    return out


def format_legs(args, sc, torch, x, fmt, name):
    nch, nf = args.channels, args.frames
    cf, T = nch * nf, nf * sc.FRAME_SIZE
    dev = x.device
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    L = sc.lib()
    inter = bool(fmt & sc.IN_INTERLEAVED)
    dt = torch.int16 if (fmt & 0x0f) == sc.IN_S16 else torch.uint8
    src = torch.empty((T, nch) if inter else (nch, T), dtype=dt, device=dev)
    sc.output_convert_device(x.view(nch, T), fmt, src)
    out = torch.empty((nch, nf, sc.FRAME_SIZE), dtype=torch.int16, device=dev)
    level = torch.empty((nch, nf, 2), dtype=torch.int64, device=dev)
    need = sc.input_level_work_bytes(fmt, nch, nf, nch)
    work = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    p, o, lv, w = src.data_ptr(), out.data_ptr(), level.data_ptr(), work.data_ptr()

    def convert():
        sc._check(L.qpsk_input_convert_device(fmt, p, nch, nch, nf, o, sp))

    def convert_meter():
        convert()
        sc._check(L.qpsk_level_device(o, cf, lv, sp))

    def fused():
        sc._check(L.qpsk_input_convert_level_device(fmt, p, nch, nch, nf, o, lv, w if need else None, need, sp))

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # the two ways give the same bytes before anything is timed
    convert_meter()
    torch.cuda.synchronize()
    ref_out, ref_level = out.clone(), level.clone()
    out.zero_()
    level.zero_()
    fused()
    torch.cuda.synchronize()
    same = bool(torch.equal(out, ref_out)) and bool(torch.equal(level, ref_level))
    del ref_out, ref_level
    passes = rounds_of({"convert": convert, "convert_meter": convert_meter, "fused": fused}, args.rounds, args.warmup,
                       args.steps, timed)

    # end to end: the squelched record call, converted in front of it or inside it
    min_sumsq = sc.sumsq_of_dbfs(args.squelch_db)
    rec = torch.empty((cf, 2), dtype=torch.int64, device=dev)
    groups = torch.empty(nch + 1, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    prev = torch.zeros((nch, 2), dtype=torch.int64, device=dev)
    rxa, rxb = sc.Receiver(nch), sc.Receiver(nch)

    def records_two():
        convert()
        sc._check(L.qpsk_rx_batch_records_squelch_device(rxa._h, o, nf, min_sumsq, prev.data_ptr(), sc.REC_BY_CHANNEL,
                                                         cf, rec.data_ptr(), None, None, groups.data_ptr(),
                                                         count.data_ptr(), None, sp))

    def records_fmt():
        sc._check(L.qpsk_rx_batch_records_squelch_device_fmt(rxb._h, p, fmt, nch, nf, min_sumsq, prev.data_ptr(),
                                                             sc.REC_BY_CHANNEL, cf, rec.data_ptr(), None, None,
                                                             groups.data_ptr(), count.data_ptr(), None, sp))

    steps = rounds_of({"records_two": records_two, "records_fmt": records_fmt}, args.rounds, args.warmup, args.steps,
                      timed)
    rxa.sync()
    rxb.sync()
    rxa.close()
    rxb.close()
    legs = {k: {"ms_round_medians": v, "ms": statistics.median(v)} for k, v in {**passes, **steps}.items()}
    fused_wins = all(c < b for c, b in zip(passes["fused"], passes["convert_meter"]))
    res = {"format": name, "fmt": fmt, "source_bytes": src.numel() * src.element_size(), "work_bytes": need,
           "fused_equals_composition": same, "legs": legs,
           "meter_ms_in_composition": legs["convert_meter"]["ms"] - legs["convert"]["ms"],
           "meter_ms_in_fused": legs["fused"]["ms"] - legs["convert"]["ms"],
           "fused_below_composition_every_round": fused_wins,
           "records_fmt_minus_records_two_ms": legs["records_fmt"]["ms"] - legs["records_two"]["ms"]}
    del src, out, level, work, rec
    torch.cuda.empty_cache()
    return res


def stream_legs(args, sc, torch, x):
    """records per second of wall time through a plain and a squelch record stream"""
    import numpy as np
    nch, nf = args.channels, args.stream_frames
    fmt = sc.IN_ALAW | sc.IN_INTERLEAVED
    T = nf * sc.FRAME_SIZE
    src = torch.empty((T, nch), dtype=torch.uint8, device=x.device)
    sc.output_convert_device(x[:, :nf].reshape(nch, T), fmt, src)
    chunk = src.cpu().numpy()
    min_sumsq = sc.sumsq_of_dbfs(args.squelch_db)
    out = {}
    for name, kw in (("records", {}), ("records_squelch", {"min_sumsq": min_sumsq})):
        st = sc.Stream(nch, nf, nslot=3, fmt=fmt, records=True, order=sc.REC_BY_FRAME, **kw)
        rates = []
        for _ in range(args.rounds):
            n = recs = 0
            t0 = time.perf_counter()
            for k in range(args.stream_chunks + st.nslot):
                if st.pending == st.nslot or (k >= args.stream_chunks and st.pending):
                    recs += st.retrieve_records(copy=False)["count"]
                    n += 1
                if k < args.stream_chunks:
                    np.copyto(st.acquire_raw(), chunk)
                    st.submit()
            dt = time.perf_counter() - t0
            assert n == args.stream_chunks
            rates.append(n * nch * nf / dt)
        st.close()
        out[name] = {"channel_frames_per_s_rounds": rates, "channel_frames_per_s": statistics.median(rates),
                     "records_last_round": recs}
    out["squelch_over_plain"] = out["records_squelch"]["channel_frames_per_s"] / out["records"]["channel_frames_per_s"]
    return {"channels": nch, "frames_per_chunk": nf, "chunks": args.stream_chunks, "slots": 3, "format": "alaw_interleaved",
            "chunk_bytes": int(chunk.nbytes), "legs": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--stream-frames", type=int, default=4)
    ap.add_argument("--stream-chunks", type=int, default=12)
    ap.add_argument("--squelch-db", type=float, default=-60.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import singlecarrier_amd as sc
    x = sc.synth_device(args.seed, args.channels, args.frames, 1000.0)
    res = {"bench": "meter_fused", "device": torch.cuda.get_device_name(0), "kernel_hash": sc.kernel_hash(),
           "channels": args.channels, "frames": args.frames, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds, "squelch_dbfs": args.squelch_db, "formats": []}
    for fmt, name in ((sc.IN_ALAW | sc.IN_PLANAR, "alaw_planar"), (sc.IN_ALAW | sc.IN_INTERLEAVED, "alaw_interleaved"),
                      (sc.IN_S16 | sc.IN_INTERLEAVED, "s16_interleaved")):
        res["formats"].append(format_legs(args, sc, torch, x, fmt, name))
        print(json.dumps(res["formats"][-1]), file=sys.stderr, flush=True)
    res["streams"] = stream_legs(args, sc, torch, x)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
