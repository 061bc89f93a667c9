#!/usr/bin/env python3
"""The level meter and the squelch (include/qpsk_level.h) against the copy
ceiling and against the receive step they follow, in one process on one GPU.
Prints one JSON line and writes it to --out (a copy is committed as
profiles/level_bench.json and cited by README.md and DESIGN.md).

    python profiles/level_bench.py [--channels 65536] [--frames 32] [--steps 7] [--warmup 2] [--rounds 3]
                                   [--host-frames 4] [--host-steps 3] [--squelch-db -60]
                                   [--out profiles/level_bench.json]

Device legs, on the benchmark's input (synth_device(seed 3), noiseless)
resident in HBM, timed with HIP events around the enqueue and alternated step
by step after a warm-up; `rounds` rounds, the median of each:
  meter            qpsk_level_device over the whole input
  squelch          qpsk_squelch_device on the dense outputs of a receive of it
                   (flags to a second array, bits rows zeroed, last written)
  memcpy_d2d       hipMemcpyAsync device to device of the same input: the
                   practical ceiling of reading its bytes once (and writing them)
  records          qpsk_rx_batch_records_device: the receive step as it is
  records_squelch  qpsk_rx_batch_records_squelch_device: the same with the
                   meter and the squelch between receive and compaction
GB/s counts the bytes read plus the bytes written.

Host legs: qpsk_rx_batch_records and qpsk_rx_batch_records_squelch on channels
x host-frames from pageable host memory, every second channel idle (zeros), by
the host clock; with the record counts and the bytes copied back.
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


def hip_runtime():
    """The HIP runtime this process already has loaded (torch's)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


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


def device_legs(args, sc, torch, hip):
    nch, nf = args.channels, args.frames
    cf = nch * nf
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    L = sc.lib()
    x = sc.synth_device(args.seed, nch, nf, 1000.0)
    in_bytes = x.numel() * 2
    min_sumsq = sc.sumsq_of_dbfs(args.squelch_db)
    # the dense outputs the squelch leg works on, from a receive of x
    rx = sc.Receiver(nch)
    bits = torch.empty((nch, nf, sc.NBITS), dtype=torch.uint8, device=dev)
    valid = torch.empty((nch, nf), dtype=torch.uint8, device=dev)
    rx.demod_device(x, bits, valid)
    rx.sync()
    rx.close()
    level = sc.level_device(x)
    vout = torch.empty_like(valid)
    last = torch.empty((nch, 2), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    nvalid = int((valid != 0).sum())
    s = sc.squelch_device(level, valid, min_sumsq, valid_out=vout, last=last)
    torch.cuda.synchronize()
    nkept = int((s["valid"] != 0).sum())
    silent = int((sc.level_from_tensor(level)["sumsq"] == 0).sum())
    copy = torch.empty_like(x)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    def meter():
        sc._check(L.qpsk_level_device(x.data_ptr(), cf, level.data_ptr(), sp))

    def squelch():
        sc._check(L.qpsk_squelch_device(level.data_ptr(), None, nch, nf, min_sumsq, valid.data_ptr(), vout.data_ptr(),
                                        bits.data_ptr(), None, last.data_ptr(), sp))

    def memcpy():
        rc = hip.hipMemcpyAsync(copy.data_ptr(), x.data_ptr(), in_bytes, 3, sp)   # hipMemcpyDeviceToDevice
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync: {rc}")

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    passes = rounds_of({"meter": meter, "squelch": squelch, "memcpy_d2d": memcpy}, args.rounds, args.warmup,
                       args.steps, timed)
    del copy
    torch.cuda.empty_cache()

    # the receive step with and without the two passes: a context each, the same outputs
    rec = torch.empty((cf, 2), dtype=torch.int64, device=dev)
    groups = torch.empty(nch + 1, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    prev = torch.zeros((nch, 2), dtype=torch.int64, device=dev)
    rxa, rxb = sc.Receiver(nch), sc.Receiver(nch)

    def records():
        sc._check(L.qpsk_rx_batch_records_device(rxa._h, x.data_ptr(), nf, sc.REC_BY_CHANNEL, cf, rec.data_ptr(), None,
                                                 None, groups.data_ptr(), count.data_ptr(), sp))

    def records_squelch():
        sc._check(L.qpsk_rx_batch_records_squelch_device(rxb._h, x.data_ptr(), nf, min_sumsq, prev.data_ptr(),
                                                         sc.REC_BY_CHANNEL, cf, rec.data_ptr(), None, None,
                                                         groups.data_ptr(), count.data_ptr(), None, sp))

    steps = rounds_of({"records": records, "records_squelch": records_squelch}, args.rounds, args.warmup, args.steps,
                      timed)
    rxa.sync()
    rxb.sync()
    rxa.close()
    rxb.close()

    moved = {"meter": in_bytes + 16 * cf, "squelch": 16 * cf + 2 * cf + sc.NBITS * (nvalid - nkept) + 16 * nch,
             "memcpy_d2d": 2 * in_bytes}
    legs = {}
    for k, v in {**passes, **steps}.items():
        med = statistics.median(v)
        legs[k] = {"ms_round_medians": v, "ms": med}
        if k in moved:
            legs[k]["bytes_moved"] = moved[k]
            legs[k]["gb_per_s"] = moved[k] / (med * 1e-3) / 1e9
    m = {k: legs[k]["ms"] for k in legs}
    return {"channels": nch, "frames": nf, "input_bytes": in_bytes, "level_bytes": 16 * cf, "steps": args.steps,
            "warmup": args.warmup, "rounds": args.rounds, "squelch_dbfs": args.squelch_db, "min_sumsq": min_sumsq,
            "valid_frames": nvalid, "valid_after_squelch": nkept, "frames_without_energy": silent, "legs": legs,
            "meter_ms_over_memcpy_ms": m["meter"] / m["memcpy_d2d"],
            "meter_gb_per_s_read": in_bytes / (m["meter"] * 1e-3) / 1e9,
            "meter_share_of_receive_step": m["meter"] / m["records"],
            "squelch_share_of_receive_step": m["squelch"] / m["records"],
            "records_squelch_over_records": m["records_squelch"] / m["records"]}


def host_legs(args, sc, torch):
    import numpy as np
    nch, nf = args.channels, args.host_frames
    cf = nch * nf
    x = sc.synth_device(args.seed, nch, nf, 1000.0).cpu().numpy()
    x[1::2] = 0   # every second channel idle
    min_sumsq = sc.sumsq_of_dbfs(args.squelch_db)
    L = sc.lib()
    rec = np.zeros(cf, sc.REC_DTYPE)
    groups = np.zeros(nch + 1, np.uint32)
    count = C.c_uint32(0)
    prev = np.zeros(nch, sc.LEVEL_DTYPE)
    rxa, rxb = sc.Receiver(nch), sc.Receiver(nch)
    counts = {}

    def records():
        sc._check(L.qpsk_rx_batch_records(rxa._h, x.ctypes.data, nf, sc.REC_BY_CHANNEL, cf, rec.ctypes.data, None, None,
                                          groups.ctypes.data, C.addressof(count)))
        counts["records"] = int(count.value)

    def records_squelch():
        prev[...] = 0   # every call is the start of the same stream
        rxb.reset()
        sc._check(L.qpsk_rx_batch_records_squelch(rxb._h, x.ctypes.data, nf, min_sumsq, prev.ctypes.data,
                                                  sc.REC_BY_CHANNEL, cf, rec.ctypes.data, None, None,
                                                  groups.ctypes.data, C.addressof(count), None))
        counts["records_squelch"] = int(count.value)

    def records_fresh():
        rxa.reset()
        records()

    def timed(fn):
        t0 = time.perf_counter()
        fn()   # ends in the call's own synchronisation
        return (time.perf_counter() - t0) * 1e3

    res = rounds_of({"records": records_fresh, "records_squelch": records_squelch}, args.rounds, 1, args.host_steps,
                    timed)
    rxa.close()
    rxb.close()
    head = 4 * (nch + 2)
    out = {"channels": nch, "frames": nf, "idle_channels": nch // 2, "input_bytes": x.nbytes, "steps": args.host_steps,
           "squelch_dbfs": args.squelch_db, "legs": {}}
    for k, v in res.items():
        back = head + 16 * counts[k] + (16 * nch if k == "records_squelch" else 0)
        out["legs"][k] = {"ms_round_medians": v, "ms": statistics.median(v), "records": counts[k],
                          "bytes_copied_back": back}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--squelch-db", type=float, default=-60.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_bench.json"))
    args = ap.parse_args()

    import torch

    import singlecarrier_amd as sc

    if not torch.cuda.is_available():
        raise SystemExit("level_bench: no GPU")
    hip = hip_runtime()
    res = {"bench": "level_squelch", "device": torch.cuda.get_device_name(0), "kernel_hash": sc.kernel_hash(),
           "device_calls": device_legs(args, sc, torch, hip), "host_calls": host_legs(args, sc, torch)}
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
