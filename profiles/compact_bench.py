#!/usr/bin/env python3
"""The record layer of the receive output (include/qpsk_compact.h) in one
process on one GPU.  Prints one JSON line and writes it to --out (a copy is
committed as profiles/compact_bench.json and cited by README.md and DESIGN.md).

    python profiles/compact_bench.py [--channels 65536] [--frames 32] [--ebn0 1000] [--steps 5] [--warmup 2]
                                     [--rounds 3] [--host-frames 4] [--stream-chunks 12]
                                     [--out profiles/compact_bench.json]

Pass time alone: the dense outputs of one receive of qpsk_synth_device input
stay on the device; every leg is enqueued on one stream and timed with HIP
events around the enqueue, the legs alternated step by step (odd steps in
reverse order), `rounds` rounds of `steps` steps after `warmup` steps, a
round's figure the median of its steps.  Legs: qpsk_compact_device by channel
and by frame, each with and without the soft and trace rows; a pure count;
qpsk_bits_pack_device; a hipMemcpyAsync device-to-device of the dense bits +
valid; and the receive step itself (qpsk_rx_batch_device).

Host call: qpsk_rx_batch against qpsk_rx_batch_records at channels x
host-frames by the host clock, alternated over `rounds` rounds after one
warm-up call each, with the bytes each copies back.

Stream: the plain stream against the record stream, both from planar int16, in
samples per second as bench.py measures its stream (3 slots, the pinned slots
filled once), alternated over `rounds` rounds.  The committed JSON holds one
more stream leg, records_direct_store: the same with the scatter storing the
records straight into the slot's pinned block, measured once with a build that
had that path; it tied with the copy after the count and was not kept
(DESIGN.md).  There is no CPU fallback: without a GPU this fails.
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


def pass_alone(args, sc, torch, hip, nch, nf):
    import numpy as np
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    L = sc.lib()
    n = nch * nf
    x = sc.synth_device(args.seed, nch, nf, args.ebn0)
    bits = torch.zeros((nch, nf, sc.NBITS), dtype=torch.uint8, device=dev)
    valid = torch.zeros((nch, nf), dtype=torch.uint8, device=dev)
    trace = torch.zeros((nch, nf, 4), dtype=torch.int32, device=dev)
    soft = torch.zeros((nch, nf, sc.DATA_SYMBOLS, 2), dtype=torch.float32, device=dev)
    rx = sc.Receiver(nch)
    rx.demod_device(x, bits, valid, trace, soft)
    rx.sync()
    count = int(valid.sum())
    rec = torch.empty((n, 2), dtype=torch.int64, device=dev)
    rtr = torch.empty((count + 1, 4), dtype=torch.int32, device=dev)
    rso = torch.empty((count + 1, sc.DATA_SYMBOLS, 2), dtype=torch.float32, device=dev)
    groups = torch.empty(max(nch, nf) + 1, dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    work = torch.empty(sc.compact_work_bytes(nch, nf), dtype=torch.uint8, device=dev)
    words = torch.empty(n, dtype=torch.int64, device=dev)
    copy = torch.empty(n * (sc.NBITS + 1), dtype=torch.uint8, device=dev)
    bits2, valid2 = torch.empty_like(bits), torch.empty_like(valid)

    def compact(order, rows, cap):
        def run():
            sc._check(L.qpsk_compact_device(bits.data_ptr(), valid.data_ptr(), trace.data_ptr() if rows else None,
                                            soft.data_ptr() if rows else None, nch, nf, order, cap,
                                            rec.data_ptr() if cap else None, rtr.data_ptr() if rows else None,
                                            rso.data_ptr() if rows else None, groups.data_ptr(), cnt.data_ptr(),
                                            work.data_ptr(), work.numel(), sp))
        return run

    def pack():
        sc._check(L.qpsk_bits_pack_device(bits.data_ptr(), n, words.data_ptr(), sp))

    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    def memcpy():
        for dst, src, nb in ((copy.data_ptr(), bits.data_ptr(), n * sc.NBITS),
                             (copy.data_ptr() + n * sc.NBITS, valid.data_ptr(), n)):
            rc = hip.hipMemcpyAsync(dst, src, nb, 3, sp)   # hipMemcpyDeviceToDevice
            if rc != 0:
                raise RuntimeError(f"hipMemcpyAsync: {rc}")

    def receive():
        sc._check(L.qpsk_rx_batch_device(rx._h, x.data_ptr(), nf, bits2.data_ptr(), valid2.data_ptr(), None, None, sp))

    BC, BF = sc.REC_BY_CHANNEL, sc.REC_BY_FRAME
    # with rows, cap is the count: rec_soft of every channel-frame would be the dense array again
    legs = {"by_channel": compact(BC, False, n), "by_frame": compact(BF, False, n),
            "by_channel_soft_trace": compact(BC, True, count), "by_frame_soft_trace": compact(BF, True, count),
            "count_only_by_channel": compact(BC, False, 0), "pack_dense": pack, "memcpy_d2d_bits_valid": memcpy,
            "receive_step": receive}
    rounds = {k: [] for k in legs}
    steps_all = {k: [] for k in legs}
    for rnd in range(args.rounds):
        ms = {k: [] for k in legs}
        for step in range(args.warmup + args.steps):
            for name, fn in (list(legs.items())[::-1] if step & 1 else legs.items()):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                torch.cuda.synchronize()
                if step >= args.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        for k in legs:
            rounds[k].append(statistics.median(ms[k]))
            steps_all[k] += ms[k]
    rx.sync()
    got = int(cnt.cpu().numpy().view(np.uint32)[0])
    rx.close()
    res = {name: {"round_median_ms": rounds[name], "ms": spread(steps_all[name])} for name in legs}
    return {"channels": nch, "frames": nf, "ebn0_db": args.ebn0, "channel_frames": n, "valid_frames": count,
            "valid_share": count / n, "count_reported": got, "dense_bytes_bits_valid": n * (sc.NBITS + 1),
            "record_bytes": 16 * count, "soft_row_bytes": 248 * count, "steps": args.steps, "warmup": args.warmup,
            "rounds": args.rounds, "legs": res}


def host_call(args, sc, torch, nch, nf):
    import numpy as np
    x = sc.synth_device(args.seed, nch, nf, args.ebn0).cpu().numpy()
    n = nch * nf
    bits = np.zeros((nch, nf, sc.NBITS), np.uint8)     # touched here, so no call pays for the pages
    valid = np.zeros((nch, nf), np.uint8)
    rec = np.zeros(n, sc.REC_DTYPE)
    groups = np.zeros(nf + 1, np.uint32)
    count = C.c_uint32(0)
    rx = sc.Receiver(nch)
    L = sc.lib()

    def dense():
        sc._check(L.qpsk_rx_batch(rx._h, x.ctypes.data, nf, bits.ctypes.data, valid.ctypes.data, None, None))

    def records():
        sc._check(L.qpsk_rx_batch_records(rx._h, x.ctypes.data, nf, sc.REC_BY_FRAME, n, rec.ctypes.data, None, None,
                                          groups.ctypes.data, C.addressof(count)))

    legs = {"qpsk_rx_batch": dense, "qpsk_rx_batch_records": records}
    ms = {k: [] for k in legs}
    for fn in legs.values():
        fn()
    for _ in range(args.rounds):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    rx.close()
    return {"channels": nch, "frames": nf, "rounds": args.rounds, "ms": ms, "valid_frames_last_call": int(count.value),
            "bytes_copied_back": {"qpsk_rx_batch": bits.nbytes + valid.nbytes,
                                  "qpsk_rx_batch_records": 4 + groups.nbytes + 16 * int(count.value)},
            "input_bytes": x.nbytes,
            "dense_over_records": [a / b for a, b in zip(ms["qpsk_rx_batch"], ms["qpsk_rx_batch_records"])]}


def stream_legs(args, sc, torch, nch, fpc):
    x = sc.synth_device(args.seed, nch, fpc, args.ebn0).cpu().numpy()

    def run(records):
        st = sc.Stream(nch, fpc, nslot=3, records=records, order=sc.REC_BY_FRAME)
        take = (lambda: st.retrieve_records(copy=False)) if records else (lambda: st.retrieve(copy=False))
        for _ in range(3):   # untimed: fill every slot's pinned buffer once
            st.acquire()[...] = x
            st.submit()
        while st.pending:
            take()
        t = time.perf_counter()
        for _ in range(args.stream_chunks):
            if st.pending == 3:
                take()
            st.acquire()
            st.submit()
        while st.pending:
            last = take()
        dt = time.perf_counter() - t
        st.close()
        return nch * fpc * sc.FRAME_SIZE * args.stream_chunks / dt / 1e9, (last["count"] if records else None)

    legs = {"plain": lambda: run(False), "records_copy_after_count": lambda: run(True)}
    gs = {k: [] for k in legs}
    counts = {}
    for rnd in range(args.rounds):
        for name, fn in (list(legs.items())[::-1] if rnd & 1 else legs.items()):
            g, c = fn()
            gs[name].append(g)
            counts[name] = c
    plain = gs["plain"]
    return {"chunk": f"{nch} channels x {fpc} frames", "chunks": args.stream_chunks, "slots": 3, "rounds": args.rounds,
            "gsamples_s": gs, "valid_frames_last_chunk": counts,
            "plain_round_spread": (max(plain) - min(plain)) / statistics.median(plain),
            "median_over_plain": {k: statistics.median(v) / statistics.median(plain) for k, v in gs.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--ebn0", type=float, default=1000.0, help="bench.py's default: noiseless")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--stream-chunks", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_bench.json"))
    args = ap.parse_args()

    import torch

    import singlecarrier_amd as sc

    if not torch.cuda.is_available():
        raise SystemExit("compact_bench: no GPU")
    hip = hip_runtime()
    res = {"bench": "compact_records", "device": torch.cuda.get_device_name(0), "kernel_hash": sc.kernel_hash(),
           "tiling": sc.compact_tiling(),
           "pass_alone": pass_alone(args, sc, torch, hip, args.channels, args.frames),
           "host_call": host_call(args, sc, torch, args.channels, args.host_frames),
           "stream": stream_legs(args, sc, torch, args.channels, args.host_frames)}
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
