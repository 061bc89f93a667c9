#!/usr/bin/env python3
"""Batched transmitter against the lane-per-channel generator and the write
ceiling, in one process on one GPU.  Prints one JSON line (a copy is committed
as profiles/tx_bench.json and cited by DESIGN.md).

    python profiles/tx_bench.py [--channels 65536] [--packets 22] [--gap 903]
                                [--steps 20] [--warmup 3]

Three legs over the same output buffer int16 [channels][packets * (1880 + gap)],
alternated step by step after a warm-up of each:
  (a) qpsk_tx_batch_device (qpsk_tx.hip) on a fixed random payload;
  (b) qpsk_synth_device, noiseless, same channel count and nsamples
      (qpsk_synth_dev.hip: its own dibits, a memset pass plus lane = channel
      int16 stores) -- the GPU modulator the project had before;
  (c) hipMemsetAsync of the buffer: the practical ceiling of writing the bytes.
Each is timed two ways: HIP events around the enqueue (kernel time; for (a)
and (b) it includes the carrier table's upload), and a host clock around the
call plus a synchronise (call time; it includes the host's carrier table,
which (a) also reports on its own).  There is no CPU fallback: without a GPU
this fails.
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

# MI355X peaks the bounds are computed against (spec): HBM3E 8.0 TB/s; fp32
# vector 157.3 TFLOP/s counts an fma as 2, so fp32 instructions (an fma, an add
# or a multiply each count once) issue at half of it
PEAK_HBM_BPS = 8.0e12
PEAK_FP32_OPS = 157.3e12 / 2
# fp32 instructions per transmitted sample (qpsk_tx.hip period()): the tap fmas
# of both components (10 taps, 9 for the period's last sample), 2 gain
# multiplies, the carrier's 2 multiplies and subtract, the scale; making +-1.0
# from the sign bits is integer work
FP32_PER_TX_SAMPLE = 2 * (4 * 10 + 9) / 5 + 2 + 3 + 1


def hip_runtime():
    """The HIP runtime this process already has loaded (torch's)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--packets", type=int, default=22)
    ap.add_argument("--gap", type=int, default=903)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch

    import singlecarrier_amd as sc

    if not torch.cuda.is_available():
        raise SystemExit("tx_bench: no GPU")
    nch, npk, gap = args.channels, args.packets, args.gap
    ns = npk * (sc.TX_PACKET + gap)
    L = sc.lib()
    hip = hip_runtime()
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    dev = torch.device("cuda", 0)
    out = torch.empty((nch, ns), dtype=torch.int16, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    bits = torch.randint(0, 2, (nch, npk, 8, sc.NBITS), dtype=torch.uint8, device=dev, generator=g)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    tx = sc.Transmitter(nch, device=0, gap=gap)

    def leg_tx():
        tx.modulate_device(bits, out, stream)

    def leg_synth():
        sc._check(L.qpsk_synth_device(1, 0, nch, 1000.0, out.data_ptr(), ns, sp))

    def leg_memset():
        rc = hip.hipMemsetAsync(out.data_ptr(), 0, out.numel() * 2, sp)
        if rc != 0:
            raise RuntimeError(f"hipMemsetAsync: {rc}")

    legs = {"tx": leg_tx, "synth": leg_synth, "memset": leg_memset}
    ev_ms = {k: [] for k in legs}
    call_ms = {k: [] for k in legs}
    for step in range(args.warmup + args.steps):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if step >= args.warmup:
                ev_ms[name].append(e0.elapsed_time(e1))
                call_ms[name].append((t1 - t0) * 1e3)
    # the host's share of a transmitter call: the carrier table of npk packets
    tab = np.empty((npk * sc.TX_PACKET, 2), np.float32)
    table_ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        L.qpsk_tx_phase_table(tab.ctypes.data, npk * sc.TX_PACKET)
        table_ms.append((time.perf_counter() - t0) * 1e3)
    tx.close()

    samples = nch * ns
    med = {k: statistics.median(v) for k, v in ev_ms.items()}
    rel = {k: (max(v) - min(v)) / statistics.median(v) for k, v in ev_ms.items()}
    # counted traffic and arithmetic of (a), per output sample
    bytes_per_sample = 2.0 + sc.PACKET_BITS / (sc.TX_PACKET + gap)
    fp32_per_sample = FP32_PER_TX_SAMPLE * sc.TX_PACKET / (sc.TX_PACKET + gap)
    t_mem = samples * bytes_per_sample / PEAK_HBM_BPS * 1e3
    t_alu = samples * fp32_per_sample / PEAK_FP32_OPS * 1e3
    res = {
        "bench": "tx_batch", "device": torch.cuda.get_device_name(0),
        "channels": nch, "packets": npk, "gap": gap, "samples": samples,
        "output_bytes": samples * 2, "steps": args.steps, "warmup": args.warmup,
        "kernel_ms": {k: spread(v) for k, v in ev_ms.items()},
        "call_ms": {k: spread(v) for k, v in call_ms.items()},
        "host_carrier_table_ms": spread(table_ms),
        "tx_samples_per_s_kernel": samples / (med["tx"] * 1e-3),
        "synth_samples_per_s_kernel": samples / (med["synth"] * 1e-3),
        "tx_samples_per_s_call": samples / (statistics.median(call_ms["tx"]) * 1e-3),
        "synth_samples_per_s_call": samples / (statistics.median(call_ms["synth"]) * 1e-3),
        "tx_over_synth_kernel": med["synth"] / med["tx"],
        "share_of_write_ceiling": med["memset"] / med["tx"],
        "spread_rel": rel,
        "tx_faster_than_synth_by_more_than_spread":
            min(ev_ms["synth"]) > max(ev_ms["tx"]),
        "counted": {"bytes_per_sample": bytes_per_sample, "fp32_ops_per_sample": fp32_per_sample,
                    "memory_bound_ms": t_mem, "fp32_bound_ms": t_alu,
                    "nearer_bound": "memory" if t_mem >= t_alu else "fp32",
                    "share_of_nearer_bound": max(t_mem, t_alu) / med["tx"]},
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
