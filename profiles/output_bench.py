#!/usr/bin/env python3
"""The output formats of the transmitter (include/qpsk_output.h) against the
plain int16 call and the copy ceiling, in one process on one GPU.  Prints one
JSON line and writes it to --out (a copy is committed as
profiles/output_bench.json and cited by README.md and DESIGN.md).

    python profiles/output_bench.py [--channels 65536] [--packets 22] [--gap 903] [--steps 5] [--warmup 2]
                                    [--rounds 3] [--host-packets 4] [--parent-lib PATH]
                                    [--out profiles/output_bench.json]

Device rounds: every leg is enqueued on one stream and timed with HIP events
around the enqueue; the legs are alternated step by step (odd steps in reverse
order, so a leg's predecessor alternates too), `rounds` rounds of
`steps` steps after `warmup` steps, and a round's figure is the median of its
steps.  Legs: the plain int16 call (qpsk_tx_batch_device); planar A-law by the
fused store of tx_batch_kernel and by modulator + pre-pass; interleaved A-law
and interleaved int16 (modulator + pre-pass); the pre-passes alone on an
int16 block whose rows are padded to 8 samples, as the format calls lay it out,
and two of them on dense rows; and a hipMemcpyAsync device-to-device of the int16 block, the
practical ceiling of moving its bytes once.  With --parent-lib (a
libqpsk_hip.so built from the commit before the output formats) the same int16
call of that library runs as one more leg in the same alternation, and then
alone against this library's in the order new, parent, parent, new: the A/B of
the templated kernel's int16 instantiation against the kernel it came from.  A
second copy of the parent's library then takes this library's place in the same
loop: what two loads of one and the same code differ by.

Host call: qpsk_tx_batch (int16, planar) against qpsk_tx_batch_fmt
(interleaved A-law) at channels x host-packets, by the host clock, alternated
over `rounds` rounds after one warm-up call each; the expectation is that the
time follows the bytes copied back (2 : 1).  There is no CPU fallback: without
a GPU this fails.
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

PATH_PREPASS, PATH_FUSED = 0, 1   # csrc/qpsk_fmt_internal.h


def hip_runtime():
    """The HIP runtime this process already has loaded (torch's)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


class ParentTx:
    """qpsk_tx_* of another build of the library, loaded beside this one"""

    def __init__(self, path, nch, gap):
        vp, i32 = C.c_void_p, C.c_int
        self.L = C.CDLL(path)
        self.L.qpsk_tx_create.restype = vp
        self.L.qpsk_tx_create.argtypes = [i32, i32, i32, C.POINTER(C.c_int)]
        self.L.qpsk_tx_destroy.restype = None
        self.L.qpsk_tx_destroy.argtypes = [vp]
        self.L.qpsk_tx_batch_device.argtypes = [vp, vp, i32, vp, C.c_long, vp]
        self.L.qpsk_tx_sync.argtypes = [vp]
        self.L.qpsk_kernel_hash.restype = C.c_char_p
        err = C.c_int(0)
        self.h = self.L.qpsk_tx_create(0, nch, gap, C.byref(err))
        if not self.h:
            raise RuntimeError(f"parent qpsk_tx_create: {err.value}")

    def close(self):
        self.L.qpsk_tx_destroy(self.h)


def device_rounds(args, sc, torch, hip, nch, npk):
    gap = args.gap
    N = npk * (sc.TX_PACKET + gap)
    n = nch * N
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    L = sc.lib()
    bits = torch.randint(0, 2, (nch, npk, 8, sc.NBITS), dtype=torch.uint8, device=dev)
    lin = torch.zeros((nch, N), dtype=torch.int16, device=dev)     # the plain call's block, the pre-passes' source
    lin2 = torch.empty((nch, N), dtype=torch.int16, device=dev)    # interleaved int16, the memcpy's destination
    codes = torch.empty(n, dtype=torch.uint8, device=dev)
    # the pre-passes' source as the format calls lay it out: rows padded to 8 samples, so 16-byte aligned
    Np = (N + 7) // 8 * 8
    linp = torch.zeros((nch, Np), dtype=torch.int16, device=dev)
    tx = sc.Transmitter(nch, gap=gap)
    parent = ParentTx(args.parent_lib, nch, gap) if args.parent_lib else None
    A, S, IL = sc.OUT_ALAW, sc.OUT_S16, sc.OUT_INTERLEAVED

    def plain():
        sc._check(L.qpsk_tx_batch_device(tx._h, bits.data_ptr(), npk, lin.data_ptr(), N, sp))

    def plain_parent():
        rc = parent.L.qpsk_tx_batch_device(parent.h, bits.data_ptr(), npk, lin.data_ptr(), N, sp)
        if rc != 0:
            raise RuntimeError(f"parent qpsk_tx_batch_device: {rc}")

    def fmt_call(fmt, dst, ld, path):
        def run():
            sc._check(L.qpsk_tx_batch_device_fmt_path(tx._h, bits.data_ptr(), npk, dst.data_ptr(), fmt, ld, sp, path))
        return run

    def prepass(fmt, dst, ld, src=None, src_ld=None):
        src, src_ld = (linp, Np) if src is None else (src, src_ld)

        def run():
            sc._check(L.qpsk_output_convert_device(fmt, src.data_ptr(), src_ld, nch, N, dst.data_ptr(), ld, sp))
        return run

    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    def memcpy():
        rc = hip.hipMemcpyAsync(lin2.data_ptr(), lin.data_ptr(), 2 * n, 3, sp)   # hipMemcpyDeviceToDevice
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync: {rc}")

    # (enqueue, bytes the leg writes to the caller's block)
    legs = {"s16_planar": (plain, 2 * n)}
    if parent:
        legs["s16_planar_parent"] = (plain_parent, 2 * n)
    legs.update({
        "alaw_planar_fused": (fmt_call(A, codes, N, PATH_FUSED), n),
        "alaw_planar_prepass": (fmt_call(A, codes, N, PATH_PREPASS), n),
        "alaw_interleaved": (fmt_call(A | IL, codes, nch, PATH_PREPASS), n),
        "s16_interleaved": (fmt_call(S | IL, lin2, nch, PATH_PREPASS), 2 * n),
        "prepass_alone_alaw_planar": (prepass(A, codes, N), n),
        "prepass_alone_alaw_interleaved": (prepass(A | IL, codes, nch), n),
        "prepass_alone_s16_interleaved": (prepass(S | IL, lin2, nch), 2 * n),
        # the same from dense rows (src_ld = N: for an odd N most rows are not 16-byte aligned)
        "prepass_alone_alaw_planar_dense_rows": (prepass(A, codes, N, lin, N), n),
        "prepass_alone_alaw_interleaved_dense_rows": (prepass(A | IL, codes, nch, lin, N), n),
        "memcpy_d2d": (memcpy, 2 * n),
    })
    sc._check(L.qpsk_tx_batch_device(tx._h, bits.data_ptr(), npk, linp.data_ptr(), Np, sp))   # samples to convert
    rounds = {k: [] for k in legs}
    steps_all = {k: [] for k in legs}
    for rnd in range(args.rounds):
        ms = {k: [] for k in legs}
        for step in range(args.warmup + args.steps):
            # odd steps run the legs in reverse, so a leg's predecessor alternates
            for name, (fn, _) in (list(legs.items())[::-1] if step & 1 else legs.items()):
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
    res = {}
    for name, (_, nbytes) in legs.items():
        med = statistics.median(rounds[name])
        res[name] = {"round_median_ms": rounds[name], "ms": spread(steps_all[name]), "block_bytes": nbytes,
                     "block_gb_per_s": nbytes / (med * 1e-3) / 1e9}
    out = {"channels": nch, "packets": npk, "gap": gap, "samples": n, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds, "legs": res,
           "fused_faster_than_prepass_in_every_round":
               all(f < p for f, p in zip(rounds["alaw_planar_fused"], rounds["alaw_planar_prepass"]))}
    if parent:
        def abba(fa, fb):
            """round medians of fa and fb alone in the loop, in the order a, b, b, a"""
            med = {"a": [], "b": []}
            for rnd in range(args.rounds):
                ms = {"a": [], "b": []}
                for step in range(args.warmup + 2 * args.steps):
                    for name in ("a", "b", "b", "a"):
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        (fa if name == "a" else fb)()
                        e1.record(stream)
                        torch.cuda.synchronize()
                        if step >= args.warmup:
                            ms[name].append(e0.elapsed_time(e1))
                for k in med:
                    med[k].append(statistics.median(ms[k]))
            return med

        def spread_of(xs):
            return (max(xs) - min(xs)) / statistics.median(xs)

        # the A/B proper: nothing but the two int16 calls, in the order new, parent, parent, new
        ab = abba(plain, plain_parent)
        out["s16_ab_parent"] = {"order": "new, parent, parent, new",
                                "round_median_ms": {"new": ab["a"], "parent": ab["b"]},
                                "new_over_parent": [a / b for a, b in zip(ab["a"], ab["b"])],
                                "parent_round_spread": spread_of(ab["b"]),
                                "parent_kernel_hash": parent.L.qpsk_kernel_hash().decode()}
        # the control: a second copy of the parent's library in the place of this one
        import shutil
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            twin_path = shutil.copy(args.parent_lib, os.path.join(tmp, "libqpsk_hip_twin.so"))
            twin = ParentTx(twin_path, nch, gap)

            def plain_twin():
                rc = twin.L.qpsk_tx_batch_device(twin.h, bits.data_ptr(), npk, lin.data_ptr(), N, sp)
                if rc != 0:
                    raise RuntimeError(f"parent twin qpsk_tx_batch_device: {rc}")

            aa = abba(plain_twin, plain_parent)
            twin.close()
        out["s16_aa_parent"] = {"order": "parent's copy, parent, parent, parent's copy",
                                "round_median_ms": {"copy": aa["a"], "parent": aa["b"]},
                                "copy_over_parent": [a / b for a, b in zip(aa["a"], aa["b"])],
                                "parent_round_spread": spread_of(aa["b"])}
        parent.close()
    tx.close()
    del bits, lin, lin2, linp, codes
    torch.cuda.empty_cache()
    return out


def host_call(args, sc, torch, nch, npk):
    import numpy as np
    gap = args.gap
    N = npk * (sc.TX_PACKET + gap)
    bits = np.random.default_rng(1).integers(0, 2, (nch, npk, 8, sc.NBITS), dtype=np.uint8)
    fmt = sc.OUT_ALAW | sc.OUT_INTERLEAVED
    lin = np.zeros((nch, N), np.int16)       # touched here, so no call pays for the pages
    trunk = np.zeros((N, nch), np.uint8)
    tx = sc.Transmitter(nch, gap=gap)
    L = sc.lib()

    def s16():
        sc._check(L.qpsk_tx_batch(tx._h, bits.ctypes.data, npk, lin.ctypes.data, N))

    def alaw():
        sc._check(L.qpsk_tx_batch_fmt(tx._h, bits.ctypes.data, npk, trunk.ctypes.data, fmt, nch))

    legs = {"s16_planar": s16, "alaw_interleaved": alaw}
    ms = {k: [] for k in legs}
    for fn in legs.values():
        fn()
    for _ in range(args.rounds):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    tx.close()
    return {"channels": nch, "packets": npk, "gap": gap, "rounds": args.rounds, "ms": ms,
            "bytes_copied_back": {"s16_planar": lin.nbytes, "alaw_interleaved": trunk.nbytes},
            "s16_over_alaw": [a / b for a, b in zip(ms["s16_planar"], ms["alaw_interleaved"])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--packets", type=int, default=22)
    ap.add_argument("--gap", type=int, default=903)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-packets", type=int, default=4)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "output_bench.json"))
    args = ap.parse_args()

    import torch

    import singlecarrier_amd as sc

    if not torch.cuda.is_available():
        raise SystemExit("output_bench: no GPU")
    hip = hip_runtime()
    res = {"bench": "output_formats", "device": torch.cuda.get_device_name(0), "kernel_hash": sc.kernel_hash(),
           "device_rounds": device_rounds(args, sc, torch, hip, args.channels, args.packets),
           "device_rounds_host_size": device_rounds(args, sc, torch, hip, args.channels, args.host_packets),
           "host_call": host_call(args, sc, torch, args.channels, args.host_packets)}
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
