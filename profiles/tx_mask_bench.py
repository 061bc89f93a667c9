#!/usr/bin/env python3
"""What a per-channel packet index costs the transmitter, on one GPU.  Prints
one JSON line (a copy is committed as profiles/tx_mask_bench.json and cited by
DESIGN.md "Transmit channels that come and go").

    python profiles/tx_mask_bench.py --parent-lib PATH [--variant-lib PATH2] [--channels 65536]
                                     [--packets 22] [--gap 903] [--steps 16] [--warmup 3] [--rounds 3]

PATH is libqpsk_hip.so of the parent commit, built beside this one.  Four cases
over one int16 block [channels][packets * (1880 + gap)], HIP events around each
call (for a uniform context that includes the carrier table's upload and
tx_state_kernel, for a general one tx_plan_kernel), `rounds` rounds of medians:
  (a) the plain call on a uniform context: tx_batch_kernel, as before.  Its A/B
      against the parent's library is output_bench.py's: the two alone in the
      loop in the order new, parent, parent, new, and as a control a second copy
      of the parent's library in this library's place;
  (b) the plain call on a general context whose channels share one index: what
      tx_plan_kernel and tx_mask_kernel cost with nothing to gain from them;
  (c) a masked call, a random half of the slots idle;
  (d) the plain call on a general context whose every 16th channel is 3 packets
      behind: both carrier signs inside the 16-channel loops of class 0.
(a) .. (d) alternate step by step (odd steps in reverse order) and (b), (c), (d)
are reported per round as ratios to (a).  With --variant-lib, another build of
this library (for the record in DESIGN.md: tx_mask_kernel with a block-uniform
branch that keeps the carrier in registers where a block's channels agree on
it, which was measured and left out) runs (b), (c) and (d) on contexts of its
own as further legs of the same alternation, `variant_*`, so the two builds are
compared on one box in one loop.  The general kernel's registers come
from the compiler's resource remarks for qpsk_tx.hip (no GPU needed for those).
"""
import argparse
import ctypes as C
import json
import os
import re
import shlex
import shutil
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from output_bench import ParentTx, spread   # noqa: E402


def kernel_resources():
    """{kernel: {vgprs, sgprs, scratch, lds, occupancy}} of qpsk_tx.hip's kernels"""
    csrc = os.path.join(ROOT, "singlecarrier_amd", "csrc")
    cmd = shlex.split(subprocess.run(["make", "-s", "--no-print-directory", "-C", csrc, "kcmd"], check=True,
                                     capture_output=True, text=True).stdout)
    with tempfile.TemporaryDirectory() as tmp:
        err = subprocess.run(cmd + ["-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-c",
                                    "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(tmp, "tx.co"),
                                    os.path.join(csrc, "qpsk_tx.hip")], check=True, capture_output=True, text=True).stderr
    names = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
             "LDS Size [bytes/block]": "lds_bytes", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd"}
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: \s*([^:]+): (\S+) \[-Rpass", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip()
                                 .replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0], {})
        elif cur is not None and m.group(1) in names:
            cur[names[m.group(1)]] = int(m.group(2))
    return out


class VariantTx:
    """a general context of another build of this library"""

    def __init__(self, L, nch, gap):
        vp, i32 = C.c_void_p, C.c_int
        L.qpsk_tx_create.restype = vp
        L.qpsk_tx_create.argtypes = [i32, i32, i32, C.POINTER(C.c_int)]
        L.qpsk_tx_destroy.restype = None
        L.qpsk_tx_destroy.argtypes = [vp]
        L.qpsk_tx_reset_channels.argtypes = [vp, i32, i32]
        L.qpsk_tx_state_load.argtypes = [vp, i32, i32, vp, C.c_size_t]
        L.qpsk_tx_batch_masked_device.argtypes = [vp, vp, vp, i32, vp, C.c_long, vp]
        self.L = L
        err = C.c_int(0)
        self._h = L.qpsk_tx_create(0, nch, gap, C.byref(err))
        if not self._h:
            raise RuntimeError(f"variant qpsk_tx_create: {err.value}")

    def reset_channels(self, c0, n):
        if self.L.qpsk_tx_reset_channels(self._h, c0, n) != 0:
            raise RuntimeError("variant qpsk_tx_reset_channels")

    def state_load(self, snap):
        n = int.from_bytes(snap[8:12], "little")
        if self.L.qpsk_tx_state_load(self._h, 0, n, snap, len(snap)) != 0:
            raise RuntimeError("variant qpsk_tx_state_load")

    def close(self):
        self.L.qpsk_tx_destroy(self._h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--variant-lib", default=None)
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--packets", type=int, default=22)
    ap.add_argument("--gap", type=int, default=903)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch

    import singlecarrier_amd as sc

    if not torch.cuda.is_available():
        raise SystemExit("tx_mask_bench: no GPU")
    nch, npk, gap = args.channels, args.packets, args.gap
    N = npk * (sc.TX_PACKET + gap)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    L = sc.lib()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    bits = torch.randint(0, 2, (nch, npk, 8, sc.NBITS), dtype=torch.uint8, device=dev, generator=g)
    half = (torch.rand((nch, npk), device=dev, generator=g) < 0.5).to(torch.uint8)
    out = torch.zeros((nch, N), dtype=torch.int16, device=dev)

    uniform = sc.Transmitter(nch, gap=gap)
    equal = sc.Transmitter(nch, gap=gap)
    equal.reset_channels(0, 1)                     # general, every channel at index 0
    idle = sc.Transmitter(nch, gap=gap)            # general from its first masked call
    behind = sc.Transmitter(nch, gap=gap)
    idx = np.full(nch, 1003, np.uint64)
    idx[::16] = 1000
    behind_snap = (np.array([0x53585451, 1, nch, 0], "<u4").tobytes() + idx.tobytes() +
                   np.zeros(nch, "<u4").tobytes())
    behind.state_load(behind_snap)
    parent = ParentTx(args.parent_lib, nch, gap)

    def call(tx, mask=None, lib=L):
        def run():
            sc._check(lib.qpsk_tx_batch_masked_device(tx._h, bits.data_ptr(), None if mask is None else mask.data_ptr(),
                                                      npk, out.data_ptr(), N, sp))
        return run

    def parent_call(p):
        def run():
            rc = p.L.qpsk_tx_batch_device(p.h, bits.data_ptr(), npk, out.data_ptr(), N, sp)
            if rc != 0:
                raise RuntimeError(f"parent qpsk_tx_batch_device: {rc}")
        return run

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    legs = {"a_uniform_plain": call(uniform), "b_general_equal_indices": call(equal),
            "c_general_half_idle": call(idle, half), "d_general_every_16th_3_behind": call(behind)}
    variants = []
    if args.variant_lib:
        V = C.CDLL(args.variant_lib)
        v_equal, v_idle, v_behind = (VariantTx(V, nch, gap) for _ in range(3))
        v_equal.reset_channels(0, 1)
        v_behind.state_load(behind_snap)
        variants = [v_equal, v_idle, v_behind]
        legs.update({"variant_b_general_equal_indices": call(v_equal, None, V),
                     "variant_c_general_half_idle": call(v_idle, half, V),
                     "variant_d_general_every_16th_3_behind": call(v_behind, None, V)})
    rounds = {k: [] for k in legs}
    steps_all = {k: [] for k in legs}
    for rnd in range(args.rounds):
        ms = {k: [] for k in legs}
        for step in range(args.warmup + args.steps):
            for name in (list(legs)[::-1] if step & 1 else list(legs)):
                t = timed(legs[name])
                if step >= args.warmup:
                    ms[name].append(t)
        for k in legs:
            rounds[k].append(statistics.median(ms[k]))
            steps_all[k] += ms[k]

    def abba(fa, fb):
        """round medians of fa and fb alone in the loop, in the order a, b, b, a"""
        med = {"a": [], "b": []}
        for rnd in range(args.rounds):
            ms = {"a": [], "b": []}
            for step in range(args.warmup + 2 * args.steps):
                for name in ("a", "b", "b", "a"):
                    t = timed(fa if name == "a" else fb)
                    if step >= args.warmup:
                        ms[name].append(t)
            for k in med:
                med[k].append(statistics.median(ms[k]))
        return med

    def spread_of(xs):
        return (max(xs) - min(xs)) / statistics.median(xs)

    ab = abba(call(uniform), parent_call(parent))
    with tempfile.TemporaryDirectory() as tmp:
        twin = ParentTx(shutil.copy(args.parent_lib, os.path.join(tmp, "libqpsk_hip_twin.so")), nch, gap)
        aa = abba(parent_call(twin), parent_call(parent))
        twin.close()
    # the general contexts really were general, the uniform one uniform: their indices
    checks = {"equal_indices": sorted(set(equal.channel_packets().tolist())),
              "behind_indices": sorted(set(behind.channel_packets().tolist())),
              "idle_active_share": float(half.float().mean())}
    for tx in [uniform, equal, idle, behind] + variants:
        tx.close()
    parent.close()

    a = rounds["a_uniform_plain"]
    res = {
        "bench": "tx_mask", "device": torch.cuda.get_device_name(0), "channels": nch, "packets": npk, "gap": gap,
        "samples": nch * N, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
        "legs": {k: {"round_median_ms": rounds[k], "ms": spread(steps_all[k])} for k in legs},
        "ratio_to_a": {k: [x / y for x, y in zip(rounds[k], a)] for k in legs if k != "a_uniform_plain"},
        "a_against_parent": {"order": "new, parent, parent, new",
                             "round_median_ms": {"new": ab["a"], "parent": ab["b"]},
                             "new_over_parent": [x / y for x, y in zip(ab["a"], ab["b"])],
                             "parent_round_spread": spread_of(ab["b"])},
        "control_parent_twice": {"order": "parent's copy, parent, parent, parent's copy",
                                 "round_median_ms": {"copy": aa["a"], "parent": aa["b"]},
                                 "copy_over_parent": [x / y for x, y in zip(aa["a"], aa["b"])],
                                 "parent_round_spread": spread_of(aa["b"])},
        "checks": checks,
        "kernel_resources": kernel_resources(),
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
