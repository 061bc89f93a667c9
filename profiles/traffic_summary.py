"""Writes profiles/traffic_summary.txt to stdout: what the committed seeds of
tests/traffic.py cover, observe and catch, made on the CPU from the model, the
oracle and the stand-ins of tests/test_traffic_model.py.

    python profiles/traffic_summary.py [log of pytest --durations=0 -m gpu tests/test_gpu_traffic.py]

With a log, its "slowest durations" section is appended (the GPU run's per-test
durations)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_traffic_model as T  # noqa: E402
import traffic  # noqa: E402


def caught_by(run):
    try:
        run()
    except AssertionError as e:
        msg = str(e)
        return msg.split(": ")[0].split(", ", 1)[1] if ", op " in msg else "end of script (snapshot bytes)"
    return None


def main():
    print("Random call traffic (tests/traffic.py): what the committed seeds cover, observe and catch.")
    print("Written by profiles/traffic_summary.py.\n")
    print(f"receive seeds {traffic.RX_SEEDS}, transmit seeds {traffic.TX_SEEDS}, exchange seed {traffic.EX_SEED}\n")
    scripts = {s: traffic.gen_rx(s) for s in traffic.RX_SEEDS}
    for s, ops in scripts.items():
        kinds = {}
        for o in ops:
            kinds[o[0]] = kinds.get(o[0], 0) + 1
        print(f"seed {s}: {len(ops)} ops, {sum(o[2] for o in ops if o[0] == 'rx')} frames, {kinds}")
    cover = T.coverage(scripts)
    print("\ncoverage counts (over the four scripts)")
    print(f"  ordered pairs of op kinds back to back on a channel: {sum(1 for k in cover if k[0] == 'pair')} of 36")
    for k in sorted((k for k in cover if k[0] != "pair"), key=str):
        print(f"  {k}: {cover[k]}")
    print("\nobserved ops per kind (a frame valid with matches < 128 on a channel of the op's range before its "
          "next start),\nand the rows of the plain record calls with F > 0 per (order, cap)")
    for mode, name in zip(T.MODES, T.MODE_IDS):
        tot, rows = {}, {}
        for s, ops in scripts.items():
            c, m = traffic.observe_script(ops, mode, s)
            for k, v in c.items():
                tot[k] = tot.get(k, 0) + v
            for call in m.calls:
                if call["form"][0] == "rec" and call["F"]:
                    rows[call["form"][1:]] = rows.get(call["form"][1:], 0) + len(call["rec"]["rec"])
        print(f"  {name}: {tot}\n      rec rows {rows}")
    print("\nthe exchange (32 channels, 14 slots), from the host twin and the oracle")
    for gap in (0, 903):
        _, st = traffic.exchange_expected(traffic.exchange_plan(traffic.EX_SEED, gap))
        print(f"  gap {gap}: {st}")
    print("\nplanted faults in the stand-in receiver: the scripts that catch them (seed: first failing op)")
    for f in T.FAULTS:
        hits = [(s, caught_by(lambda: traffic.run_rx(ops, T._make([f]), 0, s))) for s, ops in scripts.items()]
        print(f"  {f}\n      " + "; ".join(f"{s}: {h}" for s, h in hits if h))
    print("\nplanted faults in the stand-in transmitter")
    for f in T.TX_FAULTS:
        hits = [(s, caught_by(lambda: traffic.run_tx(traffic.gen_tx(s), lambda n, g: T.CpuTx(n, g, [f]), s)))
                for s in traffic.TX_SEEDS]
        print(f"  {f}\n      " + "; ".join(f"{s}: {h}" for s, h in hits if h))
    if len(sys.argv) > 1:
        log = open(sys.argv[1]).read()
        print("\nGPU run's per-test durations on one MI355X (pytest --durations=0 -m gpu tests/test_gpu_traffic.py)")
        for line in log[log.index("slowest durations"):].splitlines()[1:]:
            if line.strip():
                print("  " + line)


if __name__ == "__main__":
    main()
