"""bench.py on hardware (run with -m gpu): the N = 1 line and the N = 2
launcher.  On a one-GPU box both ranks share the GPU (`shared_gpus` in the
line; the time is not a scaling figure): what is checked is the contract the
driver reads -- rank 0's stdout is exactly one JSON line -- and per-rank
parity of the timed outputs against the oracle (a --full leg).  A plain run
(no --full) runs the timed steps only; --dump-outputs writes their outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--full", "--steps", "2", "--warmup", "1", "--channels", "4096", "--cpu-channels", "0",
         "--cpu-all-channels", "0", "--stream-chunks", "0", "--verify", "64"]


def _run(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_one_gpu_line():
    d = _run(SMALL)
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["verified_vs_oracle"] is True
    assert d["config"]["channels_total"] == 4096 and d["roofline"]["kernels_us"]["rx_kernel"] > 0


def test_bench_two_ranks_one_json_line():
    d = _run(["--gpus", "2", *SMALL])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong"
    assert d["config"]["channels_per_gpu"] == 2048 and d["config"]["channels_total"] == 4096
    assert [v["channels"][0] for v in d["verified_per_rank"]] == [0, 2048]
    assert d["verified_vs_oracle"] is True


def test_bench_plain_run_dumps_last_step(tmp_path):
    """No --full: only the timed steps run (every other leg's field is null),
    the line keeps its headline fields, and --dump-outputs writes the last
    step's bits and valid as float32 .npy next to the sampled channel ids."""
    d = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--channels", "4096", "--frames", "8",
              "--dump-outputs", str(tmp_path / "out")])
    assert d["full"] is False and d["steps"] == 3 and d["n_gpus"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "Msamples/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["metric"]
    # value and ms_per_step are the same measurement.  The line rounds both to
    # 3 decimals: ms_per_step is off by at most 0.0005 ms, and value's rounding
    # (0.0005 in ~2e5 Msamples/s) moves the quotient by < 1e-9 ms
    assert 4096 * 8 * 1880 / d["value"] / 1e3 == pytest.approx(d["ms_per_step"], abs=0.000501)
    for leg in ("verified_vs_oracle", "stream_pcie", "drop_in_frame_latency", "cpu_baseline",
                "cpu_baseline_all_cores", "h2d_s", "h2d_incl_msamples_s"):
        assert d[leg] is None, leg
    out = tmp_path / "out"
    assert sorted(os.listdir(out)) == ["bits.npy", "channels.npy", "valid.npy"]
    assert d["dumped_outputs"] == {"channels.npy": [4096], "bits.npy": [4096, 8, 62],
                                   "valid.npy": [4096, 8]}
    bits, valid, ch = (np.load(out / f"{n}.npy") for n in ("bits", "valid", "channels"))
    assert bits.dtype == np.float32 and valid.dtype == np.float32 and ch.dtype == np.float64
    assert bits.shape == (4096, 8, 62) and valid.shape == (4096, 8)
    assert (ch == np.arange(4096)).all()
    assert np.isin(bits, (0, 1)).all() and np.isin(valid, (0, 1)).all() and valid.sum() > 0
    # the noiseless synthetic batch: what the library returns for the same
    # stream (1 warmup + 3 timed batches of the same input), last batch
    import singlecarrier_amd as sc
    x = sc.synth(3, 64, 8)
    rx = sc.Receiver(64)
    ref = rx.demod(np.concatenate([x] * 4, axis=1))
    rx.close()
    assert (bits[:64] == ref["bits"][:, -8:]).all() and (valid[:64] == ref["valid"][:, -8:]).all()
