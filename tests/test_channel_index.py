"""What the per-channel frame index (qpsk_rx_reset_channels, qpsk_rx_state_join)
rests on, checked on the CPU.

A channel that starts on its own keeps the context's mixer sign and state
parity and gets only its descrambler word moved.  That is right
if, and only if,

  A. the receiver's outputs do not change when every input sample is negated
     (a channel whose own index differs from the context's by an odd number
     sees every mixed sample negated): pinned here on the unmodified reference
     (where oracle/_ref is built) and on the restatement, in every mode;
  B. a receiver started at frame index g instead of 0 differs in nothing but
     the keystream words: pinned on the restatement's qc_rx_frame;
  C. the index arithmetic of csrc/qpsk_rx_plan.h is right for any two 64-bit
     indices: a stand-alone program under ASan + UBSan
     (tests/sanitize/rx_index_check.cc), as tests/test_rx_plan.py does.

CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hostile
import oracle
import rxcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "singlecarrier_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
KS_FRAMES = 1057
CPU_MODES = (oracle.MODE_REF, oracle.MODE_DEC752, oracle.MODE_FFT_HUNT, oracle.MODE_DEC752 | oracle.MODE_FFT_HUNT)
TRACE_FIELDS = ("max_index", "matches", "valid", "rx_timing")


# ------------------------------------------------------------ A. symmetry pin
def _inputs(name):
    """int16 [nch][nframes][1880] with -32768 clamped to -32767, so that -x is
    an int16 stream too (the feature itself never negates an integer)."""
    if name == "clean":
        x = oracle.synth(11, 24, 12, 1000.0)
    elif name == "eb4":
        x = oracle.synth(12, 24, 12, 4.0)
    else:
        x = hostile.group(name)
    return np.maximum(x, -32767).astype(np.int16)


def _assert_symmetric(rx, name):
    x = _inputs(name)
    bits, valid, tr = rx(x)
    nbits, nvalid, ntr = rx(-x)
    assert valid.sum() > 0, "no valid frame: the case shows nothing"
    nans = int(np.isnan(tr["soft"]).sum())
    print(f"{name}: {int(valid.sum())} valid frames of {valid.size}, {nans} NaN soft values")
    if name == "wave":
        assert nans > 0, "the wave group no longer reaches NaN soft symbols"
    np.testing.assert_array_equal(nvalid, valid)
    np.testing.assert_array_equal(nbits, bits)
    for f in TRACE_FIELDS:
        np.testing.assert_array_equal(ntr[f], tr[f], err_msg=f)
    assert not rxcheck.same_soft(ntr["soft"], tr["soft"]).any()


@pytest.mark.parametrize("name", ["clean", "eb4", "wave", "impaired"])
@pytest.mark.parametrize("mode", CPU_MODES)
def test_restatement_is_even_in_its_input(mode, name):
    """cpu_rx(x) == cpu_rx(-x): trace, bits and soft symbols (NaN as a class)."""
    _assert_symmetric(lambda x: oracle.cpu_rx(x, trace=True, mode=mode), name)


@pytest.mark.parametrize("name", ["clean", "eb4", "wave", "impaired"])
@pytest.mark.parametrize("mode", [oracle.MODE_REF, oracle.MODE_DEC752])
def test_reference_is_even_in_its_input(mode, name):
    """ref_rx(x) == ref_rx(-x) on the unmodified reference, both builds."""
    if not oracle.ref_available(mode):
        pytest.skip("oracle/_ref not built")
    _assert_symmetric(lambda x: oracle.ref_rx(x, trace=True, mode=mode), name)


# ------------------------------------------------------- B. offset invariance
def _run_from(x, mode, frame):
    """One channel x [nframes][1880] through qc_rx_frame with ch->frame preset;
    (bits, trace) per frame."""
    lib = oracle.chan_lib()
    ch = oracle.Chan()
    lib.qc_chan_init_mode(C.byref(ch), mode)
    assert ch.frame == 0 and ch.rx_timing == 3 and ch.mode == mode, "qc_chan_t layout changed"
    ch.frame = frame
    nf = x.shape[0]
    bits = np.zeros((nf, 62), np.uint8)
    tr = np.zeros(nf, oracle.TRACE_DTYPE)
    for n in range(nf):
        v = lib.qc_rx_frame(C.byref(ch), x[n].ctypes.data, bits[n].ctypes.data, tr[n:n + 1].ctypes.data)
        assert v == tr["valid"][n]
    assert ch.frame == (frame + nf) & 0xffffffff
    return bits, tr


def _keywords(first, nf):
    """The 62 keystream bits of frames first .. first + nf - 1 (src/scramble.c:
    bit 62 g + b of a stream of period 32767)."""
    ks = oracle.keystream(32767)
    idx = (62 * (first + np.arange(nf))[:, None] + np.arange(62)[None, :]) % 32767
    return ks[idx]


@pytest.mark.parametrize("mode", CPU_MODES)
def test_a_start_at_another_frame_index_changes_the_keystream_only(mode):
    """qc_rx_frame with ch->frame preset to g: everything but the bits equals
    the run from 0, and the bits equal it once both keystreams are removed.
    The restatement's counter is 32 bits wide, so 2^32 + 1 is held as 1 (the
    keystream is removed at the index the receiver holds)."""
    x = np.concatenate([oracle.synth(21, 6, 12, 1000.0), oracle.synth(22, 6, 12, 6.0)])
    nf = x.shape[1]
    base = [_run_from(x[c], mode, 0) for c in range(x.shape[0])]
    assert sum(int(tr["valid"].sum()) for _, tr in base) >= 12
    for g in (1, 2, 777, 1056, 1057, 2**32 + 1):
        held = g & 0xffffffff
        for c in range(x.shape[0]):
            bits0, tr0 = base[c]
            bits, tr = _run_from(x[c], mode, held)
            for f in TRACE_FIELDS:
                np.testing.assert_array_equal(tr[f], tr0[f], err_msg=f"{f} at g = {g}")
            np.testing.assert_array_equal(tr["soft"].view(np.uint32), tr0["soft"].view(np.uint32))
            vm = tr0["valid"].astype(bool)
            np.testing.assert_array_equal((bits ^ _keywords(held, nf))[vm], (bits0 ^ _keywords(0, nf))[vm])
            assert not bits[~vm].any()
            if held % KS_FRAMES:
                assert (bits[vm] != bits0[vm]).any(), "the keystream did not move"
            else:
                np.testing.assert_array_equal(bits, bits0)


# --------------------------------------------------------- C. index arithmetic
@pytest.fixture(scope="module")
def index_out(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("index") / "rx_index_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *SAN, "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    "-o", exe, os.path.join(ROOT, "tests", "sanitize", "rx_index_check.cc")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"rx_index_check failed ({r.returncode}):\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_index_arithmetic(index_out):
    """Own and context indices at 0, 1056, 1057, 2113, 2^32 +- 1, 2^63 and
    2^64 - 1, every pair: koff in [0, 1057) and equal to (own - ctx) mod 1057
    computed in 128 bits; the host's lead gives the own index back exactly."""
    assert "FAILED" not in index_out
    assert index_out.splitlines()[-1] == "pairs 64"
