"""Deterministic corpora for the data-dependent paths of the receive front:
every preamble position, every incoming rx_timing, and preamble hunts whose
maximum is held by two lags at exactly the same value.

Plain module, integer arithmetic plus oracle.synth (the C generator, the same
on every machine); no GPU import.  Arrays are made once and are read-only.

sweep(nf)         [2783][nf][1880]: the modem's noiseless signal at every delay
                  of one packet period (640 + 8 * 31 * 5 + 903 = 2783 samples).
                  The base stream is oracle.synth(SEED, 1, nf + 3)[0] without
                  its leading zeros (1740 of them at SEED = 5); channel d is d
                  zeros followed by it.  The preamble so falls on every
                  max_index 0..127 and leaves every rx_timing 128..255 behind.
sweep_noisy(nf, ebn0)
                  sweep(nf) plus the generator's own AWGN: the int32 difference
                  synth(SEED + 1, 2783, nf, ebn0) - synth(SEED + 1, 2783, nf, 1000.0),
                  the sum clipped to int16.  Match counts then land on both
                  sides of the validity threshold (src/qpsk.c:196), and invalid
                  frames occur at most incoming rx_timing values.
impulses(nf)      One block of channels per amplitude a in AMPS; in each, for
                  t in range(0, 1880, IMPULSE_STEP), a channel that is zero
                  but for x[1][t] = a and x[2][(3 t) % 1880] = -a.  One
                  non-zero sample leaves about 10 non-zero decimated symbols;
                  two lags whose preamble signs over those are equal or
                  negated sum the same terms in the same order, so their
                  cnormf is bitwise equal: an exact tie at the hunt's maximum,
                  which must go to the first lag (src/qpsk.c:172-183).

coverage() and hunt_classes() say, from the oracle alone, what a corpus
reaches; tests/test_timing_corpus.py asserts it, so that the GPU cases of
tests/test_gpu_timing.py cannot pass on an empty corpus.
"""
import functools

import numpy as np

import oracle
from rxcheck import frozen

FRAME = 1880
PERIOD = 640 + 8 * 31 * 5 + 903    # samples from one packet's start to the next
SEED = 5
AMPS = (1, 32767)
IMPULSE_STEP = 7
RT_INITIAL = 3                     # FINE_TIMING_OFFSET, a fresh channel's rx_timing
assert PERIOD == 2783

# what tests/test_gpu_timing.py and tests/test_gpu_spacing.py run on: receiver modes (the oracle's
# numbers are the library's), the two whose hunt hunt_classes restates, and the frames of a split
# stream's first calls (then the remaining frames)
MODES = [0, 1, 2, 3]
DIRECT = [oracle.MODE_REF, oracle.MODE_DEC752]
CALLS = (1, 1, 2, 1)


@functools.lru_cache(maxsize=None)
def base(nf=6):
    """The noiseless stream of nf + 3 frames without its lead delay."""
    s = oracle.synth(SEED, 1, nf + 3)[0].reshape(-1)
    nz = np.flatnonzero(s)
    assert nz.size and s.size - nz[0] >= nf * FRAME
    return frozen(s[nz[0]:].copy())[0]


@functools.lru_cache(maxsize=None)
def sweep(nf=6):
    b = base(nf)
    n = nf * FRAME
    x = np.zeros((PERIOD, n), np.int16)
    for d in range(PERIOD):
        x[d, d:] = b[:n - d]
    return frozen(x.reshape(PERIOD, nf, FRAME))[0]


@functools.lru_cache(maxsize=None)
def sweep_noisy(nf=6, ebn0=4.0):
    y = oracle.synth(SEED + 1, PERIOD, nf, ebn0).astype(np.int32)
    y -= oracle.synth(SEED + 1, PERIOD, nf, 1000.0)    # the noise alone, int32
    y += sweep(nf)
    np.clip(y, -32768, 32767, out=y)
    return frozen(y.astype(np.int16))[0]


@functools.lru_cache(maxsize=None)
def impulses(nf=4):
    assert nf >= 3
    ts = range(0, FRAME, IMPULSE_STEP)
    x = np.zeros((len(AMPS), len(ts), nf, FRAME), np.int16)
    for k, a in enumerate(AMPS):
        for c, t in enumerate(ts):
            x[k, c, 1, t] = a
            x[k, c, 2, (3 * t) % FRAME] = -a
    return frozen(x.reshape(-1, nf, FRAME))[0]


CORPORA = {"sweep": sweep, "sweep_noisy": sweep_noisy, "impulses": impulses}


def corpus(name):
    return CORPORA[name]()


@functools.lru_cache(maxsize=None)
def expected(name, mode=0):
    """The oracle's (bits, valid, trace) for a corpus, computed once, read-only."""
    return frozen(*oracle.cpu_rx(corpus(name), trace=True, mode=mode))


def same_as_reference(x, mode, what):
    """The oracle against the unmodified reference on x, bit for bit; returns
    the number of valid frames."""
    bits, valid, tr = oracle.cpu_rx(x, trace=True, mode=mode)
    rbits, rvalid, rtr = oracle.ref_rx(x, trace=True, mode=mode)
    np.testing.assert_array_equal(valid, rvalid, err_msg=what)
    np.testing.assert_array_equal(bits, rbits, err_msg=what)
    for k in ("max_index", "matches", "valid", "rx_timing"):
        np.testing.assert_array_equal(tr[k], rtr[k], err_msg=f"{what}: {k}")
    vm = valid.astype(bool)
    np.testing.assert_array_equal(tr["soft"][vm].view(np.uint32), rtr["soft"][vm].view(np.uint32),
                                  err_msg=what)
    return int(vm.sum())


def rt_in(tr):
    """The rx_timing each frame starts with: the previous frame's traced value,
    the initial one for the first frame."""
    rt = np.empty(tr.shape, np.int32)
    rt[:, 0] = RT_INITIAL
    rt[:, 1:] = tr["rx_timing"][:, :-1]
    return rt


def coverage(x, mode=0, exp=None):
    """What the oracle's run over x reaches: the max_index values of valid
    frames, the incoming rx_timing values of valid and of invalid frames, the
    smallest match count of a valid frame and the largest of an invalid one."""
    _, valid, tr = exp if exp is not None else oracle.cpu_rx(x, trace=True, mode=mode)
    vm = valid.astype(bool)
    rt = rt_in(tr)
    return {
        "nvalid": int(vm.sum()),
        "nframes": int(vm.size),
        "mi_valid": set(np.unique(tr["max_index"][vm]).tolist()),
        "rt_valid": set(np.unique(rt[vm]).tolist()),
        "rt_invalid": set(np.unique(rt[~vm]).tolist()),
        "min_matches_valid": int(tr["matches"][vm].min()) if vm.any() else None,
        "max_matches_invalid": int(tr["matches"][~vm].max()) if (~vm).any() else None,
    }


# ---------------------------------------------------------------- the hunt
def ref_sums_index(dec):
    """The reference's hunt (src/qpsk.c:88-96, 172-183) over windows dec
    [n][255] complex64, in float32 and in its order of operations: the sums'
    real and imaginary parts [n][128], max_index, and W = sum |T| + |U|."""
    p = oracle.preamble().astype(np.float32)
    dr, di = dec.real.astype(np.float32), dec.imag.astype(np.float32)
    tr, ti = (dr - di).astype(np.float32), (di + dr).astype(np.float32)
    n = dec.shape[0]
    re = np.zeros((n, 128), np.float32)
    im = np.zeros((n, 128), np.float32)
    for i in range(128):
        re = (re + p[i] * tr[:, i:i + 128]).astype(np.float32)
        im = (im + p[i] * ti[:, i:i + 128]).astype(np.float32)
    c = (re * re + im * im).astype(np.float32)
    best = np.zeros(n, np.float32)
    idx = np.zeros(n, np.int64)
    for lag in range(128):
        up = c[:, lag] > best
        best = np.where(up, c[:, lag], best)
        idx = np.where(up, lag, idx)
    w = (np.abs(tr) + np.abs(ti)).sum(axis=1, dtype=np.float64).astype(np.float32)
    return re, im, idx, w


def pick(sr, si, w):
    """pick_h (singlecarrier_amd/csrc/qpsk_hunt.h) in float32: -1 when undecided."""
    f32 = np.float32
    d = (w * f32(2.0 ** -13) + f32(2.0 ** -100)).astype(f32)[:, None]
    ar, ai = np.abs(sr), np.abs(si)
    ur, ui = (ar + d).astype(f32), (ai + d).astype(f32)
    lr = np.maximum((ar - d).astype(f32), f32(0))
    li = np.maximum((ai - d).astype(f32), f32(0))
    U = ((ur * ur).astype(f32) + (ui * ui).astype(f32)).astype(f32) * f32(1 + 2.0 ** -18)
    L = ((lr * lr).astype(f32) + (li * li).astype(f32)).astype(f32) * f32(1 - 2.0 ** -18)
    lm = L.max(axis=1)
    cand = U >= lm[:, None]
    ok = (lm > 0) & (cand.sum(axis=1) == 1)
    return np.where(ok, np.argmax(cand, axis=1), -1)


def hunt_windows(x, mode=0):
    """The hunt's input dec[0..254] of every frame, [nch][nf][255] complex64,
    from the oracle's stages."""
    assert mode in (oracle.MODE_REF, oracle.MODE_DEC752)
    x = np.asarray(x)
    out = np.empty(x.shape[:2] + (255,), np.complex64)
    for c in range(x.shape[0]):
        dec = oracle.cpu_stages(x[c], mode)[:, :255]
        out[c] = dec[..., 0] + 1j * dec[..., 1]
    return out


def hunt_classes(x, mode=0):
    """Per-frame masks [nch][nf] of the direct hunt (modes 0 and 1) over x:
      zero       the window dec[0..254] is all zero;
      undecided  the filtered hunt's rule (pick) commits to no lag on the
                 reference's own sums, so no sums within its error budget let
                 it commit either: the frame goes to the exact chain;
      tie        two or more lags hold exactly the maximum cnormf;
      split      the first and the last lag at the maximum differ;
    and max_index, recomputed here as the reference computes it."""
    dec = hunt_windows(x, mode)
    shape = dec.shape[:2]
    dec = dec.reshape(-1, 255)
    re, im, idx, w = ref_sums_index(dec)
    c = (re * re + im * im).astype(np.float32)
    at_max = c == c.max(axis=1)[:, None]
    first = np.argmax(at_max, axis=1)
    last = 127 - np.argmax(at_max[:, ::-1], axis=1)
    out = {
        "zero": ~dec.any(axis=1),
        "undecided": pick(re, im, w) < 0,
        "tie": at_max.sum(axis=1) >= 2,
        "split": first != last,
        "max_index": idx,
    }
    return {k: v.reshape(shape) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def tied_channels(mode=0, n=16):
    """The first n channels of impulses() that hold a non-zero window with an
    exact tie at the maximum and first != last maximum lag."""
    hc = hunt_classes(impulses(), mode)
    ch = np.flatnonzero((hc["split"] & ~hc["zero"]).any(axis=1))[:n]
    assert ch.size == n
    return frozen(ch)[0]
