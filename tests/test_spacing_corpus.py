"""What the corpus of tests/spacing.py reaches, asserted on the oracle's results
alone (no GPU): the cases of tests/test_gpu_spacing.py compare the kernels with
the oracle on this input, and the conditions here keep them from passing on a
corpus that no longer reaches a pair of incoming rx_timing and max_index, a
timing carried through an invalid frame, the validity threshold or a hunt the
filtered rule leaves undecided.  The oracle itself is pinned to the reference
on the corpus: bit for bit where oracle/_ref is built, by digest everywhere.

Pairs, over rx_timing 128..255 (16,384 of each):
  A  (rt_in(n), max_index(n)),      frame n valid;
  B  (rt_in(n), max_index(n + 1)),  frames n and n + 1 valid.
No pair is excepted.

The fresh row.  rx_timing 3 is what a channel's first call starts with, and
that call's window is the zero-initialised decimated_frame: it is valid at
max_index 0 on every input and leaves rx_timing 128.  (3, m) with m != 0 is
therefore no state of the reference at all, whatever the samples, and A's row
3 is asserted to be exactly {0}.

Figures measured when the corpus was made: 5,472 channels x 12 frames = 65,664
frames (directed 2,560 channels, random 2,048, carried 768, tails 96).
  mode  valid    A       B       carried  undecided / valid / distinct max_index
  0     58,483   16,384  16,384  128      816 / 777 / 100
  1     58,032   16,384  16,384  128      676 / 673 /  68
  2     58,483   16,384  16,384  128
  3     58,032   16,384  16,384  128
  every mode: a valid frame at matches = 99, an invalid one at 98; A's row 3
  holds max_index 0 alone.
  The directed group by itself holds all 16,384 pairs of A and of B in every
  mode, with every frame valid.
  The carried group by itself carries all 128 timings in every mode.
For comparison, timing.sweep() reaches 1,287 pairs of A and 394 of B in mode 0
(1,130 and 220 in mode 1); with sweep_noisy 1,698 and 394 (1,150 and 220).
"""
import json
import os

import numpy as np
import pytest

import oracle
import spacing
import timing

ALL_MODES = [0, 1, 2, 3]
DIRECT = [oracle.MODE_REF, oracle.MODE_DEC752]
TIMINGS = set(range(128, 256))
EXCEPT_A = {0: [], 1: [], 2: [], 3: []}     # (rx_timing, max_index) no directed attempt reaches: none
EXCEPT_B = {0: [], 1: [], 2: [], 3: []}
EXCEPT_CARRIED = {0: [], 1: [], 2: [], 3: []}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spacing_ref.json")


def _missing(table, excepted):
    assert len(excepted) <= 16
    want = np.ones((128, 128), bool)
    for r, m in excepted:
        want[r - 128, m] = False
    return np.argwhere(want & ~table[128:]) + [128, 0]


def test_corpus_size():
    x = spacing.corpus()
    assert x.dtype == np.int16 and x.shape[1:] == (spacing.NFRAMES, spacing.FRAME)
    assert x.shape[0] <= 8192
    assert not x.flags.writeable
    assert spacing.group_slices()["tails"].stop == x.shape[0]


@pytest.mark.parametrize("mode", ALL_MODES)
def test_every_pair_of_timing_and_position(mode):
    cv = spacing.pair_coverage(mode)
    a, b = cv["A"], cv["B"]
    print(mode, cv["nvalid"], cv["nframes"], int(a[128:].sum()), int(b[128:].sum()),
          int(a[spacing.RT_INITIAL].sum()), len(cv["carried"] & TIMINGS))
    ma, mb = _missing(a, EXCEPT_A[mode]), _missing(b, EXCEPT_B[mode])
    assert ma.size == 0, ma[:32].tolist()
    assert mb.size == 0, mb[:32].tolist()
    assert int(a[128:].sum()) + len(EXCEPT_A[mode]) == 16384
    assert int(b[128:].sum()) + len(EXCEPT_B[mode]) == 16384
    # the only rows there are: the fresh one and 128..255
    rows = set(np.flatnonzero(a.any(axis=1)).tolist())
    assert rows == TIMINGS | {spacing.RT_INITIAL}


@pytest.mark.parametrize("mode", ALL_MODES)
def test_fresh_row_is_the_silent_first_frame(mode):
    """See the module docstring: rx_timing 3 meets the zero-initialised window
    only, so A's row 3 is max_index 0, on every channel's frame 0 and nowhere
    else."""
    _, valid, tr = spacing.expected(mode)
    rt = timing.rt_in(tr)
    assert (rt[:, 0] == spacing.RT_INITIAL).all() and (rt[:, 1:] != spacing.RT_INITIAL).all()
    assert valid[:, 0].all() and not tr["max_index"][:, 0].any()
    assert np.flatnonzero(spacing.pair_coverage(mode)["A"][spacing.RT_INITIAL]).tolist() == [0]


@pytest.mark.parametrize("mode", ALL_MODES)
def test_directed_group_alone_holds_every_pair(mode):
    """The construction, not luck: every frame of the directed group is valid
    and found where it was placed, so the group by itself holds A and B."""
    s = spacing.group_slices()["directed"]
    cv = spacing.pair_coverage(mode, s)
    assert cv["nvalid"] == cv["nframes"]
    assert cv["A"][128:].all() and cv["B"][128:].all()


@pytest.mark.parametrize("mode", ALL_MODES)
def test_timing_carried_through_an_invalid_frame(mode):
    """For every rx_timing 128..255 an invalid frame starts with it and a valid
    frame follows.  (An invalid frame's window is never silent: silence is
    valid and resets the timing to 128.)"""
    cv = spacing.pair_coverage(mode)
    assert len(EXCEPT_CARRIED[mode]) <= 16
    assert TIMINGS - cv["carried"] - set(EXCEPT_CARRIED[mode]) == set()
    own = spacing.pair_coverage(mode, spacing.group_slices()["carried"])["carried"]
    print(mode, len(cv["carried"] & TIMINGS), len(own & TIMINGS))
    assert TIMINGS <= own                           # by the group built for it, not by luck


@pytest.mark.parametrize("mode", ALL_MODES)
def test_validity_threshold_from_both_sides(mode):
    cv = spacing.pair_coverage(mode)
    assert cv["min_matches_valid"] == 99
    assert cv["max_matches_invalid"] == 98


@pytest.mark.parametrize("mode", DIRECT)
def test_undecided_hunts_on_valid_frames(mode):
    """Non-zero windows on which the filtered hunt's rule commits to no lag,
    on valid frames at 32 or more distinct max_index: the exact chain runs on
    real signal.  hunt_classes' recomputed max_index is the oracle's."""
    hc = timing.hunt_classes(spacing.corpus(), mode)
    _, valid, tr = spacing.expected(mode)
    np.testing.assert_array_equal(hc["max_index"], tr["max_index"])
    und = hc["undecided"] & ~hc["zero"]
    uv = und & valid.astype(bool)
    nmi = len(set(tr["max_index"][uv].tolist()))
    print(mode, int(und.sum()), int(uv.sum()), nmi, int((~hc["zero"]).sum()))
    assert nmi >= 32
    for name in ("random", "tails"):              # bursts that arrived so, and the directed pieces
        assert uv[spacing.group_slices()[name]].any()


@pytest.mark.parametrize("mode", DIRECT)
def test_old_sweeps_for_comparison(mode):
    """What tests/timing.py's sweeps reach of the same tables: a few lines of
    the plane.  Printed, and bounded from above so the docstrings stay true."""
    n = {}
    for name in ("sweep", "sweep_noisy"):
        _, valid, tr = timing.expected(name, mode)
        n[name] = spacing.pairs(valid, tr)[:2]
    a = n["sweep"][0] | n["sweep_noisy"][0]
    b = n["sweep"][1] | n["sweep_noisy"][1]
    print(mode, int(n["sweep"][0][128:].sum()), int(n["sweep"][1][128:].sum()),
          int(a[128:].sum()), int(b[128:].sum()))
    assert a[128:].sum() < 16384 // 8 and b[128:].sum() < 16384 // 8


@pytest.mark.parametrize("mode", DIRECT)
def test_oracle_equals_the_reference_on_the_corpus(mode):
    """The unmodified reference against the restatement on every channel:
    bits, valid flags, the trace and the soft symbols of valid frames, bit for
    bit."""
    if not oracle.ref_available(mode):
        pytest.skip("reference build not present")
    assert timing.same_as_reference(spacing.corpus(), mode, "spacing") > 0


@pytest.mark.parametrize("mode", DIRECT)
def test_oracle_equals_the_references_digests(mode):
    """With or without the reference build: the oracle's outputs over the
    whole corpus hash to what the reference's own did."""
    import hashlib
    with open(GOLDEN) as f:
        gold = json.load(f)
    x = spacing.corpus()
    assert list(x.shape[:2]) == [gold["channels"], gold["frames"]]
    assert hashlib.sha256(x.tobytes()).hexdigest() == gold["input_sha256"]
    assert spacing.digests(*spacing.expected(mode)) == gold["modes"][str(mode)]
