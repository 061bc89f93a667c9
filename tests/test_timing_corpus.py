"""What the corpora of tests/timing.py reach, asserted on the oracle's results
alone (no GPU): the cases of tests/test_gpu_timing.py compare the kernels with
the oracle on these inputs, and the conditions here keep them from passing on
a corpus that no longer reaches a preamble position, an incoming rx_timing,
the validity threshold or an exact tie at the hunt's maximum.

Figures measured when the corpora were made (valid frames of 16,698, distinct
max_index on valid frames, distinct incoming rx_timing on valid / invalid
frames):
  sweep        mode 0: 10,715, 128, 129 / 112    mode 1: 11,339, 128, 129 / 113
               mode 2: 10,715, 128, 129 / 112    mode 3: 11,339, 128, 129 / 114
  sweep_noisy  mode 0:  6,014, 122,  49 / 120    mode 1:  6,385, 128,  38 / 128
  both sweeps, every mode: a valid frame at matches = 99, an invalid one at 98
  impulses     mode 0: 54 non-zero windows (27 per amplitude) with an exact tie
               and first != last maximum lag, at 26 distinct max_index;
               mode 1: 44 (22 per amplitude) at 22; every one of those frames
               valid and undecided by the filtered hunt's rule.

What these corpora do not claim: the pairs (incoming rx_timing 128..255,
max_index) on valid frames.  Every channel of the sweeps is one clocked stream
at some delay, so of the 16,384 pairs sweep reaches 1,287 in mode 0 (1,130 in
mode 1) and both sweeps together 1,698 (1,150); of the pairs (rx_timing of
frame n, max_index of frame n + 1), both frames valid, 394 (220).  The plane
is tests/spacing.py's, asserted in tests/test_spacing_corpus.py.
"""
import numpy as np
import pytest

import oracle
import timing

ALL_MODES = [0, 1, 2, 3]
DIRECT = [oracle.MODE_REF, oracle.MODE_DEC752]   # the hunts hunt_classes restates


@pytest.mark.parametrize("mode", ALL_MODES)
def test_sweep_reaches_every_position_and_timing(mode):
    """Every max_index 0..127, every incoming rx_timing 128..255 and the
    initial one occur on a valid frame."""
    cv = timing.coverage(timing.sweep(), mode, timing.expected("sweep", mode))
    print(mode, cv["nvalid"], cv["nframes"], len(cv["mi_valid"]), len(cv["rt_valid"]), len(cv["rt_invalid"]))
    assert cv["nframes"] == timing.PERIOD * 6
    assert cv["mi_valid"] == set(range(128))
    assert cv["rt_valid"] == set(range(128, 256)) | {timing.RT_INITIAL}


@pytest.mark.parametrize("name", ["sweep", "sweep_noisy"])
@pytest.mark.parametrize("mode", ALL_MODES)
def test_sweeps_hit_the_validity_threshold_from_both_sides(name, mode):
    """valid = matches > 98 (src/qpsk.c:196): some valid frame has 99 matches
    and some invalid frame has 98."""
    cv = timing.coverage(timing.corpus(name), mode, timing.expected(name, mode))
    assert cv["min_matches_valid"] == 99
    assert cv["max_matches_invalid"] == 98


@pytest.mark.parametrize("mode", DIRECT)
def test_noisy_sweep_has_invalid_frames_at_most_timings(mode):
    cv = timing.coverage(timing.sweep_noisy(), mode, timing.expected("sweep_noisy", mode))
    print(mode, cv["nvalid"], len(cv["mi_valid"]), len(cv["rt_valid"]), len(cv["rt_invalid"]))
    assert len(cv["rt_invalid"]) >= 112


@pytest.mark.parametrize("name", list(timing.CORPORA))
@pytest.mark.parametrize("mode", DIRECT)
def test_hunt_classes_recompute_the_oracles_max_index(name, mode):
    hc = timing.hunt_classes(timing.corpus(name), mode)
    tr = timing.expected(name, mode)[2]
    np.testing.assert_array_equal(hc["max_index"], tr["max_index"])
    assert not (hc["split"] & ~hc["tie"]).any()
    if name == "impulses":
        _impulse_ties(hc, mode)


def _impulse_ties(hc, mode):
    """Exact ties at the maximum of non-zero windows, first != last maximum
    lag: at least 16 of them at 12 or more distinct max_index, all on valid
    frames; and every one undecided by the filtered hunt's rule, so the
    kernels resolve it in their exact chain."""
    _, valid, tr = timing.expected("impulses", mode)
    sp = hc["split"] & ~hc["zero"]
    nmi = len(set(tr["max_index"][sp].tolist()))
    print(mode, int(sp.sum()), nmi, int((~hc["zero"]).sum()))
    assert sp.sum() >= 16
    assert nmi >= 12
    assert valid[sp].all()
    assert hc["undecided"][sp].all()
    per_amp = sp.reshape(len(timing.AMPS), -1)
    assert per_amp.any(axis=1).all()          # at the smallest and the largest amplitude
    assert sp[timing.tied_channels(mode)].any(axis=1).all()


@pytest.mark.parametrize("mode", DIRECT)
def test_oracle_equals_the_reference_on_the_corpora(mode):
    """The unmodified reference against the restatement on the impulses (exact
    ties included) and on every 16th channel of both sweeps: bits, valid
    flags, the trace and the soft symbols of valid frames, bit for bit."""
    if not oracle.ref_available(mode):
        pytest.skip("reference build not present")
    assert timing.same_as_reference(timing.impulses(), mode, "impulses") > 0
    for name in ("sweep", "sweep_noisy"):
        assert timing.same_as_reference(timing.corpus(name)[::16], mode, name) > 0
