"""tests/rxcheck.py's comparison, tested by mutation (CPU only): a comparison
that passes silently is the worst failure this suite can have.  Each case
changes one element of a copy of the oracle's outputs, and `differences` must
name exactly that output, once, at the right (channel, frame)."""
import numpy as np
import pytest

import oracle
import rxcheck

CH, INVALID_FRAME = 2, 4    # frames 0 and 1 of every channel are valid, the others are not


@pytest.fixture(scope="module")
def exp():
    """4 channels x 6 frames at 4 dB: 8 valid frames of 24, no NaN."""
    e = rxcheck.expected(oracle.synth(7, 4, 6, 4.0))
    valid = e["valid"]
    assert 0 < valid.sum() < valid.size
    assert valid[CH, 1] and not valid[CH, INVALID_FRAME]
    assert not np.isnan(e["soft"]).any()
    return e


def _copy(e):
    return {k: v.copy() for k, v in e.items()}


def _bits(a):
    return a.view(np.uint32)


def test_equal_outputs_have_no_difference(exp):
    assert rxcheck.differences(_copy(exp), exp) == {}
    rxcheck.assert_same(_copy(exp), exp)


def test_one_bit(exp):
    got = _copy(exp)
    got["bits"][CH, 1, 17] ^= 1
    assert rxcheck.differences(got, exp) == {"bits": (1, (CH, 1))}


def test_one_valid_flag(exp):
    got = _copy(exp)
    got["valid"][3, 5] ^= 1
    assert rxcheck.differences(got, exp) == {"valid": (1, (3, 5))}


@pytest.mark.parametrize("col", range(4), ids=rxcheck.TRACE_COLS)
def test_each_trace_column_on_its_own(exp, col):
    got = _copy(exp)
    got["trace"][1, 3, col] += 1
    assert rxcheck.differences(got, exp) == {"trace." + rxcheck.TRACE_COLS[col]: (1, (1, 3))}


def test_one_ulp_in_a_valid_frame(exp):
    got = _copy(exp)
    _bits(got["soft"])[CH, 1, 30, 1] ^= 1
    assert rxcheck.differences(got, exp) == {"soft(valid)": (1, (CH, 1))}


def test_the_sign_of_zero_in_a_valid_frame(exp):
    e, got = _copy(exp), _copy(exp)
    e["soft"][CH, 0, 5, 0] = 0.0
    got["soft"][CH, 0, 5, 0] = -0.0
    assert got["soft"][CH, 0, 5, 0] == e["soft"][CH, 0, 5, 0]
    assert rxcheck.differences(got, e) == {"soft(valid)": (1, (CH, 0))}


@pytest.mark.parametrize("value", [-0.0, 1e-40, 1.0])
def test_anything_but_zero_bits_in_an_invalid_frame(exp, value):
    got = _copy(exp)
    got["soft"][CH, INVALID_FRAME, 0, 1] = value
    assert rxcheck.differences(got, exp) == {"soft(invalid) != 0": (1, (CH, INVALID_FRAME))}


def test_assert_same_raises_and_reports(exp, capsys):
    got = _copy(exp)
    got["trace"][0, 2, 2] ^= 1
    with pytest.raises(AssertionError, match="trace.valid"):
        rxcheck.assert_same(got, exp, "case")
    assert "case: trace.valid differs on 1 channel-frames, first at (channel, frame) (0, 2)" in capsys.readouterr().out


def test_the_oracles_triple_is_converted(exp):
    x = oracle.synth(7, 4, 6, 4.0)
    triple = oracle.cpu_rx(x, trace=True)
    assert rxcheck.differences(_copy(exp), triple) == {}
    got = _copy(exp)
    got["trace"][1, 1, 3] -= 1
    assert rxcheck.differences(got, triple) == {"trace.rx_timing": (1, (1, 1))}


def test_an_expected_nan_is_a_class_only_on_request(exp):
    e, got = _copy(exp), _copy(exp)
    _bits(e["soft"])[CH, 1, 2, 0] = 0x7FC00000
    _bits(got["soft"])[CH, 1, 2, 0] = 0xFFC00001   # another sign and payload
    assert rxcheck.differences(got, e, nan_as_class=True) == {}
    with pytest.raises(AssertionError, match="nan_as_class"):
        rxcheck.differences(got, e)
    with pytest.raises(AssertionError, match="nan_as_class"):
        rxcheck.assert_same(got, e)


@pytest.mark.parametrize("nan_as_class", [False, True])
def test_a_nan_for_a_finite_value_differs(exp, nan_as_class):
    got = _copy(exp)
    got["soft"][CH, 1, 2, 0] = np.nan
    assert rxcheck.differences(got, exp, nan_as_class=nan_as_class) == {"soft(valid)": (1, (CH, 1))}


def test_optional_outputs(exp):
    """Without trace and soft the rest is compared and nothing is reported for them."""
    got = {k: exp[k].copy() for k in ("bits", "valid")}
    assert rxcheck.differences(got, exp) == {}
    got["bits"][0, 0, 0] ^= 1
    assert rxcheck.differences(got, exp) == {"bits": (1, (0, 0))}
    got["trace"] = exp["trace"].copy()
    assert rxcheck.differences(got, exp) == {"bits": (1, (0, 0))}


def test_shapes_and_the_soft_dtype_must_match(exp):
    """Nothing is broadcast and nothing is cast: an output of another shape (a
    single frame or channel, a scalar-like array) or float64 soft symbols are
    refused, whatever their values."""
    for k, cut in (("valid", np.s_[:, :1]), ("bits", np.s_[:1]), ("trace", np.s_[:, :1]), ("soft", np.s_[:1, :1])):
        got = _copy(exp)
        got[k] = got[k][cut]
        with pytest.raises(AssertionError, match=k + ": shape"):
            rxcheck.differences(got, exp)
    got = _copy(exp)
    got["bits"] = got["bits"][..., :1] * 0 + exp["bits"][0, 0, 0]
    with pytest.raises(AssertionError, match="bits: shape"):
        rxcheck.differences(got, exp)
    got = _copy(exp)
    got["soft"] = got["soft"].astype(np.float64)
    with pytest.raises(AssertionError, match="soft: dtypes"):
        rxcheck.differences(got, exp)


class _Stub:
    """Stands in for a Receiver: echoes the frames of each call."""

    def __init__(self):
        self.calls = []

    def demod(self, x, **kw):
        assert x.flags.c_contiguous
        self.calls.append((x.shape[1], kw))
        return {"bits": x[:, :, :2].copy(), "valid": x[:, :, 0].copy()}


def test_demod_in_calls():
    x = np.arange(2 * 5 * 3, dtype=np.int16).reshape(2, 5, 3)
    rx = _Stub()
    out = rxcheck.demod_in_calls(rx, x, [1, 3, 1])
    assert rx.calls == [(n, {"trace": True, "soft": True}) for n in (1, 3, 1)]
    np.testing.assert_array_equal(out["bits"], x[:, :, :2])
    np.testing.assert_array_equal(out["valid"], x[:, :, 0])
    rx = _Stub()
    rxcheck.demod_in_calls(rx, x, [5], soft=False)
    assert rx.calls == [(5, {"trace": True, "soft": False})]
    for calls in ([1, 3], [2, 4], []):
        rx = _Stub()
        with pytest.raises(AssertionError):
            rxcheck.demod_in_calls(rx, x, calls)
        assert rx.calls == []


def test_frozen_and_expected_are_read_only(exp):
    a, d, n = rxcheck.frozen(np.zeros(3), {"k": np.zeros(2)}, None)
    assert n is None and not a.flags.writeable and not d["k"].flags.writeable
    with pytest.raises(ValueError):
        a[0] = 1
    assert all(not v.flags.writeable for v in exp.values())
    assert exp["trace"].dtype == np.int32 and exp["trace"].shape == (4, 6, 4)
    assert exp["soft"].dtype == np.float32 and not _bits(exp["soft"])[exp["valid"] == 0].any()


def test_shapes_and_force_shape(monkeypatch):
    assert rxcheck.ALL_SHAPES == [("4x2", None), ("2x4d", None), ("1x8", "64"), ("1x8", "32"), ("1x8", "16")]
    import os
    monkeypatch.delenv("QPSK_SHAPE", raising=False)
    monkeypatch.delenv("QPSK_WIDTH", raising=False)
    rxcheck.force_shape(monkeypatch, None, None)
    assert "QPSK_SHAPE" not in os.environ and "QPSK_WIDTH" not in os.environ
    rxcheck.force_shape(monkeypatch, "1x8", "32")
    assert (os.environ["QPSK_SHAPE"], os.environ["QPSK_WIDTH"]) == ("1x8", "32")
