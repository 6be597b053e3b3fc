"""tests/fingerprint_ref.py against numpy: the radix select's order statistics are bit-equal to np.sort(x)[rank] (sorted by
value; where -0.0 and +0.0 tie, numpy's order among them is free, so zeros are compared by value and by key order), and its
percentiles equal np.percentile(x.astype(float64), q) to relative 1e-12 of max(|lo|, |hi|): both are one subtraction, one
multiplication and one addition in float64 on the same two exact order statistics."""
import numpy as np
import pytest

import fingerprint_ref as ref


def _arrays():
    rng = np.random.default_rng(11)
    tiny = np.float32(1e-45)                                   # the smallest denormal
    near = np.float32(1.0) + np.arange(9, dtype=np.float32) * np.float32(2.0 ** -23)     # differ in the last digit only
    out = {
        "normal": rng.standard_normal(5000).astype(np.float32) * 300,
        "heavy duplicates": rng.choice(np.array([-3.5, 0.0, 2.0, 2.0, 7.25], dtype=np.float32), 4000),
        "CT integers": rng.integers(-1024, 3071, 6000).astype(np.float32),
        "CT pile": np.concatenate([np.full(3000, 40.0, np.float32), rng.integers(-100, 200, 500).astype(np.float32)]),
        "both zeros": np.array([0.0, -0.0, 0.0, -0.0, -0.0, 1.0, -1.0, 0.0], dtype=np.float32),
        "denormals": np.array([tiny, -tiny, 3 * tiny, 0.0, -2 * tiny, 7 * tiny, np.float32(1.1754944e-38)], dtype=np.float32),
        "last digit": rng.permutation(np.concatenate([near, near, -near])),
        "wide": (rng.standard_normal(3000) * 10.0 ** rng.integers(-30, 30, 3000)).astype(np.float32),
        "straddle": np.linspace(-1, 1, 1001).astype(np.float32),
        "all equal": np.full(777, -12.5, np.float32),
        "n=1": np.array([3.25], dtype=np.float32),
        "n=2": np.array([5.0, -1.5], dtype=np.float32),
        "n=3": np.array([2.0, 2.0, -8.0], dtype=np.float32),
    }
    return out


ARRAYS = _arrays()


def test_key_order_is_value_order():
    x = np.concatenate([a for a in ARRAYS.values()])
    k = ref.key_of(x)
    order = np.argsort(k, kind="stable")
    assert (np.diff(x[order].astype(np.float64)) >= 0).all()
    assert all(np.array_equal(np.array([ref.value_of(q)]).view(np.uint32), np.array([v]).view(np.uint32)) for q, v in zip(k[:200], x[:200]))
    assert ref.key_of(np.array([-0.0], np.float32))[0] + 1 == ref.key_of(np.array([0.0], np.float32))[0]


@pytest.mark.parametrize("name", sorted(ARRAYS))
def test_order_statistics_are_bit_equal_to_sort(name):
    x = ARRAYS[name]
    ranks = sorted({r for lo, hi, _ in ref.quantile_ranks(x.size) for r in (lo, hi)} | {0, x.size - 1})
    by_key = x[np.argsort(ref.key_of(x), kind="stable")]
    by_value = np.sort(x)
    for r in ranks:
        got = ref.radix_select(x, r)
        assert got.dtype == np.float32
        assert np.array([got]).view(np.uint32)[0] == np.array([by_key[r]]).view(np.uint32)[0], (name, r)
        assert got == by_value[r], (name, r)
        if by_value[r] != 0:
            assert np.array([got]).view(np.uint32)[0] == np.array([by_value[r]]).view(np.uint32)[0], (name, r)


@pytest.mark.parametrize("name", sorted(ARRAYS))
def test_percentiles_equal_numpy(name):
    x = ARRAYS[name]
    want = np.percentile(x.astype(np.float64), ref.QUANTILES)
    for (lo, hi, got), w in zip(ref.percentiles(x), want):
        assert abs(got - w) <= 1e-12 * max(abs(float(lo)), abs(float(hi))), (name, got, w)


@pytest.mark.parametrize("name", sorted(ARRAYS))
def test_moments_equal_numpy(name):
    x = ARRAYS[name]
    m = ref.moments(x)
    x64 = x.astype(np.float64)
    assert m["count"] == x.size and m["min"] == x.min() and m["max"] == x.max()
    assert m["mean"] == pytest.approx(x64.mean(), rel=1e-13, abs=1e-300)
    assert m["std"] == pytest.approx(x64.std(), rel=1e-12, abs=1e-300)
