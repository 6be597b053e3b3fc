"""GPU: the dataset-fingerprint kernels (csrc/fingerprint.hip) against tests/fingerprint_ref.py in float64.

Counts, min, max and the six order statistics (the ranks np.percentile needs for q = 0.5, 50, 99.5) are bit-equal; the
percentiles agree to relative 1e-12 of max(|lo|, |hi|) (three double operations on exact inputs).

Mean and std are held to two bounds.  The outer one is the a-priori bound of a sum of n doubles in any order: n * 2^-53 *
mean|x| and 4 n * 2^-53 * max|x - mean| (n: pooled foreground count).  The one that decides is fingerprint_ref.moment_bounds:
the same reasoning with the DEPTH of the kernels' summation tree (16 values per thread and step, the fixed tree of a workgroup,
the workgroups' partials, the cases: about 100 for the volumes below) and of numpy's pairwise sum in place of n - three orders of
magnitude below the outer bound at n = 2e5, so that a float32 accumulator, a lost centring or a partial added twice fails it.
Both come from operation counts; no figure of the kernels went into them.  The tests print error / bound of both (MEASURED)."""
import numpy as np
import pytest
import torch

import fingerprint_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG, SMALL, ONE = (70, 65, 67), (5, 3, 7), (1, 1, 1)      # several workgroups with a ragged tail; less than a wave; one voxel
LABEL_TYPES = {"uint8": np.uint8, "int16": np.int16, "int32": np.int32}
MEASURED = ("largest error / bound over the cases below on an MI355X (n up to 305 224): mean 0.0093 of the depth bound (4.2e-6 of the "
            "outer one), std 0.046 (1.7e-6): within an ulp or two of numpy's float64 values")


def _seg(rng, shape, fraction, dtype):
    seg = (rng.random(shape) < fraction).astype(dtype) * rng.integers(1, 100, shape).astype(dtype)
    if np.issubdtype(dtype, np.signedinteger):
        seg[rng.random(shape) < 0.05] = -1                   # nnU-Net's "outside the non-zero mask": not foreground
    return seg


def _scenarios(dtype):
    rng = np.random.default_rng(17)
    ct = lambda shape: rng.integers(-1024, 3071, shape).astype(np.float32)
    out = {}
    a, b, c = ct(BIG), ct(SMALL), (ct(BIG) * 0.25 + 500).astype(np.float32)
    out["a case without foreground between two with"] = [("a", a, _seg(rng, BIG, 0.4, dtype)), ("b", b, np.zeros(SMALL, dtype)),
                                                         ("c", c, _seg(rng, BIG, 0.3, dtype))]
    one = np.zeros(SMALL, dtype)
    one[2, 1, 4] = 3
    out["foreground count 1"] = [("a", ct(SMALL), one), ("b", ct(ONE), np.zeros(ONE, dtype))]
    out["one voxel"] = [("a", np.full(ONE, -7.5, np.float32), np.ones(ONE, dtype))]
    eq = ct(BIG)
    seg = _seg(rng, BIG, 0.5, dtype)
    eq[seg > 0] = -37.5
    out["all foreground values equal"] = [("a", eq, seg), ("b", np.full(SMALL, -37.5, np.float32), np.ones(SMALL, dtype))]
    st = (rng.standard_normal(BIG) * 1e-3).astype(np.float32)
    st[rng.random(BIG) < 0.2] = 0.0
    st[rng.random(BIG) < 0.2] = -0.0
    st[rng.random(BIG) < 0.01] = np.float32(1e-45)
    st[rng.random(BIG) < 0.01] = -np.float32(1e-45)
    out["values straddling zero"] = [("a", st, _seg(rng, BIG, 0.6, dtype))]
    lo, hi = rng.random(BIG).astype(np.float32), (rng.random(BIG) + 100).astype(np.float32)
    seg = _seg(rng, BIG, 0.5, dtype)
    out["the pooled median falls between the cases' ranges"] = [("a", lo, seg), ("b", hi, seg.copy())]
    return out


def _pooled(cases):
    return np.concatenate([x[seg > 0].astype(np.float32) for _, x, seg in cases])


def _run(cases):
    from dg_tta_amd.planning.fingerprint import MemoryCases, pooled_statistics_gpu
    dev_cases = [(name, torch.from_numpy(x[None]).to(DEV), torch.from_numpy(seg).to(DEV)) for name, x, seg in cases]
    return pooled_statistics_gpu(MemoryCases(dev_cases, DEV), 1)[0]


def _bits(v):
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


@pytest.mark.parametrize("label_type", sorted(LABEL_TYPES))
@pytest.mark.parametrize("scenario", sorted(_scenarios(np.uint8)))
def test_statistics_against_float64(scenario, label_type):
    from dg_tta_amd.planning.fingerprint import finish_statistics
    cases = _scenarios(LABEL_TYPES[label_type])[scenario]
    x = _pooled(cases)
    n = x.size
    assert n > 0
    got = _run(cases)
    assert got["count"] == n and got["nonfinite"] == 0 and got["first_nonfinite_case"] == -1
    assert _bits(got["min"]) == _bits(x.min()) and _bits(got["max"]) == _bits(x.max())
    assert float(np.float32(got["min"])) == got["min"] and float(np.float32(got["max"])) == got["max"]
    ranks = ref.quantile_ranks(n)
    assert sorted(got["order"]) == sorted({r for lo, hi, _ in ranks for r in (lo, hi)})
    by_key = x[np.argsort(ref.key_of(x), kind="stable")]
    for r, v in got["order"].items():
        assert _bits(v) == _bits(ref.radix_select(x, r)) == _bits(by_key[r]), (scenario, r)
        assert v == np.sort(x)[r]
    if scenario.startswith("the pooled median"):
        lo, hi, _ = ranks[1]
        assert got["order"][lo] < 1.0 and got["order"][hi] >= 100.0
    block = finish_statistics(got["count"], got["min"], got["max"], got["sum"], got["sumsq_centred"], got["order"])
    want = np.percentile(x.astype(np.float64), ref.QUANTILES)
    for key, (lo, hi, _), w in zip(("percentile_00_5", "median", "percentile_99_5"), ranks, want):
        a, b = got["order"][lo], got["order"][hi]
        assert abs(block[key] - w) <= 1e-12 * max(abs(a), abs(b)), (scenario, key, block[key], w)
    x64 = x.astype(np.float64)
    outer_mean = n * 2.0 ** -53 * float(np.abs(x64).mean())
    outer_std = 4 * n * 2.0 ** -53 * float(np.abs(x64 - x64.mean()).max())
    mean_bound, std_bound = ref.moment_bounds(x, [c[1].size for c in cases])
    mean_err, std_err = abs(block["mean"] - float(x64.mean())), abs(block["std"] - float(x64.std()))
    ratio = lambda err, bound: err / bound if bound else 0.0
    print(f"\n{scenario} [{label_type}] n={n}: mean error {mean_err:.3e} = {ratio(mean_err, mean_bound):.3g} of the depth bound, "
          f"{ratio(mean_err, outer_mean):.3g} of the outer bound; std error {std_err:.3e} = {ratio(std_err, std_bound):.3g} of the "
          f"depth bound, {ratio(std_err, outer_std):.3g} of the outer bound")
    assert mean_err <= mean_bound and std_err <= std_bound
    assert mean_err <= outer_mean and std_err <= outer_std
    if scenario.startswith("all foreground"):
        assert block["std"] == 0.0 and block["mean"] == -37.5 == block["median"]


def test_two_runs_give_identical_bits():
    cases = _scenarios(np.int16)["a case without foreground between two with"]
    a, b = _run(cases), _run(cases)
    assert a == b
    assert np.float64(a["sum"]).tobytes() == np.float64(b["sum"]).tobytes()
    assert np.float64(a["sumsq_centred"]).tobytes() == np.float64(b["sumsq_centred"]).tobytes()


@pytest.mark.parametrize("label_type", sorted(LABEL_TYPES))
def test_alignment_changes_no_bit(label_type):
    """Buffers that are not 16-byte aligned take scalar loads of the same voxels in the same order: the sums are bit-equal."""
    from dg_tta_amd import ops
    rng = np.random.default_rng(9)
    x = (rng.standard_normal(BIG) * 300).astype(np.float32).reshape(-1)
    seg = _seg(rng, BIG, 0.5, LABEL_TYPES[label_type]).reshape(-1)
    results = []
    for shift_x, shift_seg in ((0, 0), (1, 0), (0, 1), (3, 2)):
        xd = torch.zeros(x.size + 4, device=DEV)[shift_x:shift_x + x.size].copy_(torch.from_numpy(x))
        sd = torch.zeros(seg.size + 4, dtype=torch.from_numpy(seg).dtype, device=DEV)[shift_seg:shift_seg + seg.size].copy_(torch.from_numpy(seg))
        assert xd.is_contiguous() and xd.data_ptr() % 16 == 4 * shift_x
        state, counters = ops.fingerprint_state(DEV), ops.fingerprint_counters(DEV, 1)
        ops.fingerprint_sweep(xd, sd, counters, moment=1, state=state)
        first = ops.fingerprint_read_state(state)
        ops.fingerprint_sweep(xd, sd, counters, moment=2, state=state, mean=first["sum"] / first["count"])
        results.append((state.cpu(), counters.cpu()))
    for state, counters in results[1:]:
        assert torch.equal(state, results[0][0]) and torch.equal(counters, results[0][1])


def test_prefixed_histograms_are_exact():
    """One sweep with six prefixes, as the second and third sweeps run it: every counter equals the restatement's."""
    from dg_tta_amd import ops
    rng = np.random.default_rng(5)
    x = rng.integers(-200, 400, BIG).astype(np.float32)
    seg = _seg(rng, BIG, 0.5, np.uint8)
    keys = ref.key_of(x[seg > 0])
    xd, sd = torch.from_numpy(x).to(DEV), torch.from_numpy(seg).to(DEV)
    for prefix_bits, digit_bits in ((11, 11), (22, 10), (0, 11), (21, 11), (5, 3)):
        present = np.unique(keys >> np.uint32(32 - prefix_bits)) if prefix_bits else np.array([0])
        prefixes = [int(p) for p in present[:: max(len(present) // 5, 1)][:5]] + ([int(present[-1]) + 1] if prefix_bits else [])
        prefixes = sorted(set(prefixes))[:6] if prefix_bits else None
        count = len(prefixes) if prefixes else 1
        counters = ops.fingerprint_counters(DEV, count)
        for _ in range(2):                                   # the counters persist: two cases add up
            ops.fingerprint_sweep(xd, sd, counters, prefix_bits=prefix_bits, digit_bits=digit_bits, prefixes=prefixes)
        got = counters.cpu().numpy()
        for t in range(count):
            want = ref.digit_histogram(keys, prefix_bits, digit_bits, prefixes[t] if prefixes else 0)
            assert np.array_equal(got[t, :1 << digit_bits], 2 * want.astype(np.int64)), (prefix_bits, digit_bits, t)
            assert not got[t, 1 << digit_bits:].any()


def test_a_nan_in_the_foreground_names_the_case():
    from dg_tta_amd.planning.fingerprint import MemoryCases, intensity_statistics_gpu
    cases = _scenarios(np.int16)["a case without foreground between two with"]
    name, x, seg = cases[2]
    bg = x.copy()
    bg[tuple(np.argwhere(seg <= 0)[7])] = np.nan             # background: counted nowhere
    clean = _run(cases)
    assert _run([cases[0], cases[1], (name, bg, seg)]) == clean
    for bad_value in (np.nan, np.inf):
        fg = x.copy()
        fg[tuple(np.argwhere(seg > 0)[11])] = bad_value
        dev_cases = [(n_, torch.from_numpy(x_[None]).to(DEV), torch.from_numpy(s_).to(DEV)) for n_, x_, s_ in
                     [cases[0], cases[1], ("the_bad_case", fg, seg)]]
        with pytest.raises(ValueError, match="the_bad_case"):
            intensity_statistics_gpu(MemoryCases(dev_cases, DEV), 1)


def test_arguments_are_checked():
    from dg_tta_amd import ops
    x = torch.zeros(SMALL, device=DEV)
    seg = torch.ones(SMALL, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="distinct"):
        ops.fingerprint_sweep(x, seg, ops.fingerprint_counters(DEV, 2), prefix_bits=11, prefixes=[5, 5])
    with pytest.raises(ValueError, match="counters"):
        ops.fingerprint_sweep(x, seg, ops.fingerprint_counters(DEV, 2), prefix_bits=11, prefixes=[5])
    with pytest.raises(ValueError, match="seg"):
        ops.fingerprint_sweep(x, seg.to(torch.int64), ops.fingerprint_counters(DEV, 1))
    with pytest.raises(ValueError, match="state"):
        ops.fingerprint_sweep(x, seg, ops.fingerprint_counters(DEV, 1), moment=1)
    with pytest.raises(ValueError, match="ws"):
        ops.fingerprint_sweep(x, seg, ops.fingerprint_counters(DEV, 1), ws=torch.empty(16, dtype=torch.uint8, device=DEV))
    from dg_tta_amd._lib import DgttaError
    with pytest.raises(DgttaError, match="bad digits"):
        ops.fingerprint_sweep(x, seg, ops.fingerprint_counters(DEV, 1), prefix_bits=0, digit_bits=12)
    with pytest.raises(DgttaError, match="more than"):
        ops.fingerprint_sweep(x, seg, ops.fingerprint_counters(DEV, 1), prefix_bits=4, digit_bits=4, prefixes=[16])
