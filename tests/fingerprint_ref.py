"""numpy restatement of the dataset-fingerprint kernels (dg_tta_amd/csrc/fingerprint.hip): the order-preserving key of a float32,
the three-level (11 + 11 + 10 bit) radix select from digit histograms, and the moments in float64.  Written without the
package: tests/test_fingerprint_ref.py checks it against np.sort / np.percentile, tests/test_gpu_fingerprint.py checks the
kernels against it."""
import math

import numpy as np

DIGITS = (11, 11, 10)
QUANTILES = (0.5, 50.0, 99.5)


def key_of(x):
    """uint32 keys whose unsigned order is the order of the float32 values (-0.0 before +0.0)."""
    u = np.ascontiguousarray(x, dtype=np.float32).reshape(-1).view(np.uint32)
    neg = (u >> np.uint32(31)).astype(bool)
    return np.where(neg, ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def value_of(key):
    key = np.uint32(key)
    u = key ^ np.uint32(0x80000000) if key >> np.uint32(31) else ~key
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def digit_histogram(keys, prefix_bits, digit_bits, prefix):
    """Counts of the digit (the digit_bits bits after the leading prefix_bits) of the keys that start with `prefix`."""
    keys = keys.astype(np.uint64)
    if prefix_bits:
        keys = keys[(keys >> np.uint64(32 - prefix_bits)) == np.uint64(prefix)]
    digit = (keys >> np.uint64(32 - prefix_bits - digit_bits)) & np.uint64((1 << digit_bits) - 1)
    return np.bincount(digit.astype(np.int64), minlength=1 << digit_bits).astype(np.uint64)


def radix_select(x, rank, digits=DIGITS):
    """The value of 0-based rank `rank` among the float32 values x, digit by digit from histograms alone."""
    keys = key_of(x)
    prefix, bits, residual = 0, 0, int(rank)
    for d in digits:
        hist = digit_histogram(keys, bits, d, prefix)
        cum = np.cumsum(hist)
        digit = int(np.searchsorted(cum, residual, side="right"))
        residual -= int(cum[digit - 1]) if digit else 0
        prefix, bits = (prefix << d) | digit, bits + d
    assert bits == 32
    return value_of(prefix)


def quantile_ranks(n, quantiles=QUANTILES):
    out = []
    for q in quantiles:
        pos = (q / 100.0) * (n - 1)
        lo = int(math.floor(pos))
        out.append((lo, min(lo + 1, n - 1), pos - lo))
    return out


def percentiles(x, quantiles=QUANTILES):
    """[(lower order statistic, upper order statistic, percentile)] per quantile: lo + (hi - lo) * frac in float64."""
    out = []
    for lo, hi, frac in quantile_ranks(np.size(x), quantiles):
        a, b = radix_select(x, lo), radix_select(x, hi)
        out.append((a, b, float(a) + (float(b) - float(a)) * frac))
    return out


def moments(x):
    """count, min, max, mean and population std of float32 values, sums in float64, the second centred on the mean."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    x64 = x.astype(np.float64)
    mean = float(x64.sum()) / x.size
    return {"count": int(x.size), "min": float(x.min()), "max": float(x.max()), "mean": mean,
            "std": math.sqrt(float(((x64 - mean) ** 2).sum()) / x.size)}


def fingerprint_block(x):
    """The channel's block of dataset_fingerprint.json for the pooled foreground values x."""
    m = moments(x)
    p = percentiles(x)
    return {"max": m["max"], "mean": m["mean"], "median": p[1][2], "min": m["min"], "percentile_00_5": p[0][2],
            "percentile_99_5": p[2][2], "std": m["std"]}


# ------------------------------------------------------------------------------------------------ rounding bounds of the moments
U = 2.0 ** -53


def kernel_summation_depth(voxel_counts):
    """The largest number of double additions between one value and the final sum in csrc/fingerprint.hip, for cases of these
    voxel counts: a workgroup walks steps of 4096 voxels, at most 512 workgroups per case; a thread adds its at most 16 values
    of a step one after the other (16 * steps), 6 shuffle levels add the 64 lanes, 3 additions the four waves, one thread adds
    the workgroups' partials in order (workgroups), and every case is added to the running sum (cases)."""
    depth = 0
    for v in voxel_counts:
        chunks = -(-int(v) // 4096)
        workgroups = max(min(chunks, 512), 1)
        steps = -(-chunks // workgroups)
        depth = max(depth, 16 * steps + 6 + 3 + workgroups)
    return depth + len(voxel_counts)


def numpy_summation_depth(n):
    """The same for numpy's pairwise float64 sum: blocks of 128 values in 8 accumulators (16 + 3 additions), then a binary tree."""
    return 19 + max(int(math.ceil(math.log2(max(n, 1) / 128.0))), 0) + 1


def moment_bounds(x, voxel_counts):
    """(mean bound, std bound): how far the kernels' mean and std of the pooled float32 values x may lie from numpy's float64
    x.mean() and x.std(), from the operation counts of BOTH evaluations (first order in u = 2^-53, D = the summation depths):
      a sum of n values through a tree of depth D is within D u sum|x| of the exact sum; the division by n rounds once more:
          |mean_k - mean_np| <= (D_k + D_np + 2) u mean|x|
      a term (x - m)^2 carries 3 u (one rounding of the difference, doubled by the square, one of the square), the sum of these
      non-negative terms D u more, the division 1 u; the square root halves the relative error and rounds once:
          |std_k - std_np| <= ((D_k + D_np) / 2 + 6) u std + e,
      e = the effect of centring on a mean that is off by d <= the mean bound: sqrt(var + d^2) - sqrt(var) <= d^2 / (2 std), d
      when std = 0.
    No figure measured on the kernels enters."""
    x64 = np.asarray(x, dtype=np.float64)
    n = x64.size
    depth = kernel_summation_depth(voxel_counts) + numpy_summation_depth(n)
    mean_bound = (depth + 2) * U * float(np.abs(x64).mean())
    std = float(x64.std())
    centring = mean_bound if std == 0.0 else mean_bound ** 2 / (2 * std)
    return mean_bound, (depth / 2 + 6) * U * std + centring
