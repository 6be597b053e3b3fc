"""float64 numpy / scipy restatement of every stage of dg_tta_amd/pretraining/intensity.py (the intensity chain of
`dgtta pretrain --augmentation full`; kernels in csrc/intensity_aug.hip, formulas in include/dgtta.h) and the cases the CPU
and GPU tests share.  tests/test_intensity_ref.py pins it to scipy.ndimage and checks that the bounds below are tight enough
to tell a wrong parameter; tests/test_gpu_intensity.py pins the kernels to it.  The noise comes through tests/philox_ref.py.

ERROR BOUNDS of the fp32 kernels against this reference, per voxel, derived from operation counts (u = 2^-24: every fp32
operation returns its exact result times 1 + d, |d| <= u; first order in u; the GPU tests assert them on ALL voxels and print
the largest error / bound ratio).  The inputs are exact fp32 arrays and the parameters are handed to the reference as the fp32
values the descriptors hold, so neither carries an error.  The statistics (min, max exact; mean, std from double sums) reach
the kernels with a relative error of about 1e-14 (stats_bound below), four orders of magnitude below u: it is not carried
through the bounds; the one rounding of each statistic to fp32 is.

  linear     y = fl(fl(x m) + fl(s n')), n' the kernel's normal, |n' - n| <= 1e-5 (the tolerance this generator carries in
             tests/test_gpu_mind_seeded.py: fp32 log / sqrt / sincospi against float64):
                 |err| <= u (|x m| + |s n| + |y|) + 1e-5 |s|
  contrast   mean' = fl32(mean), |mean' - mean| <= u |mean|;  x - mean' (u |mean| + u |x - mean|), times f (one more
             rounding of f |x - mean|), plus mean' (u |mean| again, and the sum's rounding u |y|); the clip to the exact fp32
             min / max does not grow an error:
                 |err| <= u ((f + 1) |mean| + 2 f |x - mean| + |y|),      y before the clip
  gamma      (x - lo) carries ONE rounding (x and lo are exact fp32), r' = fl32(r) one, r' + 1e-7f one more (relative to
             r + 1e-7: 2 u), the division one: t = (x - lo) / (r + 1e-7) has 4 u RELATIVE error, whatever the cancellation
             in x - lo - the power is well conditioned in relative terms.  t^g multiplies a relative error by g: 4 g u.  powf
             is documented to 1 ulp (HIP math API); an ulp is at most 2 u relative; taken as 2 ulp: 4 u.  Times r' (its
             rounding and the product's: 2 u), plus lo (u |y|):
                 |err| <= u ((4 g + 6) t^g r + |y|)
  restore    q = sd / (sd2 + 1e-8).  x - mn2' with mn2' = fl32(mn2): u |mn2| + u |x - mn2|; divided by fl(sd2' + 1e-8f) (2 u
             relative, and the division's u), times sd' (its rounding and the product's: 2 u): q u (|mn2| + 6 |x - mn2|);
             plus mn' (u |mn| and the sum's u |y|):
                 |err| <= u (q (|mn2| + 6 |x - mn2|) + |mn| + |y|)
  blur       one pass is sum_k t'_k x_k over n = 2 radius + 1 taps, t'_k = fl32(t_k) (u), each product rounded (u), added
             in ascending k: the first sum is exact, a term passes through at most n - 1 more: (n + 1) u sum |t_k x_k| <=
             (n + 1) u M, M = max |x| of the item, because the taps are positive and sum to 1.  A later pass hands an earlier
             error on with gain sum t'_k <= 1 + u.  Three passes:
                 |err| <= 3 (2 radius + 2) u M
  stats      e = 2^-53.  A partial sum sees 16 additions in a thread, 6 + 2 in the workgroup's tree; the last workgroup
             ceil(chunks / 256) + 8 more; x - p, its square, the division by V and the final sum 4: K = 36 + ceil(chunks /
             256) roundings on a sum of magnitudes.  mean = p + S1 / V:  |err| <= K e max |x - p| + e |mean|.
             var = m2 - m1^2 with m1^2 <= m2:  |err| <= 3 K e m2 + e var;  std = sqrt(var):  |err| <= that / (2 std) + 2 e
             std.  A constant item gives x - p = 0 everywhere: mean = p and std = 0 exactly.
Nothing in these is fitted to an observed error."""
import math

import numpy as np

import philox_ref

U = 2.0 ** -24
E64 = 2.0 ** -53
EPS7 = float(np.float32(1e-7))      # the kernels' 1e-7f and 1e-8f
EPS8 = float(np.float32(1e-8))
NOISE_TOL = 1e-5
CHUNK = 4096
M32 = 0xFFFFFFFF

# the shapes of the GPU tests: lines shorter and longer than a wave, extents that are no multiple of 4 (the scalar paths), one
# that is (the 16-byte paths; (4, 4, 130) is not: W % 4 = 2), extents equal to (4) and below (3) the blur radius
SHAPES = [(5, 6, 7), (9, 70, 11), (4, 4, 130), (3, 5, 66), (4, 8, 132)]
SELECTED = (0, 2)                    # items of the 3-item batches that are named; item 1 must stay as it is
# per selected item, as fp32 values: noise scale, blur sigma (radii 2 .. 4 and the upper end), brightness, contrast, gamma
PARAMS = {
    "s": [np.float32(0.03), np.float32(0.1)],
    "sigma": [0.5, 0.7, 0.875, 1.0],
    "m": [np.float32(0.8), np.float32(1.2)],
    "f": [np.float32(0.77), np.float32(1.21)],
    "g": [np.float32(0.72), np.float32(1.45)],
}
KEYS = [0x0123456789ABCDEF, 0xFEDCBA9876543210]
REL_OFF = 1e-3                       # the sensitivity tests move a parameter by this much


def make_batch(shape, seed=0):
    """[3, 1, D, H, W] float32: normalised-CT-like values, each item with a scale and an offset of its own."""
    rs = np.random.RandomState(1000 + seed + sum(shape))
    x = rs.standard_normal((3, 1, *shape))
    x = x * np.array([1.0, 0.3, 2.5]).reshape(3, 1, 1, 1, 1) + np.array([0.2, -1.0, 1.5]).reshape(3, 1, 1, 1, 1)
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------ stages
def noise_field(key, b, voxels, offset=0):
    """n(v), v = 0 .. voxels - 1, of item index b under the 64-bit key: normal v & 3 of Philox call v >> 2."""
    key, offset = int(key) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    calls = np.arange((voxels + 3) // 4, dtype=np.uint64)
    words = philox_ref.philox4x32_10(calls, int(b), offset & M32, offset >> 32, key & M32, key >> 32)
    return np.stack(philox_ref.normals(words), axis=1).reshape(-1)[:voxels]


def linear(x, m=1.0, s=0.0, n=None):
    x = np.asarray(x, dtype=np.float64)
    return x * float(m) if s == 0.0 else x * float(m) + float(s) * n.reshape(x.shape)


def linear_bound(x, m, s, n):
    x = np.asarray(x, dtype=np.float64)
    if s == 0.0:
        return U * np.abs(x * float(m))
    n = n.reshape(x.shape)
    return U * (np.abs(x * float(m)) + np.abs(float(s) * n) + np.abs(linear(x, m, s, n))) + NOISE_TOL * abs(float(s))


def gauss_taps(sigma):
    """(radius, float64 taps) of scipy.ndimage.gaussian_filter(sigma, truncate=4)."""
    radius = int(4.0 * float(sigma) + 0.5)
    xs = np.arange(-radius, radius + 1, dtype=np.float64)
    t = np.exp(-0.5 / (float(sigma) ** 2) * xs ** 2)
    return radius, t / t.sum()


def reflect_index(j, n):
    """scipy's mode="reflect" (d c b a | a b c d | d c b a): j mod 2n, mirrored when >= n."""
    j = np.mod(j, 2 * n)
    return np.where(j >= n, 2 * n - 1 - j, j)


def blur(x, sigma):
    """Explicit taps on reflected indices, axis after axis."""
    out = np.asarray(x, dtype=np.float64)
    radius, taps = gauss_taps(sigma)
    for axis in range(out.ndim):
        n = out.shape[axis]
        src = np.moveaxis(out, axis, 0)
        acc = np.zeros_like(src)
        for k, t in enumerate(taps):
            acc = acc + t * src[reflect_index(np.arange(n) + k - radius, n)]
        out = np.moveaxis(acc, 0, axis)
    return out


def blur_bound(x, sigma):
    radius = gauss_taps(sigma)[0]
    return 3.0 * (2 * radius + 2) * U * float(np.abs(np.asarray(x, dtype=np.float64)).max())


def stats(x):
    """(min, max, mean, population std), the sums exact (math.fsum)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    mean = math.fsum(x) / x.size
    var = math.fsum((x - mean) ** 2) / x.size
    return float(x.min()), float(x.max()), mean, math.sqrt(var)


def stats_bound(x):
    """(bound of the mean, bound of the std)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    chunks = (x.size + CHUNK - 1) // CHUNK
    k = 36 + (chunks + 255) // 256
    _, _, mean, std = stats(x)
    d = x - x[0]
    m2 = math.fsum(d * d) / x.size
    b_mean = k * E64 * float(np.abs(d).max()) + E64 * abs(mean)
    b_std = 0.0 if std == 0.0 else (3 * k * E64 * m2 + E64 * std * std) / (2 * std) + 2 * E64 * std
    return b_mean, b_std


def contrast(x, f, clip=True):
    x = np.asarray(x, dtype=np.float64)
    lo, hi, mean, _ = stats(x)
    y = (x - mean) * float(f) + mean
    return np.clip(y, lo, hi) if clip else y


def contrast_bound(x, f):
    x = np.asarray(x, dtype=np.float64)
    mean = stats(x)[2]
    return U * ((float(f) + 1.0) * abs(mean) + 2.0 * float(f) * np.abs(x - mean) + np.abs(contrast(x, f, clip=False)))


def gamma_power(x, g, negate=False):
    """((x - lo) / (r + 1e-7))^g r + lo of x, or of -x (left negated: its statistics are the next step's)."""
    x = np.asarray(x, dtype=np.float64)
    x = -x if negate else x
    lo, hi = float(x.min()), float(x.max())
    r = hi - lo
    return ((x - lo) / (r + EPS7)) ** float(g) * r + lo


def gamma_power_bound(x, g, negate=False):
    x = np.asarray(x, dtype=np.float64)
    x = -x if negate else x
    lo = float(x.min())
    y = gamma_power(x, g)
    return U * ((4.0 * float(g) + 6.0) * np.abs(y - lo) + np.abs(y))


def restore(y, before, after, negate=False, eps8=EPS8):
    """(y - mn2) / (sd2 + 1e-8) sd + mn with before = stats of the item the power was applied to, after = stats of y; negate:
    `before` are the statistics of the item BEFORE it was negated - the mean changes sign - and the result is negated back.
    The guard 1e-8 makes the result's std sd sd2 / (sd2 + 1e-8), not sd: eps8 = 0 is the formula without it."""
    y = np.asarray(y, dtype=np.float64)
    mn, sd, mn2, sd2 = (-before[2] if negate else before[2]), before[3], after[2], after[3]
    z = (y - mn2) / (sd2 + eps8) * sd + mn
    return -z if negate else z


def restore_bound(y, before, after, negate=False):
    y = np.asarray(y, dtype=np.float64)
    mn, sd, mn2, sd2 = before[2], before[3], after[2], after[3]
    q = sd / (sd2 + EPS8)
    return U * (q * (abs(mn2) + 6.0 * np.abs(y - mn2)) + abs(mn) + np.abs(restore(y, before, after, negate)))


def gamma(x, g, inverted=False, eps8=EPS8):
    """Stage 7, or stage 6 (x = -x, stage 7, x = -x), in one piece."""
    x = np.asarray(x, dtype=np.float64)
    x = -x if inverted else x
    y = gamma_power(x, g)
    z = restore(y, stats(x), stats(y), eps8=eps8)
    return -z if inverted else z


def low_resolution(x, zoom, thin=None):
    """Stage 5: skimage.transform.resize(mode="edge", anti_aliasing=False) down with order 0 and back with order 3, restated
    as scipy.ndimage.zoom(mode="nearest", grid_mode=True) + the clip to the input range (scikit-image is not a dependency)."""
    from scipy import ndimage
    x = np.asarray(x, dtype=np.float64)
    target = [max(int(t), 1) for t in np.round(np.asarray(x.shape, dtype=np.float64) * float(zoom))]
    if thin is not None:
        target[thin] = x.shape[thin]

    def resize(v, shape, order):
        out = ndimage.zoom(v, [t / s for t, s in zip(shape, v.shape)], order=order, mode="nearest", grid_mode=True)
        return np.clip(out, v.min(), v.max()) if order else out
    return resize(resize(x, target, 0), x.shape, 3)
