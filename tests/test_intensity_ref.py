"""Host tests of tests/intensity_ref.py, the float64 restatement the GPU tests of csrc/intensity_aug.hip compare against: it is
pinned to scipy.ndimage where scipy has the operation, its invariants hold, and the error bounds its docstring derives are
tight enough to tell a parameter that is off by 1e-3 on the very inputs the GPU tests use."""
import numpy as np
import pytest
from scipy import ndimage

import intensity_ref as iref


@pytest.mark.parametrize("sigma, radius", [(0.5, 2), (0.7, 3), (0.875, 4), (1.0, 4)])
def test_explicit_taps_on_reflected_indices_are_scipys_gaussian_filter(sigma, radius):
    assert iref.gauss_taps(sigma)[0] == radius and len(iref.gauss_taps(sigma)[1]) == 2 * radius + 1
    for shape in [(3, 5, 66), (4, 4, 13), (9, 7, 11), (3, 3, 3), (1, 2, 5)]:      # extents below the radius too
        x = np.random.RandomState(sum(shape)).standard_normal(shape)
        ref = ndimage.gaussian_filter(x, sigma, order=0, mode="reflect", truncate=4.0)
        assert np.abs(iref.blur(x, sigma) - ref).max() <= 1e-14, (sigma, shape)


def test_the_products_taps_are_the_references_taps_rounded_once():
    from dg_tta_amd.ops import gauss_blur_taps
    for sigma in iref.PARAMS["sigma"] + [0.51234, 0.999]:
        radius, taps = gauss_blur_taps(sigma)
        r, t = iref.gauss_taps(sigma)
        assert radius == r and taps.dtype == np.float32 and np.array_equal(taps, t.astype(np.float32))
    for bad in (0.0, -0.5, 1.0001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            gauss_blur_taps(bad)


@pytest.mark.parametrize("inverted", [False, True])
def test_gamma_with_restore_keeps_mean_and_std(inverted):
    for shape in iref.SHAPES:
        x = iref.make_batch(shape)[0, 0]
        for g in (0.7, 0.72, 1.0, 1.45, 1.5):
            a = iref.stats(x)
            b = iref.stats(iref.gamma(x, g, inverted, eps8=0.0))                   # the formula without its 1e-8 guard
            assert abs(a[2] - b[2]) <= 1e-12 and abs(a[3] - b[3]) <= 1e-12, (shape, g)
            # with the guard the std is sd sd2 / (sd2 + 1e-8) by the definition itself - 1e-8 relative below sd - and the
            # stage keeps exactly that, and the mean, to 1e-12
            y = iref.gamma_power(x, g, negate=inverted)
            sd2 = iref.stats(y)[3]
            c = iref.stats(iref.gamma(x, g, inverted))
            assert abs(a[2] - c[2]) <= 1e-12 and abs(a[3] * sd2 / (sd2 + iref.EPS8) - c[3]) <= 1e-12, (shape, g)
    # the two-step form the kernels run (power, statistics, restore) is the one-piece stage
    x = iref.make_batch((5, 6, 7))[2, 0]
    y = iref.gamma_power(x, 1.3, negate=inverted)
    assert np.array_equal(iref.restore(y, iref.stats(x), iref.stats(y), negate=inverted), iref.gamma(x, 1.3, inverted))


def test_contrast_stays_inside_the_items_range():
    for shape in iref.SHAPES:
        x = iref.make_batch(shape)[2, 0].astype(np.float64)
        for f in (0.75, 0.77, 1.21, 1.25):
            y = iref.contrast(x, f)
            assert y.min() >= x.min() and y.max() <= x.max()
        assert (iref.contrast(x, 1.25) == x.max()).any() and (iref.contrast(x, 1.25) == x.min()).any()      # it does clip
        assert np.array_equal(iref.contrast(x, 1.0, clip=False), (x - iref.stats(x)[2]) + iref.stats(x)[2])


def test_a_constant_item_stays_finite():
    x = np.full((3, 4, 5), np.float32(-1.75), dtype=np.float32)
    assert iref.stats(x) == (-1.75, -1.75, -1.75, 0.0) and iref.stats_bound(x)[1] == 0.0
    for out in (iref.contrast(x, 1.2), iref.gamma(x, 0.8), iref.gamma(x, 1.4, inverted=True), iref.gamma_power(x, 1.4, negate=True)):
        assert np.isfinite(out).all()
    assert np.array_equal(iref.contrast(x, 1.2), x) and np.array_equal(iref.gamma(x, 0.8), x)
    assert np.array_equal(iref.gamma(x, 1.4, inverted=True), x)


def test_noise_is_a_function_of_key_item_and_voxel():
    import philox_ref
    a = iref.noise_field(iref.KEYS[0], 2, 103)
    assert a.shape == (103,) and np.array_equal(a, iref.noise_field(iref.KEYS[0], 2, 103))
    assert not np.array_equal(a, iref.noise_field(iref.KEYS[1], 2, 103)) and not np.array_equal(a, iref.noise_field(iref.KEYS[0], 1, 103))
    assert np.array_equal(a[:50], iref.noise_field(iref.KEYS[0], 2, 50))               # no dependence on the extent
    # voxel v is normal v & 3 of Philox call v >> 2 with counter (v >> 2, b, 0, 0)
    k = iref.KEYS[0]
    words = philox_ref.philox4x32_10(np.uint64(25), 2, 0, 0, k & 0xFFFFFFFF, k >> 32)
    assert [float(a[100 + i]) for i in range(3)] == [float(n) for n in philox_ref.normals(words)[:3]]
    big = iref.noise_field(5, 0, 40000)
    assert abs(big.mean()) < 5 / np.sqrt(40000) and abs(big.std() - 1.0) < 0.02


def test_low_resolution_keeps_shape_range_and_the_thin_axis():
    x = iref.make_batch((6, 20, 22))[0, 0]
    y = iref.low_resolution(x, 0.5)
    assert y.shape == x.shape and y.min() >= x.min() and y.max() <= x.max() and not np.array_equal(y, x)
    assert np.abs(iref.low_resolution(x, 1.0) - x).max() <= 1e-12                   # zoom 1: the cubic spline interpolates
    const_d = np.repeat(iref.make_batch((1, 20, 22))[0, 0], 6, axis=0)             # constant along D: thin = 0 keeps it so
    z = iref.low_resolution(const_d, 0.6, thin=0)
    assert np.abs(z - z[:1]).max() <= 1e-12 and np.abs(z - const_d).max() > 1e-3


# ------------------------------------------------------------------------------------------------ sensitivity
def _leaves(err, bound):
    return bool(np.any(err > bound))


@pytest.mark.parametrize("shape", iref.SHAPES)
def test_a_parameter_off_by_1e_3_leaves_every_bound(shape):
    """A loose bound cannot hide a wrong kernel: on the inputs of the GPU tests, the reference evaluated with s, sigma, m, f
    or g off by 1e-3 (relative) differs from itself by more than the derived bound on at least one voxel."""
    batch = iref.make_batch(shape)
    off = 1.0 + iref.REL_OFF
    for k, item in enumerate(iref.SELECTED):
        x = batch[item, 0]
        n = iref.noise_field(iref.KEYS[k], item, x.size)
        s, m, f, g = (float(iref.PARAMS[p][k]) for p in ("s", "m", "f", "g"))
        assert _leaves(np.abs(iref.linear(x, 1.0, s * off, n) - iref.linear(x, 1.0, s, n)), iref.linear_bound(x, 1.0, s, n))
        assert _leaves(np.abs(iref.linear(x, m * off) - iref.linear(x, m)), iref.linear_bound(x, m, 0.0, None))
        assert _leaves(np.abs(iref.contrast(x, f * off) - iref.contrast(x, f)), iref.contrast_bound(x, f))
        for negate in (False, True):
            assert _leaves(np.abs(iref.gamma_power(x, g * off, negate) - iref.gamma_power(x, g, negate)), iref.gamma_power_bound(x, g, negate))
            # restore has no drawn parameter of its own: g reaches it through the power's output and statistics
            y, y_off = iref.gamma_power(x, g, negate), iref.gamma_power(x, g * off, negate)
            z = iref.restore(y, iref.stats(x), iref.stats(y), negate)
            z_off = iref.restore(y_off, iref.stats(x), iref.stats(y_off), negate)
            assert _leaves(np.abs(z_off - z), iref.restore_bound(y, iref.stats(x), iref.stats(y), negate))
        for sigma in iref.PARAMS["sigma"]:
            assert _leaves(np.abs(iref.blur(x, sigma * off) - iref.blur(x, sigma)), iref.blur_bound(x, sigma))
