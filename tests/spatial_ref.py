"""float64 restatement of csrc/spatial_aug.hip (the sampler of `dgtta pretrain --augmentation spatial`) and the cases the
CPU and GPU tests share.  tests/test_spatial_ref.py pins it to scipy.ndimage; tests/test_gpu_spatial.py pins the kernels to it.

ERROR BOUND of the fp32 kernels against this reference, derived from operation counts (u = 2^-24, first order in u; the GPU
test asserts it and prints the largest error / bound ratio).  For an image voxel inside the volume

    |gpu - ref| <= K_SUM[order] u (S + E_pre) + E_pre + 6 u T,    E_pre = K_PRE u M for order 3, 0 for order 1

  * S = sum |w c| over the voxel's taps (w: the separable tap weights, c: the reference's coefficients), T = max |c| over
    the taps, M = max |volume|.
  * K_SUM: every term w_d w_h w_w c of the kernel's sum carries the relative errors of its three 1-D weights and of the
    roundings it passes through.  Order 3, weights written as in bspline3_weights: the outer two are cubes, t^3 / 6 (3
    roundings) and u^3 / 6 with u = 1 - t (6); the inner two are (q + 4) / 6 with q = 3 t^2 (t - 2) in [-3, 0]: 4 roundings
    of q (absolute 12 u), the sum in [1, 4] (4 u more), the division: 17 u relative to a weight >= 1 / 6; with u = 1 - t in
    place of t, |dq/du| <= 4 adds 4 u before the sum and the same steps give 25 u.  So 25 u per weight at most, 75 u for three.
    The nested sums (w innermost) cost a term one product and at most three additions per level (the first addition, to
    zero, is exact): 12 roundings.  75 + 12 = 87 -> K_SUM[3] = 88.  Order 1: weights 1 - t (one rounding) and t (none), 3 u;
    one product and one addition per level, 6: K_SUM[1] = 10.
  * K_PRE: one axis of the prefilter on a line with |x| <= m, r = |pole| = 0.26795.  Causal y[k] = 6 x[k] + z y[k-1]:
    |y| <= Y = 6 m / (1 - r) = 8.2 m; a step rounds 6 x (6 m u), z y (r Y u), the sum (Y u), and the fp32 pole is off by a
    factor 1 + u (r Y u): 18.6 m u per step, accumulated with sum r^k = 1.366: 25.4 m u.  The mirror initialisation is a sum
    of terms r^i 6 x that have each seen at most i + 3 roundings: 6 m u (r / (1 - r)^2 + 3 / (1 - r)) = 27.6 m u, decaying
    with r^k; its terms beyond 64 are below 1e-36.  Causal error <= 28 m u.  Anticausal c[k] = z (c[k+1] - y[k]): |c| <= 3 m
    (the filter's infinity norm is 6 r / (1 - r)^2 = 3), the difference is c[k] / z, <= 11.2 m; its rounding times r, the
    product's rounding and the pole's error give 9 m u per step, the causal error enters as r 28 m u = 7.5 m u; accumulated
    with 1.366: 22.5 m u.  Its initialisation (z y[n-2] + y[n-1]) z / (z^2 - 1) passes the causal error with r / (1 - r) =
    0.366 (10.2 m u) plus five roundings of a value <= 3 m: 25.2 m u, decaying.  One axis: <= 26 m u.  Three axes: every later
    axis multiplies the error it is handed and the magnitude it works on by at most 3: 26 u M (9 + 3 * 3 + 9) = 702 u M.
    The sampler then mixes coefficient errors with weights that sum to 1: E_pre = 702 u M.
  * the position x is evaluated in double from the fp32 map (error 1e-14); its fractional part is rounded to fp32 once
    (<= 2^-25).  Taken as 2^-24 per axis, times the spline's derivative bound sum |w'| max |c| <= 2 T per axis: 6 u T.
Nothing in it is fitted to an observed error."""
import numpy as np

POLE = np.sqrt(3.0) - 2.0
U = 2.0 ** -24
K_SUM = {3: 88.0, 1: 10.0}
K_PRE = 702.0


def error_bound(order, s, t, m):
    e_pre = K_PRE * U * m if order == 3 else 0.0
    return K_SUM[order] * U * (s + e_pre) + e_pre + 6.0 * U * t


# ------------------------------------------------------------------------------------------------ prefilter
def prefilter_axis(x, axis):
    """scipy's spline_filter1d(order=3, mode="mirror") along one axis, in float64 (ni_splines.c)."""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0).copy()
    n = x.shape[0]
    if n == 1:
        return np.moveaxis(x, 0, axis)
    z = POLE
    c = x * 6.0
    z_n_1 = z ** (n - 1)
    c0 = c[0] + z_n_1 * c[n - 1]
    z_i = z
    for i in range(1, n - 1):
        c0 = c0 + z_i * (c[i] + z_n_1 * c[n - 1 - i])
        z_i *= z
    c[0] = c0 / (1.0 - z_n_1 * z_n_1)
    for k in range(1, n):
        c[k] += z * c[k - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1.0)
    for k in range(n - 2, -1, -1):
        c[k] = z * (c[k + 1] - c[k])
    return np.moveaxis(c, 0, axis)


def prefilter(vol):
    out = np.asarray(vol, dtype=np.float64)
    for a in range(out.ndim):
        out = prefilter_axis(out, a)
    return out


# ------------------------------------------------------------------------------------------------ sampler
def mirror_index(idx, n):
    """scipy's tap index on a mirrored line (ni_interpolation.c, every mode but grid-constant), any integer."""
    idx = np.asarray(idx, dtype=np.int64)
    if n <= 1:
        return np.zeros_like(idx)
    s2 = 2 * n - 2
    m = np.mod(idx, s2)
    return np.where(m >= n, s2 - m, m)


def bspline3_weights(t):
    u = 1.0 - t
    w0 = u * u * u / 6.0
    w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0
    return np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2])


def coordinates(map34, patch):
    """x [3, PD, PH, PW] = A v + t in float64 from the map AS THE KERNEL GETS IT (rounded to fp32)."""
    m = np.asarray(map34, dtype=np.float32).astype(np.float64).reshape(3, 4)
    v = np.stack(np.meshgrid(*[np.arange(p, dtype=np.float64) for p in patch], indexing="ij"))
    return np.tensordot(m[:, :3], v, axes=1) + m[:, 3].reshape(3, 1, 1, 1)


def sample_image(src, map34, patch, order):
    """map_coordinates(order, mode="constant", cval=0) of `src` (order 3: the COEFFICIENTS) at coordinates(map34, patch).
    Returns (value, S = sum |w c|, T = max |c| over the taps, inside mask, distance of x to the nearest face)."""
    src = np.asarray(src, dtype=np.float64)
    x = coordinates(map34, patch)
    shape = np.array(src.shape, dtype=np.float64).reshape(3, 1, 1, 1)
    inside = np.all((x >= 0.0) & (x <= shape - 1.0), axis=0)
    face = np.min(np.minimum(np.abs(x), np.abs(x - (shape - 1.0))), axis=0)
    xc = np.where(inside[None], x, 0.0)
    fl = np.floor(xc)
    t = xc - fl
    nt = order + 1
    idx, wts = [], []
    for a in range(3):
        start = fl[a].astype(np.int64) - (1 if order == 3 else 0)
        idx.append([mirror_index(start + k, src.shape[a]) for k in range(nt)])
        wts.append(bspline3_weights(t[a]) if order == 3 else np.stack([1.0 - t[a], t[a]]))
    val, s, tmax = np.zeros(x.shape[1:]), np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
    for i in range(nt):
        for j in range(nt):
            for k in range(nt):
                c = src[idx[0][i], idx[1][j], idx[2][k]]
                w = wts[0][i] * wts[1][j] * wts[2][k]
                val += w * c
                s += np.abs(w * c)
                tmax = np.maximum(tmax, np.abs(c))
    return np.where(inside, val, 0.0), s, tmax, inside, face


def sample_labels(lab, map34, patch):
    """nnU-Net's order_seg=1 rule from the 8 trilinear corners: corners outside the volume carry label 0, mass(l) = sum of
    the weights of the corners that carry l, result = the largest l > 0 with mass >= 0.5, else 0.
    Returns (labels int64, near = a mass of a label > 0 lies within 1e-5 of 0.5, all 8 corners agree)."""
    lab = np.asarray(lab).astype(np.int64)
    x = coordinates(map34, patch)
    fl = np.floor(x)
    t = x - fl
    cl, cw = [], []
    for i in range(2):
        for j in range(2):
            for k in range(2):
                w, ok, ix = 1.0, True, []
                for a, o in enumerate((i, j, k)):
                    p = fl[a].astype(np.int64) + o
                    ok = ok & (p >= 0) & (p < lab.shape[a])
                    ix.append(np.clip(p, 0, lab.shape[a] - 1))
                    w = w * (t[a] if o else 1.0 - t[a])
                cl.append(np.where(ok, lab[ix[0], ix[1], ix[2]], 0))
                cw.append(w)
    best = np.zeros(x.shape[1:], dtype=np.int64)
    near = np.zeros(x.shape[1:], dtype=bool)
    for c in range(8):
        mass = sum(np.where(cl[e] == cl[c], cw[e], 0.0) for e in range(8))
        fg = cl[c] > 0
        near |= fg & (np.abs(mass - 0.5) <= 1e-5)
        best = np.where(fg & (mass >= 0.5) & (cl[c] > best), cl[c], best)
    agree = np.all(np.stack(cl) == cl[0][None], axis=0)
    return best, near, agree


def integer_crop(vol, map34, patch, fill=0):
    """out[v] = vol[A v + t] for a map whose coordinates are all integers (identity, signed permutations), `fill` outside:
    plain integer indexing, independent of the samplers above."""
    x = coordinates(map34, patch)
    xi = np.rint(x).astype(np.int64)
    assert np.array_equal(xi.astype(np.float64), x)
    ok = np.ones(x.shape[1:], dtype=bool)
    ix = []
    for a in range(3):
        ok &= (xi[a] >= 0) & (xi[a] < vol.shape[a])
        ix.append(np.clip(xi[a], 0, vol.shape[a] - 1))
    return np.where(ok, vol[ix[0], ix[1], ix[2]], fill)


# ------------------------------------------------------------------------------------------------ shared cases
SHAPES = [(20, 18, 22), (14, 25, 9), (8, 30, 30)]          # the third is smaller than the patch in D
PATCH = (12, 10, 18)
PREFILTER_SHAPES = [(5, 6, 7), (9, 70, 11)]


def make_case(shape, seed):
    """(image float32 ~ N(0, 1) on a smooth field, label map float32 with values 0..4 in smooth regions)."""
    rs = np.random.RandomState(seed)
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    field = sum(np.sin(g[a] * f + p) for a, f, p in zip((0, 1, 2, 0, 1, 2), rs.uniform(0.2, 0.7, 6), rs.uniform(0, 6.28, 6)))
    img = (0.5 * field + rs.standard_normal(shape)).astype(np.float32)
    lab = np.clip(np.floor((field + 3.0) * (5.0 / 6.0)), 0, 4).astype(np.float32)
    return img, lab


def _rot(deg):
    from dg_tta_amd.pretraining.spatial import rotation_matrix
    return rotation_matrix(*np.radians(deg))


# name -> (A, shift added to t, all coordinates are exact integers)
MAP_TABLE = [
    ("identity", np.eye(3), (0.0, 0.0, 0.0), True),
    ("signed permutation", np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (0.0, 0.0, 0.0), True),
    ("rotation 17 -23 9", _rot((17.0, -23.0, 9.0)), (0.0, 0.0, 0.0), False),
    ("scale 0.73 with rotation", 0.73 * _rot((-11.0, 6.0, 28.0)), (0.0, 0.0, 0.0), False),
    ("scale 1.37", 1.37 * np.eye(3), (0.0, 0.0, 0.0), False),
    ("outside on two faces", _rot((4.0, -3.0, 5.0)), (-3.3, 0.0, 4.6), False),
]


def table_map(row, shape, item):
    """The 3 x 4 fp32 map of table row `row` for the volume `shape`: the patch centred on a voxel that depends on the item."""
    from dg_tta_amd.pretraining.spatial import patch_start, sampling_map
    _, a, shift, _ = MAP_TABLE[row]
    center = [n // 2 + (item - 1) * 2 for n in shape]
    m = sampling_map(a, patch_start(center, shape, PATCH), PATCH).astype(np.float64)
    m[:, 3] += np.asarray(shift)
    return m.astype(np.float32)
