"""float64 reference of the surface-distance metrics (test infrastructure, numpy only): the surface of a mask, the brute-force
squared distance to a set of sites, and HD95 / HD / ASSD / NSD as dg_tta_amd/tta/evaluation.py defines them.  Every input of the
tests is small enough for O(voxels x sites).  tests/test_surface_ref.py licenses it against scipy.ndimage; the GPU tests
(tests/test_gpu_surface.py) compare the kernels with it and import no scipy."""
import functools

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32

# (D, H, W) of the distance-transform cases: each axis in turn past a wave (64), past 128 and past a 256-thread workgroup; then
# the paths of csrc/surface.hip those do not reach: the largest axis the library takes (1024) on every axis - the 16-line LDS
# tile of the H / D passes, and in the W pass 3 lines per tile with a partial last tile - and the 32-line tile, chosen by the
# lines there are (3, 4, 20) and by the axis length (260, 1, 17)
EDT_SHAPES = [(1, 1, 1), (5, 7, 70), (33, 9, 6), (2, 130, 3), (300, 2, 3), (2, 300, 3), (3, 2, 300), (11, 13, 17),
              (1024, 1, 2), (2, 1024, 1), (1, 5, 1024), (3, 4, 20), (260, 1, 17)]
EDT_SITES = ["corner", "all", "none", "random0.02", "random0.3"]
SPACINGS = [(1.0, 1.0, 1.0), (3.0, 0.75, 1.25), (0.7, 0.9766, 5.0)]


def site_mask(shape, kind):
    """The named site set on `shape` (bool); random masks come from a fixed seed per shape and density."""
    m = np.zeros(shape, dtype=bool)
    if kind == "corner":
        m[-1, 0, -1] = True
    elif kind == "all":
        m[:] = True
    elif kind.startswith("random"):
        dens = float(kind[len("random"):])
        rng = np.random.default_rng([int(1e4 * dens), *shape])
        m = rng.random(shape) < dens
    elif kind != "none":
        raise ValueError(kind)
    return m


def surface(mask):
    """S(M): voxels of M with at least one of the six face neighbours outside M; outside the volume counts as outside."""
    m = np.pad(np.asarray(mask, dtype=bool), 1, constant_values=False)
    c = m[1:-1, 1:-1, 1:-1]
    inner = (m[:-2, 1:-1, 1:-1] & m[2:, 1:-1, 1:-1] & m[1:-1, :-2, 1:-1] & m[1:-1, 2:, 1:-1] & m[1:-1, 1:-1, :-2] & m[1:-1, 1:-1, 2:])
    return c & ~inner


def f32_spacing(spacing):
    """The spacing as the kernel receives it: rounded to fp32, then promoted to float64."""
    return np.asarray(spacing, dtype=np.float32).astype(np.float64)


def edt_sq(site, spacing=(1.0, 1.0, 1.0)):
    """float64 [D,H,W]: squared physical distance from every voxel to the nearest True voxel of `site`, +inf without one.
    Brute force over all pairs, in chunks of voxels."""
    site = np.asarray(site, dtype=bool)
    s = f32_spacing(spacing)
    pts = np.argwhere(site).astype(np.float64) * s                          # [S,3]
    vox = np.indices(site.shape).reshape(3, -1).T.astype(np.float64) * s     # [V,3]
    out = np.full(vox.shape[0], np.inf)
    if len(pts):
        step = max(1, (1 << 22) // len(pts))
        for v0 in range(0, vox.shape[0], step):
            d = vox[v0:v0 + step, None, :] - pts[None, :, :]
            out[v0:v0 + step] = (d[..., 0] ** 2 + d[..., 1] ** 2 + d[..., 2] ** 2).min(1)
    return out.reshape(site.shape)


def edt_sq_int(site):
    """Unit spacing: the exact integer squared distances as fp32 (every value is an integer below 2^24), +inf without a site."""
    d = edt_sq(site)
    assert np.all(d[np.isfinite(d)] < 2 ** 24)
    return d.astype(np.float32)


def directed_distances(surf_from, surf_to, spacing):
    """For every voxel of surf_from: the physical distance to the nearest voxel of surf_to (float64, unsorted)."""
    return np.sqrt(edt_sq(surf_to, spacing))[surf_from]


def label_distances(pred, ref, label, spacing):
    """(d_rp, d_pr) of one label, or None when the label is absent from one of the maps."""
    sp, sr = surface(pred == label), surface(ref == label)
    if not sp.any() or not sr.any():
        return None
    return directed_distances(sr, sp, spacing), directed_distances(sp, sr, spacing)


def metrics(pred, ref, label, spacing=(1.0, 1.0, 1.0), tau=1.0):
    """{HD95, HD, ASSD, NSD} of one label: NaN when it is in neither map; inf, inf, inf, 0 when it is in exactly one."""
    in_p, in_r = bool((pred == label).any()), bool((ref == label).any())
    if not in_p and not in_r:
        return dict.fromkeys(["HD95", "HD", "ASSD", "NSD"], float("nan"))
    if in_p != in_r:
        return {"HD95": float("inf"), "HD": float("inf"), "ASSD": float("inf"), "NSD": 0.0}
    d_rp, d_pr = label_distances(pred, ref, label, spacing)
    both = np.concatenate([d_rp, d_pr])
    return {"HD95": float(np.percentile(both, 95)), "HD": float(both.max()), "ASSD": float((d_rp.mean() + d_pr.mean()) / 2),
            "NSD": float(((d_rp <= tau).sum() + (d_pr <= tau).sum()) / both.size)}


def bboxes(a, b, nlab):
    """int64 [nlab,6]: inclusive (lo d, h, w, hi d, h, w) of the voxels with label l in a or b; None for a label in neither."""
    out = []
    for l in range(nlab):
        idx = np.argwhere((a == l) | (b == l))
        out.append(None if len(idx) == 0 else (*idx.min(0), *idx.max(0)))
    return out


PAIR_SHAPE = (11, 13, 17)
PAIR_LABELS = [0, 1, 2, 3, 4, 5]


def _ellipsoid(shape, centre, radii):
    g = np.indices(shape).astype(np.float64)
    return sum(((g[k] - centre[k]) / radii[k]) ** 2 for k in range(3)) <= 1.0


@functools.lru_cache(maxsize=None)
def _pair():
    ref, pred = np.zeros(PAIR_SHAPE, dtype=np.int64), np.zeros(PAIR_SHAPE, dtype=np.int64)
    ref[_ellipsoid(PAIR_SHAPE, (5, 6, 8), (4, 5, 7))] = 1
    pred[_ellipsoid(PAIR_SHAPE, (5, 7, 9), (4, 4, 6))] = 1
    ref[_ellipsoid(PAIR_SHAPE, (2, 2, 2), (2, 2, 2))] = 2          # touches the volume edge
    pred[_ellipsoid(PAIR_SHAPE, (8, 10, 14), (2, 2, 2))] = 2       # disjoint from the ball in ref
    ref[0, 0, :] = 3                                               # one voxel thick, on the edge, in both maps
    pred[0, 0, :] = 3
    ref[10, 12, 16] = 4                                            # in ref only
    ref.setflags(write=False), pred.setflags(write=False)          # label 5: in neither
    return ref, pred


def synthetic_pair():
    """(ref, pred): the fixed int64 pair of the surface tests, read-only and shared."""
    return _pair()


def nsd_tau(pred, ref, labels, spacing):
    """A tolerance near 2 that lies in the middle of the widest gap between the distances that occur (so that a distance that is
    off by rounding cannot change a count), and that gap's half width."""
    ds = [1.0, 3.0]
    for l in labels:
        d = label_distances(pred, ref, l, spacing)
        if d is not None:
            ds += [*d[0], *d[1]]
    ds = np.unique(np.asarray(ds))
    ds = ds[(ds >= 1.0) & (ds <= 3.0)]
    k = int(np.argmax(np.diff(ds)))
    return float((ds[k] + ds[k + 1]) / 2), float((ds[k + 1] - ds[k]) / 2)
