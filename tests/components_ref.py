"""numpy reference of the connected-component post-processing (test infrastructure, no scipy): groups, connectivity 6 / 18 / 26,
the canonical component map cc, component sizes, and the keep-largest / minimum-size filter with its tie rule, as
include/dgtta.h and dg_tta_amd/tta/postprocessing.py define them.  Labelling is minimum-label propagation over all neighbour
shifts, with hooking of the roots and pointer jumping in between, so that a snake through the whole volume does not need one
sweep per voxel.
tests/test_components_ref.py licenses it against scipy.ndimage.label; the GPU tests (tests/test_gpu_components.py) compare the
kernels with it and import no scipy.  The input generators live here too: seeded, cached and read-only."""
import functools
import itertools

import numpy as np

# the shapes the issue lists, and (3, 7, 63): the kernels' tile is 8 x 8 x 64, and the list has D at 7 / 9 / 17, H at 9 / 17 and
# W at 65 / 129, but neither H = 7 nor W = 63
SHAPES = [(1, 1, 1), (1, 1, 130), (2, 3, 5), (7, 9, 65), (9, 17, 33), (17, 33, 129), (3, 7, 63)]
CONNECTIVITIES = [6, 18, 26]
NOISE_SHAPE = (33, 34, 70)


# ---------------------------------------------------------------------------------------------- definitions
def neighbour_offsets(connectivity):
    """All (dd, dh, dw) != 0 in {-1, 0, 1}^3 with at most 1 / 2 / 3 non-zero entries."""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(map(abs, o)) <= most]


def group_map(seg, table):
    """g = table[seg], 0 where the label or the table entry lies outside [0, len(table))."""
    seg, table = np.asarray(seg), np.asarray(table)
    g = np.zeros(seg.shape, dtype=np.int64)
    ok = (seg >= 0) & (seg < len(table))
    g[ok] = table[seg[ok]]
    g[(g < 0) | (g >= len(table))] = 0
    return g


def _shifted(shape, off):
    """Slices (a, b) with b = a + off, both inside the volume."""
    a = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip(off, shape))
    b = tuple(slice(max(0, o), n - max(0, -o)) for o, n in zip(off, shape))
    return a, b


def label(seg, table, connectivity):
    """cc int32: 0 where g == 0, else 1 + the smallest linear index of the voxel's component."""
    g = group_map(seg, table)
    n = g.size
    lab = np.where(g != 0, np.arange(n, dtype=np.int64).reshape(g.shape), n)
    pairs = []
    for off in neighbour_offsets(connectivity):
        a, b = _shifted(g.shape, off)
        pairs.append((a, b, (g[a] == g[b]) & (g[a] != 0)))
    flat, fg = lab.reshape(-1), (g != 0).reshape(-1)
    while True:
        before = lab.copy()
        for a, b, same in pairs:
            lab[a] = np.minimum(lab[a], np.where(same, lab[b], n))
        # hand the smaller label to the voxel that named this one before (after the jumps below: the root of its tree), so that
        # a whole tree follows in this round and not only the voxel at its border
        np.minimum.at(flat, before.reshape(-1)[fg], flat[fg])
        while True:                 # lab[i] is a voxel of i's component with a label <= its index: jump to that voxel's label
            jumped = flat[flat[fg]]
            if np.array_equal(jumped, flat[fg]):
                break
            flat[fg] = jumped
        if np.array_equal(lab, before):
            break
    return np.where(g != 0, lab + 1, 0).astype(np.int32)


def sizes(cc):
    """size int32 [n]: size[r] = voxels with cc == r + 1."""
    cc = np.asarray(cc).reshape(-1)
    return np.bincount(cc[cc > 0] - 1, minlength=cc.size).astype(np.int32)


def winners(seg, table, size):
    """{group: first index of its largest component}; ties go to the smaller index."""
    g = group_map(seg, table).reshape(-1)
    out = {}
    for r in np.flatnonzero(size):              # ascending, so a later equal size does not replace an earlier one
        c = int(g[r])
        if c not in out or size[r] > size[out[c]]:
            out[c] = int(r)
    return out


def filter_map(seg, table, connectivity, keep_largest=True, min_voxels=0, background=0):
    """(filtered map int64, removed int64 [len(table)])."""
    seg = np.asarray(seg)
    g = group_map(seg, table)
    cc = label(seg, table, connectivity)
    size = sizes(cc)
    comp = cc.astype(np.int64) - 1
    keep = size[np.maximum(comp, 0)] >= min_voxels
    if keep_largest:
        win = np.full(len(table), -1, dtype=np.int64)
        for c, r in winners(seg, table, size).items():
            win[c] = r
        keep &= comp == win[g]
    drop = (g != 0) & ~keep
    out = seg.astype(np.int64)
    out[drop] = background
    return out, np.bincount(g[drop], minlength=len(table)).astype(np.int64)


# ---------------------------------------------------------------------------------------------- tables
def own_groups(nlab):
    """Every label 1 .. nlab its own group."""
    return np.arange(nlab + 1, dtype=np.int32)


def one_group(nlab):
    """Labels 1 .. nlab share group 1."""
    t = np.ones(nlab + 1, dtype=np.int32)
    t[0] = 0
    return t


# ---------------------------------------------------------------------------------------------- inputs
def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def volume(kind, shape):
    """The named int64 input on `shape`: 'background', 'solid' (all label 3), 'checkerboard' ((d + h + w) % 2), 'halves' (labels 1
    and 2 in face contact across the middle of the longest axis), 'serpentine' (a one-voxel-wide snake of label 1 through the
    whole volume), 'noise<p>x<nlab>' (occupancy p, labels 1 .. nlab uniformly)."""
    d, h, w = np.indices(shape)
    if kind == "background":
        return _ro(np.zeros(shape))
    if kind == "solid":
        return _ro(np.full(shape, 3))
    if kind == "checkerboard":
        return _ro((d + h + w) % 2)
    if kind == "halves":
        ax = int(np.argmax(shape))
        return _ro(1 + (np.indices(shape)[ax] >= (shape[ax] + 1) // 2))
    if kind == "serpentine":
        D, H, W = shape
        plane = np.zeros((H, W), dtype=np.int64)
        plane[0::2] = 1                                         # rows along W ...
        for k, hh in enumerate(range(1, H, 2)):
            plane[hh, (W - 1) if k % 2 == 0 else 0] = 1         # ... joined at alternating ends
        last = (H - 1) // 2 * 2
        ends = [(0, 0), (last, (W - 1) if (last // 2) % 2 == 0 else 0)]
        seg = np.zeros(shape, dtype=np.int64)
        seg[0::2] = plane
        for k, dd in enumerate(range(1, D, 2)):                 # planes joined where the snake of the plane below ends
            seg[(dd, *ends[(k + 1) % 2])] = 1
        return _ro(seg)
    if kind.startswith("noise"):
        p, nlab = kind[len("noise"):].split("x")
        rng = np.random.default_rng([int(1e4 * float(p)), int(nlab), *shape])
        return _ro((rng.random(shape) < float(p)) * rng.integers(1, int(nlab) + 1, shape))
    raise ValueError(kind)


GENERIC_KINDS = ["background", "solid", "checkerboard", "halves", "serpentine", "noise0.2x1", "noise0.31x1", "noise0.5x1", "noise0.2x5",
                 "noise0.31x5", "noise0.5x5"]


@functools.lru_cache(maxsize=None)
def contact_pair(kind):
    """Two voxels of label 1 across the corner (7|8, 7|8, 63|64) of four tiles, touching by an 'edge' or by a 'corner' only."""
    seg = np.zeros((10, 10, 70), dtype=np.int64)
    seg[7, 7, 63] = 1
    seg[{"edge": 7, "corner": 8}[kind], 8, 64] = 1
    return _ro(seg)


@functools.lru_cache(maxsize=None)
def u_shapes():
    """Three U's (labels 1, 2, 3) whose arms run along W, D and H, leave their tile apart and meet only in the next one."""
    seg = np.zeros((12, 20, 130), dtype=np.int64)
    seg[1, 1, 10:101] = seg[1, 3, 10:101] = seg[1, 1:4, 100] = 1
    seg[2:11, 6, 5] = seg[2:11, 8, 5] = seg[10, 6:9, 5] = 2
    seg[5, 3:14, 20] = seg[5, 3:14, 22] = seg[5, 13, 20:23] = 3
    return _ro(seg)


@functools.lru_cache(maxsize=None)
def tie_volume():
    """Label 1: two components of 3 voxels (the first wins); labels 2 and 3: one component of 4 voxels each, the one of label 3
    first, so as one region they tie too; label 4: components of 5 and of 4 voxels for the size threshold."""
    seg = np.zeros((4, 9, 70), dtype=np.int64)
    seg[0, 0, 0:3] = seg[2, 2, 65:68] = 1
    seg[1, 4, 10:14] = 3
    seg[3, 4, 60:64] = 2
    seg[0, 6, 30:35] = seg[3, 8, 1:5] = 4
    return _ro(seg)


@functools.lru_cache(maxsize=None)
def reference(kind, shape, table_name, nlab, connectivity):
    """(cc, size) of volume(kind, shape) under own_groups / one_group(nlab): computed once, shared by the tests."""
    cc = label(volume(kind, shape), {"own": own_groups, "one": one_group}[table_name](nlab), connectivity)
    size = sizes(cc)
    cc.setflags(write=False), size.setflags(write=False)
    return cc, size
