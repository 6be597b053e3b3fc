"""numpy reference of the hole filling (test infrastructure, no scipy): `enclosed`, `fill_holes` and `fill_label_holes` as
include/dgtta.h and dg_tta_amd/tta/postprocessing.py define them, built on components_ref.label of the complement.
tests/test_holes_ref.py licenses it against scipy.ndimage.binary_fill_holes; the GPU tests (tests/test_gpu_fill_holes.py) compare
the kernels with it and import no scipy.  The input generators live here too: cached and read-only."""
import functools

import numpy as np

import components_ref as R

SHAPES = R.SHAPES               # the hole filling labels with the tile kernels of the component filter: 8 x 8 x 64
CONNECTIVITIES = R.CONNECTIVITIES
NOISE_SHAPE = R.NOISE_SHAPE
MAX_LABELS = 1024


# ---------------------------------------------------------------------------------------------- definitions
def enclosed(mask, connectivity):
    """bool: the voxels outside `mask` whose component of the complement has no voxel on any of the six faces of the volume."""
    mask = np.asarray(mask).astype(bool)
    cc = R.label((~mask).astype(np.int64), R.own_groups(1), connectivity)
    face = np.zeros(mask.shape, dtype=bool)
    for ax in range(3):
        for end in (0, -1):
            face[tuple(end if a == ax else slice(None) for a in range(3))] = True
    open_names = np.unique(cc[face & ~mask])
    return ~mask & ~np.isin(cc, open_names)


def fill_holes(mask, connectivity):
    """(filled uint8, n_filled)."""
    e = enclosed(mask, connectivity)
    return (np.asarray(mask).astype(bool) | e).astype(np.uint8), int(e.sum())


def fill_label_holes(seg, labels_or_regions=None, connectivity=6, background=0):
    """(filled map int64, {group: filled voxels}): the entries in their order, each on the result of the one before."""
    out = np.asarray(seg).astype(np.int64).copy()
    if labels_or_regions is None:
        labels_or_regions = [int(l) for l in np.unique(out) if 0 < l < MAX_LABELS]
    counts = {}
    for e in labels_or_regions:
        labels = tuple(int(l) for l in e) if isinstance(e, (tuple, list)) else (int(e),)
        inside = np.isin(out, [l for l in labels if 0 <= l < MAX_LABELS])
        change = enclosed(inside, connectivity) & (out == background)
        out[change] = labels[0]
        counts[labels if isinstance(e, (tuple, list)) else labels[0]] = int(change.sum())
    return out, counts


# ---------------------------------------------------------------------------------------------- inputs
def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    a.setflags(write=False)
    return a


def _inner(shape):
    return tuple(n - 2 for n in shape)


@functools.lru_cache(maxsize=None)
def volume(kind, shape):
    """The named uint8 mask on `shape`, or None where the shape is too small for it: 'empty', 'full', 'noise<p>' (occupancy p),
    'shell' (a one-voxel wall around a cavity, one voxel off every face), 'serpentine' (solid, with an enclosed one-voxel-wide
    cavity that snakes through the whole volume one voxel off the faces), 'serpentine_open' (the same, its first voxel let out
    through the face)."""
    if kind == "empty":
        return _ro(np.zeros(shape))
    if kind == "full":
        return _ro(np.ones(shape))
    if kind.startswith("noise"):
        p = float(kind[len("noise"):])
        return _ro(np.random.default_rng([int(1e4 * p), 77, *shape]).random(shape) < p)
    if kind == "shell":
        if min(shape) < 5:
            return None
        m = np.zeros(shape)
        m[1:-1, 1:-1, 1:-1] = 1
        m[2:-2, 2:-2, 2:-2] = 0
        return _ro(m)
    if kind in ("serpentine", "serpentine_open"):
        if min(shape) < 3:
            return None
        m = np.ones(shape)
        m[1:-1, 1:-1, 1:-1] = 1 - R.volume("serpentine", _inner(shape))
        if kind == "serpentine_open":
            m[0, 1, 1] = 0              # the snake starts at the inner (0, 0, 0)
        return _ro(m)
    raise ValueError(kind)


GENERIC_KINDS = ["empty", "full", "noise0.6", "shell", "serpentine", "serpentine_open"]
NOISE_KINDS = ["noise0.5", "noise0.69", "noise0.8"]     # the complement at p = 0.69 sits at the percolation threshold (0.31)

BOX_SHAPE = (18, 20, 140)
BOX_CAVITY = 7 * 14 * 129
TUNNELS = {"closed": None, "face": (0, 0), "edge": (0, -1), "corner": (-1, -1)}
# enclosed voxels per tunnel under 6 / 18 / 26: an edge-only or corner-only tunnel that stays closed adds its inner voxel
BOX_COUNTS = {"closed": (BOX_CAVITY,) * 3, "face": (0, 0, 0), "edge": (BOX_CAVITY + 1, 0, 0), "corner": (BOX_CAVITY + 1, BOX_CAVITY + 1, 0)}


@functools.lru_cache(maxsize=None)
def box(tunnel, at_tile_corner=False):
    """A block d 7..16, h 3..18, w 5..135 with the cavity d 9..15, h 4..17, w 6..134 (it crosses the tile borders d = 8, h = 8 / 16
    and w = 64 / 128); the wall below the cavity is TWO voxels thick (d = 7, 8).  A tunnel takes the wall voxel (8, h, w) under the
    cavity and the voxel (7, h + dh, w + dw) under that: straight below ('face'), across an edge only (closed under 6, open under 18
    and 26) or across a corner only (closed under 6 and 18, open under 26).  (h, w) = (10, 70), or (8, 64) at the corner of four
    tiles, where the two voxels lie in different tiles."""
    m = np.zeros(BOX_SHAPE)
    m[7:17, 3:19, 5:136] = 1
    m[9:16, 4:18, 6:135] = 0
    if TUNNELS[tunnel] is not None:
        h, w = (8, 64) if at_tile_corner else (10, 70)
        dh, dw = TUNNELS[tunnel]
        m[8, h, w] = 0
        m[7, h + dh, w + dw] = 0
    return _ro(m)


@functools.lru_cache(maxsize=None)
def cup():
    """A block that stands on the face d = 0 with a cavity open towards that face: not a hole."""
    m = np.zeros((10, 12, 70))
    m[0:7, 2:10, 3:67] = 1
    m[0:6, 3:9, 4:66] = 0
    return _ro(m)


SHELLS_SHAPE = (13, 15, 75)
SHELLS_COUNT = 9 * 11 * 71 - 5 * 7 * 67 + 3 * 5 * 65


@functools.lru_cache(maxsize=None)
def shells():
    """A shell inside the cavity of a shell: everything inside the outer wall is filled, the inner cavity too."""
    m = np.zeros(SHELLS_SHAPE)
    m[1:-1, 1:-1, 1:-1] = 1
    m[2:-2, 2:-2, 2:-2] = 0
    m[4:-4, 4:-4, 4:-4] = 1
    m[5:-5, 5:-5, 5:-5] = 0
    return _ro(m)


def special_inputs():
    """[(name, mask)]: the boxes with every tunnel at both places, the cup, the shells."""
    out = [(f"box {t}{' at a tile corner' if c else ''}", box(t, c)) for t in TUNNELS for c in (False, True)]
    return out + [("cup", cup()), ("shells", shells())]


@functools.lru_cache(maxsize=None)
def reference(name, connectivity):
    """(filled, n_filled) of a special input or of 'kind|D,H,W': computed once, shared by the tests."""
    if "|" in name:
        kind, shape = name.split("|")
        mask = volume(kind, tuple(int(n) for n in shape.split(",")))
    else:
        mask = dict(special_inputs())[name]
    filled, n = fill_holes(mask, connectivity)
    filled.setflags(write=False)
    return filled, n


def generic_name(kind, shape):
    return f"{kind}|{','.join(map(str, shape))}"


# ---------------------------------------------------------------------------------------------- label maps
@functools.lru_cache(maxsize=None)
def organ_with_lesion():
    """Organ 2 (a block that crosses tile borders) with a lesion of label 3 and a pocket of background inside, organ 4 with a
    pocket next to it, and a stray pocket-free blob of label 1."""
    seg = np.zeros((12, 14, 80), dtype=np.int64)
    seg[1:11, 1:12, 2:70] = 2
    seg[3:5, 3:6, 10:14] = 3            # the lesion: 24 voxels
    seg[6:9, 6:10, 60:68] = 0           # the pocket: 96 voxels, across w = 64
    seg[2:9, 2:9, 72:79] = 4
    seg[4:6, 4:6, 74:76] = 0            # 8 voxels
    seg[11, 13, 0:3] = 1
    seg.setflags(write=False)
    return seg


@functools.lru_cache(maxsize=None)
def high_label_wall():
    """organ_with_lesion with a chimney of label 2000 from the pocket of organ 2 up to the background above the organ: a label
    outside [0, 1024) is never a member, so the pocket is open; organ 4 carries label 1024 and is never looked at."""
    seg = organ_with_lesion().copy()
    seg[1:6, 7, 62] = 2000
    seg[seg == 4] = 1024
    seg.setflags(write=False)
    return seg


@functools.lru_cache(maxsize=None)
def nested_label_shells():
    """A shell of label 1 around background around a shell of label 2 around background: the order of the entries decides
    what the inner cavity becomes."""
    seg = np.zeros(SHELLS_SHAPE, dtype=np.int64)
    m = shells()
    seg[m != 0] = 1
    seg[4:-4, 4:-4, 4:-4] *= 2
    seg.setflags(write=False)
    return seg
