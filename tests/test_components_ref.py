"""Licenses tests/components_ref.py (the numpy reference the GPU tests of csrc/components.hip compare with) against
scipy.ndimage.label with generate_binary_structure(3, 1 | 2 | 3): every voxel of the canonical component map, the sizes, and the
keep-largest / minimum-size filter against a direct scipy loop.  CPU only."""
import numpy as np
import pytest

import components_ref as R

ndi = pytest.importorskip("scipy.ndimage")

RANK = {6: 1, 18: 2, 26: 3}


def scipy_cc(seg, table, connectivity):
    """Per group: scipy's components, renamed to 1 + the first linear index of each."""
    g = R.group_map(seg, table)
    cc = np.zeros(g.shape, dtype=np.int32)
    for c in np.unique(g[g != 0]):
        lab, n = ndi.label(g == c, structure=ndi.generate_binary_structure(3, RANK[connectivity]))
        flat = lab.reshape(-1)
        idx = np.flatnonzero(flat)
        first = np.full(n + 1, g.size, dtype=np.int64)
        np.minimum.at(first, flat[idx], idx)
        cc[lab > 0] = (first[lab[lab > 0]] + 1).astype(np.int32)
    return cc


def scipy_filter(seg, table, connectivity, keep_largest, min_voxels, background):
    g = R.group_map(seg, table)
    out, removed = np.array(seg, dtype=np.int64), np.zeros(len(table), dtype=np.int64)
    for c in np.unique(g[g != 0]):
        lab, n = ndi.label(g == c, structure=ndi.generate_binary_structure(3, RANK[connectivity]))
        count = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
        best = 1 + int(np.argmax(count))        # scipy numbers components by their first voxel, argmax takes the first maximum
        for k in range(1, n + 1):
            if (keep_largest and k != best) or count[k - 1] < min_voxels:
                out[lab == k] = background
                removed[c] += count[k - 1]
    return out, removed


def check_cc(seg, table, connectivity):
    cc = R.label(seg, table, connectivity)
    assert cc.dtype == np.int32
    assert np.array_equal(cc, scipy_cc(seg, table, connectivity))
    size = R.sizes(cc)
    assert size.dtype == np.int32 and size.shape == (seg.size,)
    assert np.array_equal(size, np.bincount(cc[cc > 0].astype(np.int64) - 1, minlength=seg.size))
    roots = np.flatnonzero(size)
    assert np.array_equal(cc.reshape(-1)[roots], roots + 1)       # a component is named by its first voxel
    return cc


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_label_and_sizes_match_scipy(shape, connectivity):
    for kind in R.GENERIC_KINDS:
        check_cc(R.volume(kind, shape), R.own_groups(5), connectivity)
        check_cc(R.volume(kind, shape), R.one_group(5), connectivity)


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
def test_special_inputs_match_scipy(connectivity):
    for seg in (R.contact_pair("edge"), R.contact_pair("corner"), R.u_shapes(), R.tie_volume()):
        check_cc(seg, R.own_groups(5), connectivity)
        check_cc(seg, R.one_group(5), connectivity)
    for p in ("0.2", "0.31", "0.5"):
        check_cc(R.volume(f"noise{p}x1", R.NOISE_SHAPE), R.own_groups(1), connectivity)
        check_cc(R.volume(f"noise{p}x5", R.NOISE_SHAPE), R.own_groups(5), connectivity)


def n_components(seg, table, connectivity):
    return int(np.count_nonzero(R.sizes(R.label(seg, table, connectivity))))


def test_known_component_counts():
    board = R.volume("checkerboard", (4, 4, 4))
    assert [n_components(board, R.own_groups(1), c) for c in R.CONNECTIVITIES] == [32, 1, 1]
    assert [n_components(R.contact_pair("edge"), R.own_groups(1), c) for c in R.CONNECTIVITIES] == [2, 1, 1]
    assert [n_components(R.contact_pair("corner"), R.own_groups(1), c) for c in R.CONNECTIVITIES] == [2, 2, 1]
    halves = R.volume("halves", (9, 17, 33))
    assert n_components(halves, R.own_groups(2), 6) == 2 and n_components(halves, R.one_group(2), 6) == 1
    assert all(n_components(R.u_shapes(), R.own_groups(3), c) == 3 for c in R.CONNECTIVITIES)
    for shape in R.SHAPES:
        snake = R.volume("serpentine", shape)
        assert n_components(snake, R.own_groups(1), 6) == 1
    # near the percolation threshold the components are many and tangled: the hard case for a union-find
    noise = R.volume("noise0.31x1", R.NOISE_SHAPE)
    counts = [n_components(noise, R.own_groups(1), c) for c in R.CONNECTIVITIES]
    assert counts[0] > 1000 > counts[1] > counts[2] > 1


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
@pytest.mark.parametrize("keep_largest,min_voxels,background", [(True, 0, 0), (False, 5, 0), (True, 4, 7), (False, 0, 0)])
def test_filter_matches_scipy_loop(connectivity, keep_largest, min_voxels, background):
    cases = [(R.tie_volume(), R.own_groups(4)), (R.tie_volume(), np.array([0, 1, 2, 2, 3], dtype=np.int32)),
             (R.volume("noise0.31x5", R.NOISE_SHAPE), R.own_groups(5)), (R.volume("noise0.2x5", (7, 9, 65)), R.one_group(5)),
             (R.volume("noise0.5x5", (9, 17, 33)), np.array([0, 2, 0, 2, 1, 7], dtype=np.int32))]
    for seg, table in cases:
        out, removed = R.filter_map(seg, table, connectivity, keep_largest, min_voxels, background)
        ref_out, ref_removed = scipy_filter(seg, table, connectivity, keep_largest, min_voxels, background)
        assert np.array_equal(out, ref_out) and np.array_equal(removed, ref_removed)


def test_tie_and_threshold_rules():
    seg = R.tie_volume()
    out, removed = R.filter_map(seg, R.own_groups(4), 26)
    assert (out[0, 0, 0:3] == 1).all() and (out[2, 2, 65:68] == 0).all()          # equal sizes: the first component stays
    assert removed.tolist() == [0, 3, 0, 0, 4]
    out, removed = R.filter_map(seg, np.array([0, 0, 1, 1, 0], dtype=np.int32), 26)
    assert (out[1, 4, 10:14] == 3).all() and (out[3, 4, 60:64] == 0).all()        # labels 2 and 3 as one region tie as well
    assert removed.tolist() == [0, 4, 0, 0, 0]
    out, removed = R.filter_map(seg, R.own_groups(4), 26, keep_largest=False, min_voxels=5)
    assert (out[0, 6, 30:35] == 4).all() and np.count_nonzero(out) == 5           # exactly min_voxels stays, one below goes
    assert removed.tolist() == [0, 6, 4, 4, 4]
