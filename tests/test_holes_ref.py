"""CPU: licenses the numpy reference tests/holes_ref.py, which the GPU tests of the hole filling compare the kernels with, against
scipy.ndimage.binary_fill_holes: connectivity 6 is its default structure, 18 and 26 are generate_binary_structure(3, 2) and
(3, 3).  Every generator of holes_ref, all three connectivities, exact equality on every voxel."""
import numpy as np
import pytest
from scipy import ndimage as ndi

import holes_ref as HR

STRUCTURE = {6: ndi.generate_binary_structure(3, 1), 18: ndi.generate_binary_structure(3, 2), 26: ndi.generate_binary_structure(3, 3)}


def _check(name, mask, connectivity):
    want = ndi.binary_fill_holes(mask, structure=STRUCTURE[connectivity])
    filled, n = HR.reference(name, connectivity)
    assert filled.dtype == np.uint8 and np.array_equal(filled.astype(bool), want), f"{name} c{connectivity}"
    assert n == int(want.sum()) - int(np.count_nonzero(mask)), f"{name} c{connectivity}"
    return n


@pytest.mark.parametrize("connectivity", HR.CONNECTIVITIES)
@pytest.mark.parametrize("shape", HR.SHAPES, ids=str)
def test_generic_inputs_vs_scipy(shape, connectivity):
    seen = 0
    for kind in HR.GENERIC_KINDS:
        mask = HR.volume(kind, shape)
        if mask is not None:
            _check(HR.generic_name(kind, shape), mask, connectivity)
            seen += 1
    assert seen >= 3                # empty, full and noise exist on every shape


@pytest.mark.parametrize("connectivity", HR.CONNECTIVITIES)
def test_special_inputs_vs_scipy_and_their_known_counts(connectivity):
    k = HR.CONNECTIVITIES.index(connectivity)
    for name, mask in HR.special_inputs():
        n = _check(name, mask, connectivity)
        if name.startswith("box"):
            assert n == HR.BOX_COUNTS[name.split()[1]][k], name
    assert HR.reference("cup", connectivity)[1] == 0
    assert HR.reference("shells", connectivity)[1] == HR.SHELLS_COUNT


@pytest.mark.parametrize("connectivity", HR.CONNECTIVITIES)
@pytest.mark.parametrize("kind", HR.NOISE_KINDS)
def test_noise_vs_scipy(kind, connectivity):
    _check(HR.generic_name(kind, HR.NOISE_SHAPE), HR.volume(kind, HR.NOISE_SHAPE), connectivity)


def test_the_serpentine_cavity_is_one_hole_and_opens_through_one_voxel():
    shape = (17, 33, 129)
    snake = int((HR.volume("serpentine", shape) == 0).sum())
    for c in HR.CONNECTIVITIES:
        assert HR.reference(HR.generic_name("serpentine", shape), c)[1] == snake > 1000
        assert HR.reference(HR.generic_name("serpentine_open", shape), c)[1] == 0


def test_an_axis_of_extent_one_or_two_encloses_nothing():
    for shape in ((1, 9, 9), (9, 2, 9), (9, 9, 1), (2, 2, 2)):
        mask = np.ones(shape, dtype=np.uint8)
        mask[tuple(n // 2 for n in shape)] = 0
        assert HR.fill_holes(mask, 6)[1] == 0


def _scipy_label_loop(seg, entries, connectivity, background=0):
    """isin -> binary_fill_holes -> (& map == background) -> assign, entry by entry."""
    out, counts = seg.astype(np.int64).copy(), {}
    for e in entries:
        labels = e if isinstance(e, tuple) else (e,)
        filled = ndi.binary_fill_holes(np.isin(out, [l for l in labels if 0 <= l < HR.MAX_LABELS]), structure=STRUCTURE[connectivity])
        change = filled & (out == background)
        out[change] = labels[0]
        counts[e] = int(change.sum())
    return out, counts


@pytest.mark.parametrize("connectivity", HR.CONNECTIVITIES)
def test_label_filling_vs_the_scipy_loop(connectivity):
    organ, nested, wall = HR.organ_with_lesion(), HR.nested_label_shells(), HR.high_label_wall()
    cases = [(organ, [1, 2, 3, 4]), (organ, [(3, 2), 4]), (organ, [4, (2, 3)]), (nested, [1, 2]), (nested, [2, 1]), (nested, [(2, 1)]),
             (wall, [2, 1024, 2000]), (wall, [(2, 2000)]), (HR.volume("noise0.69", HR.NOISE_SHAPE).astype(np.int64) * 3, [3])]
    for seg, entries in cases:
        got, counts = HR.fill_label_holes(seg, entries, connectivity)
        want, want_counts = _scipy_label_loop(seg, entries, connectivity)
        assert np.array_equal(got, want) and counts == want_counts, entries
    got, counts = HR.fill_label_holes(organ, None, connectivity)
    want, want_counts = _scipy_label_loop(organ, [1, 2, 3, 4], connectivity)
    assert np.array_equal(got, want) and counts == want_counts
    got, counts = HR.fill_label_holes(organ, [2], connectivity, background=3)       # the lesion is the "background" here
    assert counts == {2: 24} and np.array_equal(got, _scipy_label_loop(organ, [2], connectivity, background=3)[0])


def test_label_filling_known_results():
    organ = HR.organ_with_lesion()
    got, counts = HR.fill_label_holes(organ, None, 6)
    assert counts == {1: 0, 2: 96, 3: 0, 4: 8}
    assert (got[organ == 3] == 3).all() and (got[6:9, 6:10, 60:68] == 2).all() and (got[4:6, 4:6, 74:76] == 4).all()
    assert np.array_equal(got == 0, (organ == 0) & (got == 0)) and (got != organ).sum() == 104
    got, counts = HR.fill_label_holes(HR.high_label_wall(), None, 6)          # the chimney opens organ 2's pocket; 1024 is not looked at
    assert counts == {1: 0, 2: 0, 3: 0} and np.array_equal(got, HR.high_label_wall())
    nested = HR.nested_label_shells()
    assert (HR.fill_label_holes(nested, [1, 2], 6)[0][6, 7, 37] == 1) and (HR.fill_label_holes(nested, [2, 1], 6)[0][6, 7, 37] == 2)
