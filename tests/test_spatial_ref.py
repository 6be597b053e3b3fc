"""Host test of tests/spatial_ref.py, the float64 restatement the GPU tests of csrc/spatial_aug.hip are measured against:
its prefilter against scipy.ndimage.spline_filter, its image sampler against scipy.ndimage.map_coordinates (order 3 and 1,
mode="constant", cval=0) on the shared map table plus positions outside the volume and within one voxel of its faces, its
label rule on hand-made cases - and that the shared table itself stays inside the exclusion caps the GPU test grants."""
import numpy as np
import pytest
from scipy import ndimage

import spatial_ref as sref

TOL = 1e-12


def _close(got, ref, what, tol=TOL):
    err = float(np.abs(got - ref).max())
    lim = tol * max(float(np.abs(ref).max()), 1.0)
    assert err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e}"


@pytest.mark.parametrize("shape", sref.PREFILTER_SHAPES + sref.SHAPES + [(1, 4, 2), (3, 1, 90)])
def test_prefilter_equals_scipy_spline_filter(shape):
    vol = np.random.RandomState(sum(shape)).standard_normal(shape)
    _close(sref.prefilter(vol), ndimage.spline_filter(vol, order=3, mode="mirror", output=np.float64), f"prefilter {shape}")


def _scipy_sample(vol, m, patch, order):
    x = sref.coordinates(m, patch)
    return ndimage.map_coordinates(vol.astype(np.float64), x.reshape(3, -1), order=order, mode="constant", cval=0.0).reshape(patch)


@pytest.mark.parametrize("order", [3, 1])
@pytest.mark.parametrize("row", range(len(sref.MAP_TABLE)))
def test_image_sampler_equals_scipy_map_coordinates_on_the_table(row, order):
    for item, shape in enumerate(sref.SHAPES):
        img, _ = sref.make_case(shape, 40 + item)
        m = sref.table_map(row, shape, item)
        src = sref.prefilter(img) if order == 3 else img
        val, s, t, inside, _ = sref.sample_image(src, m, sref.PATCH, order)
        _close(val, _scipy_sample(img, m, sref.PATCH, order), f"{sref.MAP_TABLE[row][0]}, item {item}, order {order}")
        assert np.all(s + 1e-12 >= np.abs(val)) and np.all(t[inside] > 0)


@pytest.mark.parametrize("order", [3, 1])
def test_image_sampler_equals_scipy_near_and_beyond_the_faces(order):
    """Positions on a fine line that crosses each face: from 1.5 voxels outside to 1.5 inside, exactly on the face included."""
    shape = (7, 6, 9)
    img = np.random.RandomState(5).standard_normal(shape)
    src = sref.prefilter(img) if order == 3 else img
    steps = np.concatenate([np.linspace(-1.5, 1.5, 25), [0.0, 1e-9, -1e-9]])
    for axis in range(3):
        for face in (0.0, shape[axis] - 1.0):
            for k, off in enumerate(steps):
                m = np.zeros((3, 4))
                m[:, :3] = np.eye(3) * 0.37                  # a 4x3x5 patch of generic positions around the point
                m[:, 3] = [2.2, 1.7, 3.1]
                m[axis, 3] = face + off                      # (both sides read the map rounded to fp32: sref.coordinates)
                val, *_ = sref.sample_image(src, m, (4, 3, 5), order)
                _close(val, _scipy_sample(img, m, (4, 3, 5), order), f"axis {axis} face {face} offset {off}")


def test_label_rule_is_the_crop_for_integer_maps():
    for row in (0, 1):
        assert sref.MAP_TABLE[row][3]
        for item, shape in enumerate(sref.SHAPES):
            _, lab = sref.make_case(shape, 40 + item)
            m = sref.table_map(row, shape, item)
            got, near, _ = sref.sample_labels(lab, m, sref.PATCH)
            assert np.array_equal(got, sref.integer_crop(lab, m, sref.PATCH).astype(np.int64)) and not near.any()


def test_label_rule_is_nearest_where_all_corners_agree():
    for row in (2, 3, 4, 5):
        for item, shape in enumerate(sref.SHAPES):
            _, lab = sref.make_case(shape, 40 + item)
            m = sref.table_map(row, shape, item)
            got, _, agree = sref.sample_labels(lab, m, sref.PATCH)
            x = sref.coordinates(m, sref.PATCH)
            nearest = ndimage.map_coordinates(lab.astype(np.float64), x.reshape(3, -1), order=0, mode="nearest").reshape(sref.PATCH)
            inside = np.all([(x[a] >= 0) & (x[a] <= shape[a] - 1) for a in range(3)], axis=0)
            sel = agree & inside
            assert sel.sum() > 50
            assert np.array_equal(got[sel], nearest[sel].astype(np.int64))


def _one_voxel(lab, pos):
    m = np.zeros((3, 4))
    m[:, 3] = pos
    got, near, _ = sref.sample_labels(lab, m, (1, 1, 1))
    return int(got[0, 0, 0]), bool(near[0, 0, 0])


def test_label_rule_on_hand_made_voxels():
    lab = np.zeros((2, 2, 2))
    lab[0], lab[1] = 2, 5                                     # along D: label 2 at d = 0, label 5 at d = 1
    assert _one_voxel(lab, (0.375, 0.25, 0.5)) == (2, False)  # masses 0.625 / 0.375
    assert _one_voxel(lab, (0.4, 0.0, 0.0))[0] == 2           # masses 0.6 / 0.4
    assert _one_voxel(lab, (0.6, 0.0, 0.0))[0] == 5
    assert _one_voxel(lab, (0.5, 0.5, 0.5)) == (5, True)      # the 0.5 / 0.5 tie goes to the higher id
    lab3 = np.zeros((2, 2, 2))
    lab3[0, 0], lab3[0, 1], lab3[1, 0], lab3[1, 1] = 1, 2, 3, 4
    assert _one_voxel(lab3, (0.5, 0.5, 0.25)) == (0, False)   # four labels with mass 0.25 each: none reaches 0.5
    assert _one_voxel(lab, (-0.75, 0.0, 0.0)) == (0, False)   # the corner outside carries label 0 with mass 0.75
    assert _one_voxel(lab, (-0.25, 0.0, 0.0)) == (2, False)
    bg = np.zeros((2, 2, 2))
    bg[1] = 3
    assert _one_voxel(bg, (0.25, 0.3, 0.3))[0] == 0           # background holds 0.75: label 3 (0.25) does not win


def test_the_shared_table_stays_inside_the_exclusion_caps():
    """What the GPU test may exclude is decided by the reference alone: per table row at most 0.5 % of the label voxels
    within 1e-5 of a tie and at most 1 % of the image voxels within 1e-4 voxel of a face; the integer rows exclude nothing."""
    for row, (name, _, _, exact) in enumerate(sref.MAP_TABLE):
        near_n = face_n = total = 0
        for item, shape in enumerate(sref.SHAPES):
            img, lab = sref.make_case(shape, 40 + item)
            m = sref.table_map(row, shape, item)
            if exact:
                x = sref.coordinates(m, sref.PATCH)
                assert np.array_equal(x, np.rint(x)), name
            near_n += int(sref.sample_labels(lab, m, sref.PATCH)[1].sum())
            face_n += int((sref.sample_image(img, m, sref.PATCH, 1)[4] <= 1e-4).sum())
            total += int(np.prod(sref.PATCH))
        if exact:
            assert near_n == 0, name
        else:
            assert near_n <= 0.005 * total and face_n <= 0.01 * total, (name, near_n, face_n, total)


def test_error_bound_terms():
    assert sref.error_bound(1, 1.0, 1.0, 5.0) == pytest.approx((10.0 + 6.0) * 2.0 ** -24)
    assert sref.error_bound(3, 0.0, 0.0, 1.0) == pytest.approx(702.0 * 2.0 ** -24 * (1 + 88 * 2.0 ** -24))
