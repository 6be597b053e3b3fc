"""Host tests of dg_tta_amd/pretraining/spatial.py (what `dgtta pretrain --augmentation spatial` draws per batch item and the
voxel map it hands to the sampler) and of the command line switch."""
import math

import numpy as np
import pytest

from dg_tta_amd.pretraining.spatial import SpatialAugmentation, patch_start, rotation_matrix, sampling_map, thin_axis

ISO, ANISO = (32, 40, 48), (8, 64, 64)


def _draws(aug, patch, n, seed):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        a = aug.draw(patch, rs)
        out.append((a, *aug.last))
    return out


def test_draws_are_reproducible_from_the_seed():
    a, b = _draws(SpatialAugmentation(), ISO, 300, 3), _draws(SpatialAugmentation(), ISO, 300, 3)
    c = _draws(SpatialAugmentation(), ISO, 300, 4)
    assert all((x[0] is None and y[0] is None) or np.array_equal(x[0], y[0]) for x, y in zip(a, b))
    assert any((x[0] is None) != (y[0] is None) or (x[0] is not None and not np.array_equal(x[0], y[0])) for x, y in zip(a, c))


def test_draws_use_the_seeded_stream_of_the_package():
    from dg_tta_amd.utils import numpy_rng
    np.random.seed(11)
    st = numpy_rng().get_state()
    a = [SpatialAugmentation(1.0, 1.0).draw(ISO) for _ in range(5)]
    numpy_rng().set_state(st)
    b = [SpatialAugmentation(1.0, 1.0).draw(ISO) for _ in range(5)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_angles_and_factors_stay_inside_their_ranges_and_the_matrix_is_a_scaled_rotation():
    seen_low = seen_high = 0
    for a, angles, factor in _draws(SpatialAugmentation(1.0, 1.0), ISO, 2000, 1):
        assert len(angles) == 3 and all(abs(x) <= math.radians(30.0) for x in angles)
        assert 0.7 <= factor <= 1.4
        seen_low, seen_high = seen_low + (factor < 1.0), seen_high + (factor > 1.0)
        r = a / factor
        assert np.allclose(r @ r.T, np.eye(3), atol=1e-14) and np.linalg.det(r) == pytest.approx(1.0, abs=1e-14)
        assert np.allclose(r, rotation_matrix(*angles), rtol=0, atol=1e-15)
    assert abs(seen_low - 1000) <= 5 * math.sqrt(2000 * 0.25) and seen_low + seen_high == 2000      # the two sides, p = 0.5 each


def test_rotation_matrix_is_rx_ry_rz():
    ax, ay, az = 0.3, -0.2, 0.5
    rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
    assert np.allclose(rotation_matrix(ax, ay, az), rx @ ry @ rz, atol=1e-15)
    assert np.allclose(rotation_matrix(ax, 0, 0) @ [1.0, 0, 0], [1.0, 0, 0])            # Rx turns about the first (D) axis


def test_anisotropic_patch_leaves_the_thin_axis_untouched():
    assert thin_axis(ISO) is None and thin_axis(ANISO) == 0 and thin_axis((64, 64, 8)) == 2 and thin_axis((20, 60, 60)) is None
    wide = 0
    for a, angles, factor in _draws(SpatialAugmentation(1.0, 1.0), ANISO, 1000, 2):
        assert len(angles) == 1 and abs(angles[0]) <= math.pi
        wide += abs(angles[0]) > math.radians(30.0)
        assert np.array_equal(a[0], [1.0, 0.0, 0.0]) and np.array_equal(a[:, 0], [1.0, 0.0, 0.0])
        r = a[1:, 1:] / factor
        assert np.allclose(r @ r.T, np.eye(2), atol=1e-14) and np.linalg.det(r) == pytest.approx(1.0, abs=1e-14)
    assert wide > 700                                                                    # U(-180, 180), not U(-30, 30)
    a = SpatialAugmentation(1.0, 1.0).draw((64, 64, 8), np.random.RandomState(0))
    assert np.array_equal(a[2], [0.0, 0.0, 1.0]) and np.array_equal(a[:, 2], [0.0, 0.0, 1.0])


def test_event_frequencies():
    """Rotation and scaling each fire with probability 0.2, independently: over n = 20 000 draws the counts lie within 5
    binomial sigma, 5 sqrt(0.2 * 0.8 / n) = 0.014 in frequency; both together within 5 sigma of 0.04."""
    n = 20000
    d = _draws(SpatialAugmentation(), ISO, n, 9)
    rot = sum(x[1] is not None for x in d) / n
    sca = sum(x[2] is not None for x in d) / n
    both = sum(x[1] is not None and x[2] is not None for x in d) / n
    none = sum(x[0] is None for x in d) / n
    sigma = math.sqrt(0.2 * 0.8 / n)
    assert abs(rot - 0.2) <= 5 * sigma and abs(sca - 0.2) <= 5 * sigma
    assert abs(both - 0.04) <= 5 * math.sqrt(0.04 * 0.96 / n)
    assert none == pytest.approx(1.0 - rot - sca + both, abs=1e-12)
    assert all((x[0] is None) == (x[1] is None and x[2] is None) for x in d)
    assert all(x[0] is None for x in _draws(SpatialAugmentation(0.0, 0.0), ISO, 200, 1))


def test_patch_start_is_the_start_center_to_offset_encodes():
    from dg_tta_amd.tta.torch_utils import center_to_offset
    shape, patch = (40, 33, 64), (16, 16, 32)
    for center in [(20, 16, 32), (9, 25, 17), (0, 0, 0), (39, 32, 63), (0, 32, 31)]:
        s = patch_start(center, shape, patch)
        assert s == [min(max(c - p // 2, 0), n - p) for c, n, p in zip(center, shape, patch)]
        assert center_to_offset(center, shape, patch) == [(2 * a + p) / n - 1.0 for a, p, n in zip(s, patch, shape)]
    assert patch_start((3, 3, 3), (8, 30, 16), (12, 10, 16)) == [-2, 0, 0]              # smaller than the patch: centred
    assert patch_start((0, 0, 0), (7, 30, 30), (12, 10, 10))[0] == -2


def test_sampling_map_is_exact_for_identity_and_permutations():
    patch, start = (12, 10, 18), [3, -2, 7]
    m = sampling_map(np.eye(3), start, patch)
    assert m.dtype == np.float32 and np.array_equal(m, np.concatenate([np.eye(3), np.array(start)[:, None]], axis=1))
    perm = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    m = sampling_map(perm, start, patch).astype(np.float64)
    assert np.array_equal(m, np.rint(m))
    c = (np.array(patch) - 1) / 2
    assert np.array_equal(m[:, :3] @ c + m[:, 3], np.array(start) + c)                  # the patch centre maps to s + (P - 1) / 2
    a = 1.2 * rotation_matrix(0.2, 0.1, -0.3)
    m = sampling_map(a, start, patch).astype(np.float64)
    assert np.allclose(m[:, :3] @ c + m[:, 3], np.array(start) + c, atol=1e-5) and np.allclose(m[:, :3], a, atol=1e-7)


def test_pretrain_parser_takes_the_augmentation_switch():
    from dg_tta_amd.run import DGTTAProgram
    base = ["802", "3d_fullres", "0", "-tr", "nnUNetTrainer_GIN"]
    parser = DGTTAProgram._pretrain_parser()
    assert parser.parse_args(base).augmentation == "reduced"
    assert parser.parse_args(base + ["--augmentation", "spatial"]).augmentation == "spatial"
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--augmentation", "elastic"])


def test_the_notes_name_what_is_missing():
    from dg_tta_amd.pretraining import trainer
    assert "rotation / scaling and noise" in trainer.REDUCED_AUGMENTATION_NOTE
    note = trainer.SPATIAL_AUGMENTATION_NOTE
    assert "rotation / scaling is applied" in note and "noise / blur / brightness / contrast / gamma" in note
    assert "rotation / scaling and noise" not in note
    with pytest.raises(ValueError):
        trainer.train_fold("802", "3d_fullres", 0, "nnUNetTrainer_GIN", augmentation="elastic")
