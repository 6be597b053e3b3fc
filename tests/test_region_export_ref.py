"""Licenses tests/region_export_ref.py (no GPU): against an explicit voxel loop of nnU-Net's region rule
(convert_probabilities_to_segmentation: seg = 0; for i, c in enumerate(regions_class_order): seg[p_i > 0.5] = c - from memory of
nnunetv2 2.2.1, unpinned) on a hand-built example with overlapping regions and a non-monotone order, and against the sign
convention of tests/region_ref.py."""
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import region_export_ref as xref      # noqa: E402
import region_ref      # noqa: E402


def _voxel_loop(logits, order, by="logit"):
    """nnU-Net's rule voxel by voxel.  by="probability": as it is written there, sigmoid(l_i) > 0.5; by="logit": l_i > 0, the same
    set in exact arithmetic and the form the engine decides by (dgtta_logits_regions) - a rounded sigmoid returns exactly 0.5 for
    0 < l < 1e-16, which is a property of the rounding, not of the rule."""
    out = []
    for row in logits:
        lab = 0
        for i, c in enumerate(order):
            x = float(row[i])
            if math.isnan(x):
                continue
            if by == "probability":
                inside = (1.0 / (1.0 + math.exp(-x)) if x >= 0 else math.exp(x) / (1.0 + math.exp(x))) > 0.5
            else:
                inside = x > 0
            if inside:
                lab = c
        out.append(lab)
    return np.asarray(out, dtype=np.int32)


def test_hand_built_overlapping_regions_with_a_non_monotone_order():
    # whole tumour (1, 2, 3) > tumour core (2, 3) > enhancing (3), written back as 1, 3, 2: a KiTS / BraTS-like nesting
    order = [1, 3, 2]
    logits = np.array([[-1.0, -1.0, -1.0],      # nothing                       -> 0
                       [2.0, -1.0, -1.0],       # region 0 only                 -> 1
                       [2.0, 1.0, -1.0],        # 0 and 1                       -> 3
                       [2.0, 1.0, 0.5],         # all three: the last one wins  -> 2
                       [-2.0, -1.0, 0.5],       # only the innermost            -> 2
                       [-2.0, 1.0, -0.5],       # only the middle one           -> 3
                       [0.0, -0.0, np.nan],     # 0, -0 and NaN are not inside  -> 0
                       [5e-324, 0.0, -5e-324]])  # the smallest positive double  -> 1
    want = np.array([0, 1, 3, 2, 2, 3, 0, 1], dtype=np.int32)
    assert np.array_equal(_voxel_loop(logits, order), want)
    assert np.array_equal(_voxel_loop(logits[:7], order, by="probability"), want[:7])      # (row 7 lies inside the sigmoid's rounding)
    for group in (1, 2, 3, 8):
        assert np.array_equal(xref.merge_groups(logits, order, group), want)
    label, probs = xref.region_export(2.0 * logits, order, 0.5, group=2)      # two members: the sum decides, the mean is squashed
    assert np.array_equal(label, want) and probs.shape == (3, 8)
    assert probs[0, 1] == 1.0 / (1.0 + math.exp(-2.0)) and probs[0, 0] == math.exp(-1.0) / (1.0 + math.exp(-1.0))
    assert probs[0, 6] == 0.5 and probs[1, 6] == 0.5 and np.isnan(probs[2, 6])


def test_random_groups_against_the_voxel_loop_and_region_ref():
    rng = np.random.default_rng(3)
    for R, group in ((1, 8), (3, 8), (9, 8), (19, 8), (32, 8), (19, 5)):
        order = (rng.permutation(1000)[:R] + 1).tolist()
        logits = rng.standard_normal((257, R)) * 2
        logits[rng.random(logits.shape) < 0.05] = 0.0
        got = xref.merge_groups(logits, order, group)
        assert np.array_equal(got, _voxel_loop(logits, order)) and np.array_equal(got, _voxel_loop(logits, order, by="probability"))
        assert np.array_equal(got, region_ref.region_label_map(logits, order))              # the sign convention of region_ref
        assert np.array_equal(got, region_ref.region_label_map(3.0 * logits, order))        # ... under any positive multiple


def test_stable_sigmoid_never_overflows_and_matches_the_textbook_form():
    x = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 745.0, -745.0, 800.0, -800.0, np.inf, -np.inf, 0.3, -0.3])
    with np.errstate(all="raise"):
        p = xref.stable_sigmoid(x)
    assert np.isfinite(p).all() and p[-4] == 1.0 and p[-3] == 0.0 and p[8] == 1.0 and p[9] == 0.0
    assert p[0] == p[1] == p[2] == p[3] == 0.5
    assert abs(p[-2] - 1.0 / (1.0 + math.exp(-0.3))) < 1e-16 and abs(p[-1] + p[-2] - 1.0) < 2e-16
    assert 0.0 < p[7] < 1e-300                      # exp(-745) is a subnormal double, not 0


def test_paste_and_bound():
    seg = np.arange(1, 25).reshape(2, 3, 4)
    probs = np.stack([seg / 100.0, seg / 50.0])
    fs, fp = xref.paste_full(seg, probs, (4, 5, 4), [[1, 3], [2, 5], [0, 4]], [2, 0, 1])
    assert fs.shape == (4, 4, 5) and fp.shape == (2, 4, 4, 5)
    assert fs[:, 0].sum() == 0 and fs[:, 3].sum() == 0 and fs[2, 1, 3] == seg[0, 1, 2] and fp[1, 2, 1, 3] == probs[1, 0, 1, 2]
    assert (fs != 0).sum() == 24 and (fp != 0).sum() == 48
    b16 = xref.prob_bound(np.array([1.0, 0.75, 0.5, 0.4999, 1e-9, 0.0, np.nan]), np.float16)
    assert list(b16[:4]) == [2.0 ** -10, 2.0 ** -11, 2.0 ** -11, 2.0 ** -12] and b16[4] == b16[5] == 2.0 ** -24 and np.isnan(b16[6])
    b32 = xref.prob_bound(np.array([1.0, 0.5, 1e-40, 0.0]), np.float32)
    assert list(b32) == [2.0 ** -23, 2.0 ** -24, 2.0 ** -149, 2.0 ** -149]
