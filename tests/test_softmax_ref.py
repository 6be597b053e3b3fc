"""CPU tests of the float64 softmax restatement (tests/softmax_ref.py) the GPU probability tests compare against, and of the
argument checks the Python layer makes before it touches the GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import softmax_ref as ref      # noqa: E402


def _logits(V=300, C=105, seed=0, scale=8.0):
    return np.random.default_rng(seed).standard_normal((V, C)) * scale


def test_restatement_equals_torch_float64():
    l = _logits()
    l[5, 17] = 300.0          # exp overflows without the max subtraction
    l[6] = 0.0                # uniform: entropy ln C, label 0
    st = ref.softmax_stats(l)
    p = torch.softmax(torch.from_numpy(l), dim=1)
    assert np.abs(st["p"] - p.numpy()).max() <= 1e-15
    h = -(p * torch.log(p.clamp_min(1e-300))).sum(1).numpy()
    assert np.abs(st["entropy"] - h).max() <= 1e-12
    assert np.array_equal(st["label"], l.argmax(1))
    assert np.abs(st["confidence"] - p.max(1).values.numpy()).max() <= 1e-15
    assert st["label"][6] == 0 and abs(st["entropy"][6] - np.log(105)) < 1e-13 and abs(st["p"][6] - 1 / 105).max() < 1e-16
    assert (st["entropy"] >= 0).all() and np.isfinite(st["entropy"]).all()


@pytest.mark.parametrize("C", [105, 33, 7])
def test_group_merge_equals_direct_form(C):
    l_sum = _logits(C=C, seed=C) * 3.0      # the chunk functions hand on the SUM over members: scale = 1 / M
    M = 3
    sel = [C - 1, 0] + ([3, 5] if C > 6 else [])
    groups = [(c0, l_sum[:, c0:c0 + 8]) for c0 in range(0, C, 8)]
    order = np.random.default_rng(1).permutation(len(groups))
    st = ref.softmax_stats(l_sum / M)
    for gs in (groups, [groups[i] for i in order]):
        conf, ent, P = ref.online_merge(gs, 1.0 / M, sel)
        assert np.abs(conf - st["confidence"]).max() <= 1e-13
        assert np.abs(ent - st["entropy"]).max() <= 1e-13
        assert np.abs(P - st["p"][:, sel].T).max() <= 1e-13


def test_outside_the_box_convention():
    """Outside the crop box: class 0 with probability 1, everything else 0, confidence 1, entropy 0 - the softmax of a logit vector
    whose class 0 dominates without bound, and consistent with the zero fill of the label map."""
    sel = [4, 0, 2]
    seg = np.full((2, 3, 2), 4)
    probs = np.full((3, 2, 3, 2), 0.25)
    fs, fp, fc, fe = ref.paste_full(seg, probs, np.full((2, 3, 2), 0.5), np.full((2, 3, 2), 1.0), sel, (4, 5, 6),
                                    [(1, 3), (1, 4), (2, 4)], (2, 0, 1))
    assert fs.shape == (6, 4, 5) and fp.shape == (3, 6, 4, 5)
    inside = np.zeros((4, 5, 6), bool)
    inside[1:3, 1:4, 2:4] = True
    inside = inside.transpose(2, 0, 1)
    assert (fs[inside] == 4).all() and (fs[~inside] == 0).all()
    assert (fp[1][~inside] == 1).all() and (fp[0][~inside] == 0).all() and (fp[2][~inside] == 0).all()
    assert (fc[~inside] == 1).all() and (fe[~inside] == 0).all()
    assert (fp[:, inside] == 0.25).all() and (fc[inside] == 0.5).all() and (fe[inside] == 1.0).all()
    lim = ref.softmax_stats(np.array([[800.0, 0.0, 0.0, 0.0, 0.0]]))
    assert lim["p"][0, 0] == 1.0 and (lim["p"][0, 1:] == 0).all() and lim["confidence"][0] == 1.0 and lim["entropy"][0] == 0.0
    # without class 0 among the selected classes every map is 0 outside the box
    _, fp2, _, _ = ref.paste_full(seg, probs[:2], np.ones((2, 3, 2)), np.zeros((2, 3, 2)), [4, 2], (4, 5, 6),
                                  [(1, 3), (1, 4), (2, 4)], (0, 1, 2))
    assert (fp2[:, ~inside.transpose(1, 2, 0)] == 0).all()


def test_bounds_are_zero_order_sane():
    st = ref.softmax_stats(_logits(V=50, C=33))
    pb, hb = ref.bounds(st, np.zeros(50))
    assert (pb > 0).all() and (pb < 1e-4).all() and (hb > 0).all() and (hb < 1e-3).all()
    pb16, _ = ref.bounds(st, np.zeros(50), np.float16)
    assert (pb16 >= pb + 2.0 ** -25).all()


def test_selected_classes_are_checked_without_a_gpu():
    from dg_tta_amd import ops
    from dg_tta_amd.tta import inference
    assert ops.check_selected_classes([3, 0, 104], 105) == [3, 0, 104]
    for bad in ([0, 3, 3], [0, 105], [-1, 2], [], list(range(33))):
        with pytest.raises(ValueError):
            ops.check_selected_classes(bad, 105)
    facc, nsum = torch.zeros(1, 2, 2, 2, 32), torch.ones(2, 2, 2)      # CPU tensors: the class check comes first
    w, b = torch.zeros(1, 5, 32), torch.zeros(5)
    with pytest.raises(ValueError, match="duplicate"):
        ops.feature_head_softmax(facc, nsum, w, b, [1, 1])
    with pytest.raises(ValueError, match="outside"):
        ops.feature_head_softmax(facc, nsum, w, b, [0, 5])
    with pytest.raises(ValueError, match="float32 or float16"):
        ops.feature_head_softmax(facc, nsum, w, b, [0, 1], prob_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="fp32 GPU accumulators"):
        ops.feature_head_softmax(facc, nsum, w, b, [0, 1])
    feats = inference.WindowFeatures(facc, nsum, (slice(0, 2),) * 3, w, b[None])
    with pytest.raises(ValueError, match="duplicate"):
        inference.export_probabilities(feats, nsum, feats.crop, None, None, None, 1, [2, 2])
    with pytest.raises(ValueError, match="outside"):
        inference.export_probabilities(torch.zeros(2, 2, 2, 5), nsum, feats.crop, None, None, None, 1, [0, 7])
    with pytest.raises(ValueError, match="members"):
        inference.export_probabilities(feats, nsum, feats.crop, None, None, None, 2, [0, 1])
    assert ops.feature_head_softmax_supported(3, 105) and ops.feature_head_softmax_supported(2, 128)
    assert not ops.feature_head_softmax_supported(2, 150) and not ops.feature_head_softmax_supported(9, 128)


def test_plan_keys_are_opt_in():
    from dg_tta_amd.tta import config_log_utils as clu
    assert "inference_save_probabilities" not in clu.TEMPLATE_PLAN and "inference_save_uncertainty" not in clu.TEMPLATE_PLAN
