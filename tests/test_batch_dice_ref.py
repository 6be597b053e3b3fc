"""CPU: tests/batch_dice_ref.py (the float64 restatement tests/test_gpu_batch_dice.py compares the batch mode of csrc/dice_ce.hip
with) against float64 torch autograd of a plain restatement of nnU-Net's expression, and the host logic that came with the batch
Dice: the plans' switch, the moving average behind checkpoint_best.pth, the new `dgtta pretrain` options.  Float64 throughout:
agreement to about 1e-12."""
import math

import numpy as np
import pytest
import torch

import batch_dice_ref
import loss_ref

TOL = dict(rtol=1e-11, atol=1e-13)


def _torch_batch_dice_ce(logits, labels, smooth, do_bg):
    """DC_and_CE_loss with MemoryEfficientSoftDiceLoss(batch_dice=True) as nnU-Net writes it (from memory of nnunetv2 2.2.1,
    unpinned), float64: logits [B][C][V], labels [B][V]; labels outside [0, C) are masked out of every sum.  The reductions run
    over the voxels of a sample, then over the samples - literally."""
    B, C, V = logits.shape
    valid = ((labels >= 0) & (labels < C))[:, None].double()                       # [B][1][V]
    safe = labels.clamp(0, C - 1)
    p = logits.softmax(1)
    oh = torch.nn.functional.one_hot(safe, C).movedim(-1, 1).double()
    intersect = torch.stack([(p[b] * oh[b] * valid[b]).sum(1) for b in range(B)]).sum(0)            # [C]
    sum_pred = torch.stack([(p[b] * valid[b]).sum(1) for b in range(B)]).sum(0)
    sum_gt = torch.stack([(oh[b] * valid[b]).sum(1) for b in range(B)]).sum(0)
    dc = (2 * intersect + smooth) / torch.clip(sum_gt + sum_pred + smooth, 1e-8)
    dl = -dc[(0 if do_bg else 1):].mean()
    logp = torch.log_softmax(logits, 1)
    ce = -(logp.gather(1, safe[:, None]) * valid).sum() / valid.sum().clamp_min(1)
    return ce + dl, ce, dl, dc


def _labels(rng, B, C, shape):
    """A class present in sample 0 only (C - 1, when C >= 3), a class absent from the whole batch (C - 2, when C >= 4), ignored
    values, and - with B >= 3 - sample 1 entirely out of range."""
    y = rng.randint(0, C, size=(B, *shape)).astype(np.int64)
    flat = y.reshape(B, -1)
    if C >= 4:
        flat[flat == C - 2] = 0
    if C >= 3 and B >= 2:
        flat[1:][flat[1:] == C - 1] = 0
    if flat.shape[1] >= 8:
        flat[0, :4] = [-1, C, 255 if C <= 255 else C + 1, -2 ** 40]
    if B >= 3:
        flat[1] = -1
    return y


@pytest.mark.parametrize("do_bg", [False, True])
@pytest.mark.parametrize("smooth", [1e-5, 0.0])
@pytest.mark.parametrize("B,C,V", [(1, 2, 1), (2, 3, 50), (3, 16, 31), (2, 105, 40), (8, 5, 9)])
def test_batch_dice_ce_matches_torch_float64(B, C, V, smooth, do_bg):
    rng = np.random.RandomState(C * 10 + V + B)
    z = rng.normal(size=(B, C, V)) * 3
    y = _labels(rng, B, C, (V,))
    tz = torch.tensor(z, requires_grad=True)
    loss, ce, dl, dice = _torch_batch_dice_ce(tz, torch.tensor(y), smooth, do_bg)
    loss.backward()
    (rl, rce, rdl), rdice, rgrad = batch_dice_ref.dice_ce_batch(z, y, smooth, do_bg)
    np.testing.assert_allclose([rl, rce, rdl], [float(x.detach()) for x in (loss, ce, dl)], **TOL)
    assert rdice.shape == (B, C) and all(np.array_equal(rdice[0], row) for row in rdice)
    np.testing.assert_allclose(rdice[0], dice.detach().numpy(), **TOL)
    np.testing.assert_allclose(rgrad, tz.grad.numpy(), **TOL)
    if B >= 3:
        assert not rgrad[1].any()                                                # the sample without a valid voxel
    if C >= 4 and smooth == 0.0:
        assert rdice[0, C - 2] == 0                                              # absent from the whole batch under smooth = 0


def test_one_sample_is_the_per_sample_loss_and_two_samples_are_not():
    rng = np.random.RandomState(4)
    z, y = rng.normal(size=(1, 5, 60)) * 3, rng.randint(0, 5, size=(1, 60))
    a, b = batch_dice_ref.dice_ce_batch(z, y), loss_ref.dice_ce(z, y)
    np.testing.assert_allclose(a[0], b[0], **TOL)
    np.testing.assert_allclose(a[1], b[1], **TOL)
    np.testing.assert_allclose(a[2], b[2], **TOL)
    y = rng.randint(0, 4, size=(2, 60))
    y[0, :10] = 4                                                                # class 4 in sample 0 only
    z = rng.normal(size=(2, 5, 60)) + 6.0 * (np.arange(5)[None, :, None] == y[:, None, :])          # a net that is mostly right
    (lb, ceb, _), db, _ = batch_dice_ref.dice_ce_batch(z, y)
    (ls, ces, _), ds, _ = loss_ref.dice_ce(z, y)
    # per sample the class costs sample 1 a Dice near 0 (nothing to find, some probability spent); pooled it is found
    assert ceb == ces and ds[1, 4] < 0.01 and ds[0, 4] > 0.9 and db[0, 4] > 0.9 and ls - lb > 0.1


def test_batch_dice_with_the_whole_batch_ignored():
    z = np.random.RandomState(0).normal(size=(2, 4, 10))
    (loss, ce, dl), dice, grad = batch_dice_ref.dice_ce_batch(z, np.full((2, 10), -1), 1e-5, False)
    assert ce == 0 and (dice == 1).all() and loss == -1 and dl == -1 and not grad.any()
    (_, _, dl0), dice0, grad0 = batch_dice_ref.dice_ce_batch(z, np.full((2, 10), 4), 0.0, True)
    assert (dice0 == 0).all() and dl0 == 0 and not grad0.any()


@pytest.mark.parametrize("strides", [(2, 2, 2), (1, 2, 2), (1, 1, 1)])
def test_batch_dice_strided_labels_are_plain_slicing(strides):
    rng = np.random.RandomState(sum(strides))
    d, h, w = 4, 6, 8
    sd, sh, sw = strides
    full = _labels(rng, 2, 5, (d * sd, h * sh, w * sw))
    low = np.ascontiguousarray(full[:, sd // 2::sd, sh // 2::sh, sw // 2::sw])
    z = rng.normal(size=(2, 5, d, h, w))
    a = batch_dice_ref.dice_ce_batch(z, full, 1e-5, False, strides)
    b = batch_dice_ref.dice_ce_batch(z.reshape(2, 5, -1), low.reshape(2, -1), 1e-5, False)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2].reshape(2, 5, -1), b[2]) and a[2].shape == z.shape
    tz = torch.tensor(z.reshape(2, 5, -1), requires_grad=True)
    loss, _, _, _ = _torch_batch_dice_ce(tz, torch.tensor(low.reshape(2, -1)), 1e-5, False)
    loss.backward()
    np.testing.assert_allclose(a[0][0], float(loss.detach()), **TOL)
    np.testing.assert_allclose(a[2].reshape(2, 5, -1), tz.grad.numpy(), **TOL)


# ------------------------------------------------------------------------------------------------ host logic of the trainer
def test_ema_first_value_nan_epoch_and_strict_best():
    from dg_tta_amd.pretraining.trainer import ema_step, is_new_best
    nan = float("nan")
    assert ema_step(None, 0.4) == 0.4                                            # the first finite value starts the average
    assert ema_step(None, nan) is None and ema_step(nan, nan) is None            # nothing to start from yet
    assert ema_step(nan, 0.25) == 0.25                                           # (a logged NaN is "no average yet")
    assert ema_step(0.4, nan) == 0.4                                             # a NaN epoch leaves it unchanged
    assert ema_step(0.4, 0.8) == 0.9 * 0.4 + 0.1 * 0.8
    assert is_new_best(0.4, None) and not is_new_best(None, None) and not is_new_best(nan, None)
    assert not is_new_best(0.4, 0.4) and is_new_best(math.nextafter(0.4, 1.0), 0.4) and not is_new_best(0.3, 0.4)


def test_ema_series_is_rebuilt_from_an_old_log():
    """A checkpoint from before the rule has mean_fg_dice only: the series and the best a continued run starts from."""
    from dg_tta_amd.pretraining.trainer import best_of, ema_step, is_new_best, rebuild_ema
    nan = float("nan")
    old = [nan, 0.5, nan, 0.7, 0.1, 0.9]
    series, best = rebuild_ema(old)
    e1 = 0.5
    e3 = 0.9 * e1 + 0.1 * 0.7
    e4 = 0.9 * e3 + 0.1 * 0.1
    e5 = 0.9 * e4 + 0.1 * 0.9
    assert math.isnan(series[0]) and series[1:] == [e1, e1, e3, e4, e5]
    assert best == max(e1, e3, e4, e5) == best_of(series) and e4 < e3
    # the same series, epoch by epoch, as the loop keeps it; the epochs that write checkpoint_best.pth
    log, b, wrote = [], None, []
    for epoch, v in enumerate(old):
        ema = ema_step(log[-1] if log else None, v)
        log.append(nan if ema is None else ema)
        if is_new_best(ema, b):
            b = ema
            wrote.append(epoch)
    assert log[1:] == series[1:] and b == best and wrote == [1, 3, 5]
    assert rebuild_ema([]) == ([], None) and best_of([nan, nan]) is None and rebuild_ema([nan])[1] is None


def test_plans_batch_dice_follows_inherits_from_and_defaults_to_false():
    from dg_tta_amd.pretraining.trainer import BATCH_DICE_NOTE, plans_batch_dice
    plans = {"configurations": {"3d_fullres": {"batch_dice": True, "patch_size": [8, 8, 8]},
                                "child": {"inherits_from": "3d_fullres", "patch_size": [4, 4, 4]},
                                "override": {"inherits_from": "child", "batch_dice": False},
                                "2d": {"patch_size": [8, 8]}}}
    assert plans_batch_dice(plans, "3d_fullres") is True and plans_batch_dice(plans, "child") is True
    assert plans_batch_dice(plans, "override") is False and plans_batch_dice(plans, "2d") is False
    assert "batch_dice: true" in BATCH_DICE_NOTE and "--dice plans" in BATCH_DICE_NOTE and "per sample" in BATCH_DICE_NOTE


def test_pretrain_parser_takes_dice_validate_and_val():
    from dg_tta_amd.pretraining import trainer
    from dg_tta_amd.run import DGTTAProgram
    base = ["802", "3d_fullres", "0", "-tr", "nnUNetTrainer_GIN"]
    parser = DGTTAProgram._pretrain_parser()
    args = parser.parse_args(base)
    assert args.dice == "sample" and args.validate is False and args.validation_only is False
    args = parser.parse_args(base + ["--dice", "plans", "--validate"])
    assert args.dice == "plans" and args.validate is True and args.validation_only is False
    assert parser.parse_args(base + ["--val"]).validation_only is True
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--dice", "batch"])
    with pytest.raises(ValueError, match="sample, plans"):
        trainer.train_fold("802", "3d_fullres", 0, "nnUNetTrainer_GIN", dice="batch")
