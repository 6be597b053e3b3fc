"""CPU: tests/sgd_ref.py (the float64 restatement the GPU tests of csrc/sgd.hip compare with) against
torch.nn.utils.clip_grad_norm_ + torch.optim.SGD in float64, PolyLRScheduler against its formula, and the host logic of
`dgtta pretrain`: centre voxel -> patch offset, the forced-foreground rule, the 5-fold split, argument parsing."""
import numpy as np
import pytest
import torch

import sgd_ref


@pytest.mark.parametrize("nesterov", [True, False])
@pytest.mark.parametrize("gscale,max_norm", [(30.0, 12.0), (0.1, 12.0), (30.0, None)])     # clipping active / inactive / off
def test_sgd_ref_matches_torch_float64(nesterov, gscale, max_norm):
    """Five steps; the middle parameter never has a gradient (skipped, outside the norm), the last one gets its first
    gradient at step 2 (its first step comes later than the others')."""
    rng = np.random.RandomState(3)
    shapes = [(7,), (3, 5), (4,), (2, 3, 2)]
    p0 = [rng.normal(size=s) for s in shapes]
    tp = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in p0]
    opt = torch.optim.SGD(tp, lr=0.05, momentum=0.9, nesterov=nesterov, weight_decay=1e-2)
    rp, rb = [p.copy() for p in p0], [None] * 4
    for step in range(5):
        grads = [rng.normal(size=s) * gscale for s in shapes]
        grads[1] = None
        if step < 2:
            grads[3] = None
        for t, g in zip(tp, grads):
            t.grad = None if g is None else torch.tensor(g, dtype=torch.float64)
        if max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_(tp, max_norm)
            assert (float(total) > max_norm) == (gscale > 1)
        opt.step()
        rp, rb, coef = sgd_ref.sgd_step(rp, grads, rb, lr=0.05, momentum=0.9, weight_decay=1e-2, nesterov=nesterov,
                                        max_norm=max_norm)
        assert (coef < 1.0) == (max_norm is not None and gscale > 1)
        for t, r in zip(tp, rp):
            np.testing.assert_allclose(t.detach().numpy(), r, rtol=1e-13, atol=1e-14)
        for t, b in zip(tp, rb):
            tb = opt.state[t].get("momentum_buffer")
            assert (tb is None) == (b is None)
            if b is not None:
                np.testing.assert_allclose(tb.numpy(), b, rtol=1e-13, atol=1e-14)
    assert rb[1] is None and np.array_equal(rp[1], p0[1])


def test_sgd_ref_divides_the_loss_scale_out():
    rng = np.random.RandomState(1)
    p, g = [rng.normal(size=9)], [rng.normal(size=9) * 40]
    a = sgd_ref.sgd_step(p, g, [None], lr=0.01)
    b = sgd_ref.sgd_step(p, [g[0] * 1024], [None], lr=0.01, grad_scale=1024.0)
    np.testing.assert_allclose(a[0][0], b[0][0], rtol=1e-15)
    assert a[2] == pytest.approx(b[2], rel=1e-15) and a[2] < 1


def test_poly_lr_scheduler_matches_its_formula():
    from dg_tta_amd.optim import PolyLRScheduler
    p = [torch.zeros(3, requires_grad=True)], [torch.zeros(2, requires_grad=True)]
    opt = torch.optim.SGD([{"params": p[0]}, {"params": p[1], "lr": 0.5}], lr=0.3)
    sched = PolyLRScheduler(opt, 1e-2, 1000)
    for step in (0, 1, 999):
        lr = sched.step(step)
        want = 1e-2 * (1 - step / 1000) ** 0.9
        assert lr == want == sgd_ref.poly_lr(1e-2, step, 1000) and [g["lr"] for g in opt.param_groups] == [want, want]
    assert sched.step(0) == 1e-2
    assert PolyLRScheduler(opt, 1e-2, 2).step(1) == 1e-2 * 0.5 ** 0.9
    assert PolyLRScheduler(opt, 2.0, 10, exponent=2.0).step(5) == 0.5


def test_hip_sgd_refuses_cpu_tensors():
    from dg_tta_amd import ops
    from dg_tta_amd._lib import DgttaError
    from dg_tta_amd.optim import HipSGD
    p = torch.zeros(5, requires_grad=True)
    p.grad = torch.ones(5)
    opt = HipSGD([p])
    assert opt.defaults["lr"] == 1e-2 and opt.defaults["momentum"] == 0.99 and opt.defaults["nesterov"] is True
    assert opt.defaults["weight_decay"] == 3e-5 and opt.max_grad_norm == 12.0 and opt.grad_scale == 1.0
    with pytest.raises(DgttaError):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(5)) and "momentum_buffer" not in opt.state[p]
    with pytest.raises(DgttaError):
        ops.grad_sumsq([torch.ones(4)])
    with pytest.raises(DgttaError):
        ops.sgd_step([torch.ones(4)], [torch.ones(4)], [torch.ones(4)], 1e-2)
    with pytest.raises(ValueError):
        HipSGD([p], momentum=0.0, nesterov=True)


def test_center_to_offset_exact_crop_and_clamping():
    """The offset goes into get_batch's affine (align_corners=False): output voxel i of a patch of P voxels reads source
    position (c + 1) S / 2 + i - P / 2 - restated here - which must be the INTEGER start + i of nnU-Net's crop."""
    from dg_tta_amd.tta.torch_utils import center_to_offset
    shape, patch = (40, 33, 64), (16, 16, 32)

    def starts(center):
        off = center_to_offset(center, shape, patch)
        return [(c + 1) * s / 2 - p / 2 for c, s, p in zip(off, shape, patch)]
    assert starts((20, 16, 32)) == pytest.approx([12, 8, 16], abs=1e-9)             # middle: centre - P // 2
    assert starts((9, 25, 17)) == pytest.approx([1, 17, 1], abs=1e-9)
    for axis in range(3):                                                         # each face: clamped to [0, S - P]
        lo, hi = [20, 16, 32], [20, 16, 32]
        lo[axis], hi[axis] = 0, shape[axis] - 1
        want_lo, want_hi = [12, 8, 16], [12, 8, 16]
        want_lo[axis], want_hi[axis] = 0, shape[axis] - patch[axis]
        assert starts(lo) == pytest.approx(want_lo, abs=1e-9) and starts(hi) == pytest.approx(want_hi, abs=1e-9)
    # offsets stay inside the range get_batch's random draw covers
    for c in ((0, 0, 0), (39, 32, 63)):
        assert all(abs(o) <= (s - p) / s + 1e-12 for o, s, p in zip(center_to_offset(c, shape, patch), shape, patch))
    # a volume not larger than the patch along an axis: the centred patch
    assert center_to_offset((3, 3, 3), (16, 10, 64), (16, 16, 32))[:2] == [0.0, 0.0]


def test_forced_foreground_rule():
    from dg_tta_amd.pretraining.trainer import is_forced_foreground
    assert [is_forced_foreground(j, 2) for j in range(2)] == [False, True]
    assert [is_forced_foreground(j, 3) for j in range(3)] == [False, False, True]
    assert [is_forced_foreground(j, 4) for j in range(4)] == [False, False, False, True]


def test_class_locations_and_center_draw():
    from dg_tta_amd.pretraining.trainer import class_locations, draw_center
    seg = np.zeros((6, 7, 8), np.int8)
    seg[1:3, 2:4, 5] = 2
    seg[4, 4, 1:4] = 5
    seg[0, 0, 0] = -1
    loc = class_locations(seg)
    assert sorted(loc) == [2, 5] and len(loc[2]) == 4 and len(loc[5]) == 3
    assert all(seg[tuple(v)] == c for c, vox in loc.items() for v in vox)
    big = np.ones((30, 30, 30), np.int8)
    capped = class_locations(big, max_per_class=100)[1]
    assert capped.shape == (100, 3) and len({tuple(v) for v in capped}) == 100
    assert np.array_equal(capped, class_locations(big, max_per_class=100)[1])          # drawn once, seeded
    rs = np.random.RandomState(0)
    seen = {int(seg[draw_center(loc, rs)]) for _ in range(40)}
    assert seen == {2, 5}
    assert draw_center({}, rs) is None


def test_five_fold_split_is_a_partition():
    from dg_tta_amd.pretraining.trainer import make_splits
    names = [f"case_{i:03d}" for i in range(23)]
    splits = make_splits(list(reversed(names)))
    assert len(splits) == 5 and splits == make_splits(names)
    vals = [set(s["val"]) for s in splits]
    assert set().union(*vals) == set(names) and sum(len(v) for v in vals) == 23
    assert sorted(len(v) for v in vals) == [4, 4, 5, 5, 5]
    for s in splits:
        assert set(s["train"]) | set(s["val"]) == set(names) and not set(s["train"]) & set(s["val"])
    three = make_splits(["a", "b", "c"])
    assert [len(s["val"]) for s in three] == [1, 1, 1, 0, 0] and len(three[0]["train"]) == 2


def test_pretrain_cli_arguments():
    from dg_tta_amd.run import DGTTAProgram
    parser = DGTTAProgram._pretrain_parser()
    a = parser.parse_args(["802", "3d_fullres", "0", "-tr", "nnUNetTrainer_GIN_MIND"])
    assert (a.dataset_id, a.configuration, a.fold, a.trainer) == ("802", "3d_fullres", "0", "nnUNetTrainer_GIN_MIND")
    assert (a.num_epochs, a.iterations_per_epoch, a.val_iterations) == (1000, 250, 50)
    assert a.device == "cuda" and a.dtype == "fp32" and a.continue_training is False and a.seed is None
    b = parser.parse_args(["Dataset802_Source", "3d_fullres", "all", "-tr", "nnUNetTrainer_MIND_MultiRes", "--num_epochs", "3",
                           "--iterations_per_epoch", "4", "--val_iterations", "1", "--device", "cuda:1", "--dtype", "fp16", "--c",
                           "--seed", "9"])
    assert (b.fold, b.trainer, b.num_epochs, b.iterations_per_epoch, b.val_iterations) == ("all", "nnUNetTrainer_MIND_MultiRes", 3, 4, 1)
    assert b.device == "cuda:1" and b.dtype == "fp16" and b.continue_training is True and b.seed == 9
    for bad in (["802", "3d_fullres", "0"], ["802", "3d_fullres", "0", "-tr", "nnUNetTrainer"],
                ["802", "3d_fullres", "0", "-tr", "nnUNetTrainer_GIN", "--dtype", "fp8"]):
        with pytest.raises(SystemExit):
            parser.parse_args(bad)
    with pytest.raises(SystemExit):
        DGTTAProgram(["dgtta", "pretrain", "802", "3d_fullres", "zero", "-tr", "nnUNetTrainer_GIN"])


def test_pretrain_says_when_the_plans_are_missing(tmp_path, monkeypatch):
    from dg_tta_amd.pretraining.trainer import load_dataset_files
    for k in ("nnUNet_raw", "nnUNet_preprocessed", "nnUNet_results"):
        monkeypatch.setenv(k, str(tmp_path / k))
    (tmp_path / "nnUNet_preprocessed" / "Dataset802_Source").mkdir(parents=True)
    with pytest.raises(FileNotFoundError, match="no experiment planning"):
        load_dataset_files("Dataset802_Source")
