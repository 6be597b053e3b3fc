"""Mirroring for the stock nnUNetTrainer, CPU side: the float64 restatement (tests/mirror_ref.py) checked on its own, and the host
logic of the trainer registry, the CLI, the fp16 refusal and the training draws."""
import numpy as np
import pytest
import torch

import mirror_ref as mr

DG_NAMES = tuple(f"nnUNetTrainer_{n}{m}" for m in ("", "_MultiRes") for n in ("GIN", "MIND", "GIN_MIND"))


def _box(x):
    """A flip-equivariant function: a symmetric 3^3 box filter with zero padding."""
    return torch.nn.functional.avg_pool3d(x, 3, stride=1, padding=1, count_include_pad=True)


def test_subset_order_and_counts():
    assert [len(mr.subsets(a)) for a in (None, (1,), (0, 2), (0, 1, 2))] == [1, 2, 4, 8]
    assert mr.subsets((0, 1, 2)) == [(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]
    assert mr.subsets((0, 2)) == [(), (0,), (2,), (0, 2)] and mr.subsets((2,)) == [(), (2,)]
    assert [mr.mask_of(s) for s in mr.subsets((0, 1, 2))] == [0, 1, 2, 4, 3, 5, 6, 7]
    assert all(mr.axes_of(mr.mask_of(s)) == s for s in mr.SUBSET_ORDER)
    from dg_tta_amd import ops
    for axes in (None, (2,), (0, 2), (1, 2), (0, 1, 2)):           # the product's work list uses the same order
        assert ops.mirror_masks(axes) == [mr.mask_of(s) for s in mr.subsets(axes)]
    assert ops.mirror_masks(()) == [0] and ops.mirror_masks([2, 0]) == [0, 1, 4, 5]
    for bad in ((3,), (0, 0), (-1,)):
        with pytest.raises(ValueError):
            ops.mirror_masks(bad)


def test_mean_over_mirrors_of_an_equivariant_function_is_the_function():
    torch.manual_seed(0)
    x = torch.randn(1, 2, 5, 6, 8, dtype=torch.float64)
    for axes in ((0, 1, 2), (1,), (0, 2)):
        assert torch.allclose(mr.mirrored(_box, axes)(x), _box(x), atol=1e-14, rtol=0)
    shift = lambda t: t.roll(1, -1)                               # NOT equivariant: the mirrored mean must differ
    assert not torch.allclose(mr.mirrored(shift, (2,))(x), shift(x), atol=1e-3)
    both = 0.5 * (shift(x) + shift(x.flip(-1)).flip(-1))
    assert torch.allclose(mr.mirrored(shift, (2,))(x), both, atol=1e-14, rtol=0)


def test_gather_and_accumulate_restatement_and_the_flipped_gaussian_guard():
    torch.manual_seed(1)
    P, V = (5, 6, 8), (9, 8, 13)
    vol = torch.randn(2, *V)
    origins, masks = [(0, 0, 0), (2, 1, 3), (4, 2, 5)], [5, 0, 7]
    w = mr.gather(vol, origins, masks, P)
    assert tuple(w.shape) == (3, 2, *P)
    assert w[0, 1, 1, 2, 3] == vol[1, 0 + 4 - 1, 0 + 2, 0 + 8 - 1 - 3]              # mask 5: D and W flipped, H not
    assert torch.equal(w[1], vol[:, 2:7, 1:7, 3:11])
    assert w[2, 0, 0, 0, 0] == vol[0, 4 + 4, 2 + 5, 5 + 7]
    g = torch.rand(*P) + 0.1                                       # no symmetry at all
    z = torch.randn(*P, 3)
    def run(weight, mask):
        acc, nsum = torch.zeros(*V, 3, dtype=torch.float64), torch.zeros(*V, dtype=torch.float64)
        absacc, counts = torch.zeros_like(acc), torch.zeros(*V, dtype=torch.int64)
        mr.accumulate(acc, nsum, absacc, counts, weight, z, (2, 1, 3), mask)
        return acc, nsum, counts
    acc, nsum, counts = run(g, 7)
    # element by element: acc[o + p] = g[p] * z[flip(p)]
    p = (1, 4, 2)
    assert torch.equal(acc[2 + 1, 1 + 4, 3 + 2], g[p].double() * z[5 - 1 - 1, 6 - 1 - 4, 8 - 1 - 2].double())
    assert torch.equal(nsum[2:7, 1:7, 3:11], g.double()) and int(counts.sum()) == 5 * 6 * 8
    # the guard: weighting with the flipped Gaussian is a DIFFERENT accumulator (what the kernels must not do)
    wrong, wrong_n, _ = run(g.flip(0, 1, 2), 7)
    assert not torch.allclose(acc, wrong) and not torch.allclose(nsum, wrong_n)
    # ... and so is it for nnU-Net's own map at even tile sizes (centred at i // 2)
    from dg_tta_amd.tta.inference import compute_gaussian
    cg = compute_gaussian((6, 6, 8))
    assert not torch.allclose(cg, cg.flip(0, 1, 2))


def test_trainer_registry():
    from dg_tta_amd.gin import gin_hook
    from dg_tta_amd.mind import mind_hook
    from dg_tta_amd.pretraining import hooks, trainer
    from dg_tta_amd.tta import nnunet_utils as nu
    assert nu.trainer_hooks("nnUNetTrainer") == (1, []) and hooks.trainer_spec("nnUNetTrainer") == (1, [])
    assert nu.trainer_mirror_axes("nnUNetTrainer") == (0, 1, 2) and hooks.trainer_mirror_axes("nnUNetTrainer") == (0, 1, 2)
    for name in DG_NAMES:
        assert nu.trainer_mirror_axes(name) is None
        assert nu.trainer_hooks(name) == hooks.trainer_spec(name) and len(nu.trainer_hooks(name)) == 2
    assert nu.trainer_hooks("nnUNetTrainer_GIN_MIND_MultiRes") == (12, [gin_hook, mind_hook])
    assert nu.trainer_hooks("nnUNetTrainer_GIN") == (1, [gin_hook]) and nu.trainer_hooks("nnUNetTrainer_MIND") == (12, [mind_hook])
    for other in ("nnUNetTrainerNoMirroring", "nnUNetTrainer_5epochs", "xnnUNetTrainer", "nnUNetTrainerV2"):
        for fn in (nu.trainer_hooks, nu.trainer_mirror_axes, hooks.trainer_spec):
            with pytest.raises(NotImplementedError):
                fn(other)
    assert trainer.DG_TRAINERS == DG_NAMES and trainer.TRAINERS == DG_NAMES + ("nnUNetTrainer",)


def test_no_hooks_leaves_the_internal_augmentation_off():
    from dg_tta_amd.pretraining.hooks import register_dg_hooks
    from dg_tta_amd.utils import disable_internal_augmentation, get_internal_augmentation_enabled
    net = torch.nn.Conv3d(1, 1, 1)
    disable_internal_augmentation()
    assert register_dg_hooks(net, "nnUNetTrainer") == [] and not get_internal_augmentation_enabled()
    handles = []
    try:
        handles = register_dg_hooks(net, "nnUNetTrainer_GIN")
        assert len(handles) == 1 and get_internal_augmentation_enabled()
    finally:
        for h in handles:
            h.remove()
        disable_internal_augmentation()


def test_pretrain_parser_takes_the_stock_trainer():
    from dg_tta_amd.run import DGTTAProgram
    from dg_tta_amd.pretraining.trainer import TRAINERS
    parser = DGTTAProgram._pretrain_parser(TRAINERS)            # what the `pretrain` command parses with
    args = parser.parse_args(["802", "3d_fullres", "0", "-tr", "nnUNetTrainer"])
    assert args.trainer == "nnUNetTrainer"
    assert parser.parse_args(["802", "3d_fullres", "0", "-tr", "nnUNetTrainer_GIN"]).trainer == "nnUNetTrainer_GIN"
    with pytest.raises(SystemExit):
        parser.parse_args(["802", "3d_fullres", "0", "-tr", "nnUNetTrainerNoMirroring"])
    # the command itself: the trainer name is taken, the run stops at the fold check that follows the parse
    with pytest.raises(SystemExit, match="neither a number"):
        DGTTAProgram(["dgtta", "pretrain", "802", "3d_fullres", "zero", "-tr", "nnUNetTrainer"])
    with pytest.raises(SystemExit) as bad:
        DGTTAProgram(["dgtta", "pretrain", "802", "3d_fullres", "zero", "-tr", "nnUNetTrainerNoMirroring"])
    assert bad.value.code == 2                                  # argparse's own refusal, before the fold check


def test_fp16_logits_accumulator_refuses_mirroring(monkeypatch):
    """Before memory is allocated (and before a device is needed): eight passes per window leave no headroom in half."""
    from conftest import SMALL_CFG
    from dg_tta_amd.tta.inference import predict_ensemble_logits, predict_sliding_window_return_logits
    from dg_tta_amd.unet import HipPlainConvUNet
    net = HipPlainConvUNet(SMALL_CFG)
    x = torch.zeros(1, 16, 16, 16)
    with pytest.raises(ValueError, match="headroom"):
        predict_sliding_window_return_logits(net, x, [16, 16, 16], acc_dtype=torch.float16, mirror_axes=(0, 1, 2))
    monkeypatch.setenv("DGTTA_WINDOW_ACC", "fp16")
    with pytest.raises(ValueError, match="headroom"):
        predict_ensemble_logits(x, net, [net.state_dict()], [16, 16, 16], mirror_axes=(2,))
    with pytest.raises(ValueError, match="subset"):
        predict_sliding_window_return_logits(net, x, [16, 16, 16], acc_dtype=torch.float32, mirror_axes=(3,))
    with pytest.raises(ValueError, match="fp32"):
        net.fuse_window_accumulate(torch.zeros(2, 2, 2, 9, dtype=torch.float16), torch.zeros(2, 2, 2), torch.zeros(2, 2, 2),
                                   [(0, 0, 0)], mirrors=[3])
    for bad in ([8], [0, 0]):
        with pytest.raises(ValueError, match="mirror mask"):
            net.fuse_window_feature_accumulate(torch.zeros(2, 2, 2, 32), torch.zeros(2, 2, 2), torch.zeros(2, 2, 2), [(0, 0, 0)],
                                               mirrors=bad)


def test_training_mask_draws_item_major_axis_zero_first():
    from dg_tta_amd.pretraining.trainer import draw_mirror_masks
    from dg_tta_amd.utils import numpy_rng
    np.random.seed(5)
    st = numpy_rng().get_state()
    masks = draw_mirror_masks(4, (0, 1, 2), numpy_rng())
    after = numpy_rng().get_state()
    numpy_rng().set_state(st)
    u = [numpy_rng().uniform() for _ in range(12)]                # one uniform per (item, axis), item-major, axis 0 first
    assert masks == [sum(1 << a for a in range(3) if u[3 * b + a] < 0.5) for b in range(4)]
    assert all(np.array_equal(x, y) for x, y in zip(after, numpy_rng().get_state()) if isinstance(x, np.ndarray))
    assert len(set(masks)) > 1 and all(0 <= m <= 7 for m in masks)
    numpy_rng().set_state(st)
    two = draw_mirror_masks(3, (1, 2), numpy_rng())               # a subset: only its axes draw
    numpy_rng().set_state(st)
    u = [numpy_rng().uniform() for _ in range(6)]
    assert two == [sum(1 << a for k, a in enumerate((1, 2)) if u[2 * b + k] < 0.5) for b in range(3)]
    # a DG trainer draws nothing: its stream does not move
    numpy_rng().set_state(st)
    assert draw_mirror_masks(4, None, numpy_rng()) == [0, 0, 0, 0]
    assert numpy_rng().uniform() == u[0]
