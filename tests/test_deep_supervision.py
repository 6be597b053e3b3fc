"""Deep supervision, host side (no GPU): the weights of the multi-scale loss, the shape checks of ops.deep_supervision_loss,
the flag's default on a fresh network and on one that load_network builds."""
import inspect
import json
import os
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_default_weights_are_nnunets(n):
    """2^-i, the lowest resolution set to 0, normalised to sum 1 (5 outputs: [8, 4, 2, 1, 0] / 15)."""
    from dg_tta_amd.ops import deep_supervision_weights
    raw = [2.0 ** -i for i in range(n)]
    raw[-1] = 0.0
    want = [r / sum(raw) for r in raw]
    got = deep_supervision_weights(n)
    assert len(got) == n and got[-1] == 0.0 and abs(sum(got) - 1.0) < 1e-12
    assert all(abs(a - b) < 1e-15 for a, b in zip(got, want))
    if n == 5:
        assert all(abs(a - b / 15.0) < 1e-15 for a, b in zip(got, [8, 4, 2, 1, 0]))


def test_loss_raises_on_shapes_that_do_not_divide():
    """The strides follow from the shapes; a shape that does not divide the label map is an error before anything is launched
    (CPU tensors get this far)."""
    from dg_tta_amd import ops
    labels = torch.zeros(2, 1, 8, 16, 24, dtype=torch.int64)
    ok = torch.zeros(2, 3, 8, 16, 24)
    with pytest.raises(ValueError, match="does not divide"):
        ops.deep_supervision_loss([ok, torch.zeros(2, 3, 4, 8, 9)], labels)
    with pytest.raises(ValueError, match="does not divide"):
        ops.deep_supervision_loss([ok, torch.zeros(2, 3, 3, 8, 12)], labels[:, 0])
    with pytest.raises(ValueError, match="weights"):
        ops.deep_supervision_loss([ok, torch.zeros(2, 3, 4, 8, 12)], labels, weights=[1.0])
    assert ops._label_strides((4, 8, 12), (8, 16, 24)) == (2, 2, 2) and ops._label_strides((8, 8, 12), (8, 16, 24)) == (1, 2, 2)


def test_flag_defaults_off_and_is_a_plain_attribute():
    from dg_tta_amd.pretraining.supervised import pretrain_supervised
    from dg_tta_amd.unet import HipPlainConvUNet
    cfg = dict(features=(4, 8), strides=(1, 2), n_conv_enc=(1, 1), n_conv_dec=(1,), in_channels=12, num_classes=3)
    net = HipPlainConvUNet(cfg)
    assert net.deep_supervision is False
    assert HipPlainConvUNet(cfg, deep_supervision=True).deep_supervision is True
    net.deep_supervision = True          # toggled after construction, as nnU-Net's decoder.deep_supervision
    assert "deep_supervision" not in net.state_dict() and not any("deep_supervision" in k for k in net.state_dict())
    # the fusion contexts know one head: refused under the flag
    with pytest.raises(ValueError, match="deep_supervision"):
        net.fuse_output_warp(torch.zeros(1, 3, 4), torch.zeros(1, 3, 4))
    with pytest.raises(ValueError, match="deep_supervision"):
        net.fuse_window_accumulate(torch.zeros(4, 4, 4, 3), torch.zeros(4, 4, 4), torch.zeros(2, 2, 2), [(0, 0, 0)])
    with pytest.raises(ValueError, match="deep_supervision"):
        net.fuse_window_feature_accumulate(torch.zeros(4, 4, 4, 32), torch.zeros(4, 4, 4), torch.zeros(2, 2, 2), [(0, 0, 0)])
    assert inspect.signature(pretrain_supervised).parameters["deep_supervision"].default is False


def test_load_network_keeps_deep_supervision_off(tmp_path, monkeypatch):
    """Inference and TTA build the network the way nnUNetPredictor does: one output."""
    from dg_tta_amd.tta import nnunet_utils as nu
    from dg_tta_amd.unet import HipPlainConvUNet
    skel = ROOT / "dg_tta_amd" / "__resources__" / "model_skeleton"
    plans, ds = json.load(open(skel / "plans.json")), json.load(open(skel / "dataset.json"))
    plans["configurations"]["3d_fullres"].update(
        UNet_base_num_features=4, unet_max_num_features=8, n_conv_per_stage_encoder=[1, 1], n_conv_per_stage_decoder=[1],
        pool_op_kernel_sizes=[[1, 1, 1], [2, 2, 2]], conv_kernel_sizes=[[3, 3, 3], [3, 3, 3]], patch_size=[16, 16, 16])
    folder = tmp_path / "res" / "DatasetX" / "nnUNetTrainer_GIN_MIND__nnUNetPlans__3d_fullres"
    (folder / "fold_0").mkdir(parents=True)
    json.dump(plans, open(folder / "plans.json", "w"))
    json.dump(ds, open(folder / "dataset.json", "w"))
    cfg, _ = nu.unet_cfg_from_plans(plans, ds, "3d_fullres", 12)
    ref = HipPlainConvUNet(cfg)
    for p in ref.parameters():
        torch.nn.init.normal_(p)
    torch.save({"network_weights": ref.state_dict(), "trainer_name": "nnUNetTrainer_GIN_MIND"},
               folder / "fold_0" / "checkpoint_final.pth")
    monkeypatch.setenv("DG_TTA_INTERNAL_AUGMENTATION", os.environ.get("DG_TTA_INTERNAL_AUGMENTATION", "false"))
    _, _, net, _ = nu.load_network(folder / "fold_0" / "checkpoint_final.pth", "cpu")
    assert net.deep_supervision is False
