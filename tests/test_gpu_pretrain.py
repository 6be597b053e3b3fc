"""GPU: source-domain pre-training with nnU-Net's optimiser (optim.HipSGD + PolyLRScheduler, csrc/sgd.hip): the small
atlas task of tests/test_pretraining.py through `pretrain_supervised(optimizer=HipSGD(...))`, and the command line end to
end on a synthetic source dataset - `dgtta pretrain` -> `dgtta prepare_tta` -> `dgtta run_tta` without nnunetv2."""
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]

ATLAS_STEPS, ATLAS_CHUNKS = 200, 10          # the poly schedule is stepped once per chunk of 20 steps


def _train_atlas(steps, chunks):
    from conftest import SMALL_CFG
    from dg_tta_amd.optim import HipSGD, PolyLRScheduler
    from dg_tta_amd.pretraining.hooks import register_dg_hooks
    from dg_tta_amd.pretraining.supervised import pretrain_supervised
    from dg_tta_amd.synthetic import atlas_case, he_init_
    from dg_tta_amd.unet import HipPlainConvUNet
    cases = [atlas_case(24, 4, s, "source") for s in range(6)]
    lut = torch.tensor([0, 3, 8, 2, 5])
    net = he_init_(HipPlainConvUNet(SMALL_CFG), seed=7)
    handles = register_dg_hooks(net, "nnUNetTrainer_GIN_MIND")
    net = net.to(DEV)
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    np.random.seed(5)
    opt = HipSGD(net.parameters())                          # nnU-Net's defaults: 1e-2, 0.99 Nesterov, 3e-5, clip 12
    sched = PolyLRScheduler(opt, 1e-2, chunks)
    losses = []
    for c in range(chunks):
        sched.step(c)
        losses.append(pretrain_supervised(net, cases, [16, 16, 16], lut, steps=steps // chunks, batch=4, device=DEV, optimizer=opt))
    for h in handles:
        h.remove()
    return net, torch.cat(losses)


def test_pretrain_supervised_learns_the_atlas_task_with_hip_sgd():
    """The loss falls: the mean of the last tenth of the step losses is below the mean of the first tenth (that inequality
    only).  200 steps instead of the 400 of tests/test_pretraining.py: measured on an MI355X, the mean loss goes from 1.5730
    (steps 0-19) to 0.3935 (steps 180-199)."""
    from dg_tta_amd.tta.torch_utils import release_resident
    from dg_tta_amd.utils import disable_internal_augmentation
    try:
        net, losses = _train_atlas(ATLAS_STEPS, ATLAS_CHUNKS)
        n = ATLAS_STEPS // 10
        first, last = float(losses[:n].mean()), float(losses[-n:].mean())
        print(f"\nHipSGD + poly LR, {ATLAS_STEPS} steps: mean loss of the first tenth {first:.4f}, of the last tenth {last:.4f}")
        assert torch.isfinite(losses).all()
        assert last < first
    finally:
        disable_internal_augmentation()
        release_resident()


def test_pretrain_supervised_with_hip_sgd_is_reproducible():
    from dg_tta_amd.tta.torch_utils import release_resident
    from dg_tta_amd.utils import disable_internal_augmentation
    try:
        (a, la), (b, lb) = _train_atlas(12, 2), _train_atlas(12, 2)
        assert torch.equal(la, lb)
        from conftest import SMALL_CFG
        from dg_tta_amd.synthetic import he_init_
        from dg_tta_amd.unet import HipPlainConvUNet
        init = he_init_(HipPlainConvUNet(SMALL_CFG), seed=7).state_dict()
        moved = 0
        for (k, v), w in zip(a.state_dict().items(), b.state_dict().values()):
            assert torch.equal(v, w), k
            moved += int(not torch.equal(v.cpu(), init[k]))
        assert moved > 30
    finally:
        disable_internal_augmentation()
        release_resident()


def test_get_batch_with_a_centre_is_the_integer_crop():
    """get_batch(..., centers=): the patch around a voxel is the crop [start, start + patch) with nnU-Net's clamped start -
    labels (nearest) exactly, the image (trilinear at integer positions up to the rounding of the coordinates) within 1e-4
    of values ~ N(0, 1); an item without a centre still draws its random offset."""
    from dg_tta_amd.tta.torch_utils import as_label_map_case, get_batch, release_resident
    g = torch.Generator().manual_seed(3)
    shape, patch = (40, 33, 64), (16, 16, 32)
    img = torch.randn(shape, generator=g)
    lab = torch.randint(0, 7, shape, generator=g)
    case = as_label_map_case(img, lab)
    try:
        for center in [(20, 16, 32), (9, 25, 17), (0, 0, 0), (39, 32, 63), (0, 32, 31), (21, 0, 63)]:
            start = [min(max(c - p // 2, 0), s - p) for c, s, p in zip(center, shape, patch)]
            sl = tuple(slice(a, a + p) for a, p in zip(start, patch))
            ims, lbs = get_batch([case], [0], list(patch), None, DEV, centers=[center])
            assert ims[0].shape == (1, 1, *patch) and lbs[0].dtype == torch.int64
            assert torch.equal(lbs[0][0, 0].cpu(), lab[sl]), center
            assert (ims[0][0, 0].cpu() - img[sl]).abs().max() < 1e-4, center
        torch.manual_seed(1)
        a, _ = get_batch([case, case], [0, 1], list(patch), None, DEV, centers=[(20, 16, 32), None])
        torch.manual_seed(1)
        b, _ = get_batch([case], [0], list(patch), None, DEV)
        assert torch.equal(a[1], b[0]) and not torch.equal(a[0], a[1])
    finally:
        release_resident()


# ------------------------------------------------------------------------------------------------ the command line
def _write_case(folder_img, folder_lab, name, size, seed, spacing=(1.5, 1.5, 1.5)):
    from dg_tta_amd.synthetic import synthetic_case
    from dg_tta_amd.tta.nifti_io import write_nifti
    case = synthetic_case(size=size, k=3, seed=seed)
    img = (case[0] * 300.0).numpy().astype(np.float32)                # CT-like range for the plans' CTNormalization
    lab = torch.cat([(case[1:].sum(0, keepdim=True) < 1).float(), case[1:]]).argmax(0).numpy().astype(np.int16)
    write_nifti(folder_img / f"{name}_0000.nii.gz", img, spacing=spacing)
    write_nifti(folder_lab / f"{name}.nii.gz", lab, spacing=spacing)
    return lab


def _small_plans():
    """The skeleton's plans with the smallest topology whose bottleneck is still 4^3: patch 32^3, four stages."""
    plans = json.load(open(ROOT / "dg_tta_amd" / "__resources__" / "model_skeleton" / "plans.json"))
    plans["configurations"]["3d_fullres"].update(
        patch_size=[32, 32, 32], batch_size=2, n_conv_per_stage_encoder=[2, 2, 2, 2], n_conv_per_stage_decoder=[2, 2, 2],
        pool_op_kernel_sizes=[[1, 1, 1], [2, 2, 2], [2, 2, 2], [2, 2, 2]], conv_kernel_sizes=[[3, 3, 3]] * 4,
        num_pool_per_axis=[3, 3, 3])
    return plans


def test_pretrain_prepare_run_cli_chain(tmp_path, monkeypatch):
    from dg_tta_amd.pretraining.trainer import build_network
    from dg_tta_amd.run import DGTTAProgram
    from dg_tta_amd.tta.nifti_io import read_nifti
    from dg_tta_amd.tta.nnunet_utils import load_network
    raw, pre, res, root = tmp_path / "raw", tmp_path / "pre", tmp_path / "res", tmp_path / "dgroot"
    src = raw / "Dataset802_Source"
    (src / "imagesTr").mkdir(parents=True)
    (src / "labelsTr").mkdir()
    for i in range(3):
        _write_case(src / "imagesTr", src / "labelsTr", f"ct{i:02d}", 48, 11 + i)
    dataset_json = {"labels": {"background": 0, "liver": 1, "spleen": 2, "kidney": 3}, "file_ending": ".nii.gz",
                    "channel_names": {"0": "CT"}, "numTraining": 3}
    json.dump(dataset_json, open(src / "dataset.json", "w"))
    plans = _small_plans()
    (pre / "Dataset802_Source").mkdir(parents=True)
    json.dump(plans, open(pre / "Dataset802_Source" / "nnUNetPlans.json", "w"))
    root.mkdir()
    for k, v in {"nnUNet_raw": str(raw), "nnUNet_results": str(res), "nnUNet_preprocessed": str(pre), "DG_TTA_ROOT": str(root)}.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("DG_TTA_INTERNAL_AUGMENTATION", os.environ.get("DG_TTA_INTERNAL_AUGMENTATION", "false"))
    pretrain = ["dgtta", "pretrain", "802", "3d_fullres", "0", "-tr", "nnUNetTrainer_GIN_MIND", "--iterations_per_epoch", "3",
                "--val_iterations", "1", "--device", DEV, "--seed", "7"]
    DGTTAProgram(pretrain + ["--num_epochs", "2"])
    folder = res / "Dataset802_Source" / "nnUNetTrainer_GIN_MIND__nnUNetPlans__3d_fullres"
    final, latest = folder / "fold_0" / "checkpoint_final.pth", folder / "fold_0" / "checkpoint_latest.pth"
    assert (folder / "plans.json").is_file() and (folder / "dataset.json").is_file() and final.is_file() and latest.is_file()
    assert json.load(open(folder / "plans.json")) == plans and json.load(open(folder / "dataset.json")) == dataset_json
    data_dir = pre / "Dataset802_Source" / "nnUNetPlans_3d_fullres"
    assert sorted(p.name for p in data_dir.iterdir()) == ["ct00.npz", "ct01.npz", "ct02.npz"]
    with np.load(data_dir / "ct00.npz") as z:
        assert z["data"].shape == (1, 48, 48, 48) and z["seg"].shape == (1, 48, 48, 48) and set(np.unique(z["seg"]).tolist()) <= {-1, 0, 1, 2, 3}
    splits = json.load(open(pre / "Dataset802_Source" / "splits_final.json"))
    assert len(splits) == 5 and len(splits[0]["val"]) == 1 and len(splits[0]["train"]) == 2
    log_lines = (folder / "fold_0" / "training_log.txt").read_text().splitlines()
    assert len(log_lines) == 2 and log_lines[0].startswith("epoch 0 ") and log_lines[1].startswith("epoch 1 ")

    ck = torch.load(final, map_location="cpu", weights_only=False)
    assert set(ck) == {"network_weights", "optimizer_state", "current_epoch", "trainer_name", "init_args",
                       "inference_allowed_mirroring_axes", "logging", "grad_scaler_state"}
    assert ck["current_epoch"] == 2 and ck["trainer_name"] == "nnUNetTrainer_GIN_MIND" and ck["inference_allowed_mirroring_axes"] is None
    assert set(ck["init_args"]) == {"plans", "configuration", "fold", "dataset_json"} and ck["init_args"]["fold"] == 0
    assert ck["grad_scaler_state"] == {"scale": 1.0}
    log = ck["logging"]
    assert log["lrs"] == pytest.approx([1e-2, 1e-2 * 0.5 ** 0.9], rel=1e-15, abs=0)
    for key in ("train_losses", "val_losses", "mean_fg_dice"):
        assert len(log[key]) == 2
    assert np.isfinite(log["train_losses"] + log["val_losses"]).all()
    init, patch = build_network(plans, dataset_json, "3d_fullres", "nnUNetTrainer_GIN_MIND", seed=7)
    assert patch == [32, 32, 32] and init.cfg["features"] == (32, 64, 128, 256) and init.cfg["num_classes"] == 4
    _, lpatch, net, _ = load_network(final, "cpu")
    assert lpatch == [32, 32, 32] and set(net.state_dict()) == set(ck["network_weights"]) == set(init.state_dict())
    moved = sum(int(not torch.equal(ck["network_weights"][k], v)) for k, v in init.state_dict().items())
    assert moved > 30
    bufs = ck["optimizer_state"]["state"]
    assert len(bufs) > 30 and all(set(s) == {"momentum_buffer"} for s in bufs.values())

    # --c with one more epoch: exactly one more epoch runs
    DGTTAProgram(pretrain + ["--num_epochs", "3", "--c"])
    ck3 = torch.load(final, map_location="cpu", weights_only=False)
    assert ck3["current_epoch"] == 3 and len(ck3["logging"]["train_losses"]) == 3
    assert ck3["logging"]["lrs"] == pytest.approx(log["lrs"] + [1e-2 * (1 - 2 / 3) ** 0.9], rel=1e-15, abs=0)
    assert ck3["logging"]["train_losses"][:2] == log["train_losses"]
    assert len((folder / "fold_0" / "training_log.txt").read_text().splitlines()) == 3
    assert any(not torch.equal(ck3["network_weights"][k], v) for k, v in ck["network_weights"].items())

    # the chain the feature exists for: adapt the model just trained to a target dataset
    tgt = raw / "Dataset803_Target"
    (tgt / "imagesTs").mkdir(parents=True)
    (tgt / "labelsTs").mkdir()
    _write_case(tgt / "imagesTs", tgt / "labelsTs", "mr01", 40, 5)
    json.dump({"labels": {"background": 0, "liver": 1, "spleen": 2, "my_organ": 3}}, open(tgt / "dataset.json", "w"))
    common = ["802", "803", "--pretrainer", "nnUNetTrainer_GIN_MIND", "--pretrainer_config", "3d_fullres", "--pretrainer_fold", "0"]
    DGTTAProgram(["dgtta", "prepare_tta"] + common)
    plan_dir = root / "plans" / "Pretrained_Dataset802_Source_at_Dataset803_Target" / "nnUNetTrainer_GIN_MIND__3d_fullres" / "fold_0"
    plan = json.load(open(plan_dir / "tta_plan.json"))
    assert Path(plan["pretrained_weights_filepath"]) == final and plan["optimized_labels"] == ["background", "liver", "spleen"]
    plan.update(epochs=1, start_tta_at_epoch=0, patches_to_be_accumulated=4, ensemble_count=1)
    json.dump(plan, open(plan_dir / "tta_plan.json", "w"), indent=4)
    DGTTAProgram(["dgtta", "run_tta"] + common + ["--device", DEV])
    runs = sorted((root / "results" / "Pretrained_Dataset802_Source_at_Dataset803_Target" / "nnUNetTrainer_GIN_MIND__3d_fullres" /
                   "fold_0").iterdir())
    assert len(runs) == 1
    seg, hdr = read_nifti(runs[0] / "tta_outputTs" / "mr01.nii.gz")
    assert seg.shape == (40, 40, 40) and set(np.unique(seg).tolist()) <= {0, 1, 2}
