"""GPU: the chain `dgtta plan` exists for - from a raw dataset folder alone (no plans file) to a trained checkpoint.  Three
cases of 40^3 voxels with two labels: the planner's own 3d_fullres configuration is what `dgtta pretrain` trains."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _write_case(folder_img, folder_lab, name, size, seed, spacing):
    from dg_tta_amd.synthetic import synthetic_case
    from dg_tta_amd.tta.nifti_io import write_nifti
    case = synthetic_case(size=size, k=1, seed=seed)
    img = (case[0] * 300.0).numpy().astype(np.float32)
    lab = torch.cat([(case[1:].sum(0, keepdim=True) < 1).float(), case[1:]]).argmax(0).numpy().astype(np.int16)
    write_nifti(folder_img / f"{name}_0000.nii.gz", img, spacing=spacing)
    write_nifti(folder_lab / f"{name}.nii.gz", lab, spacing=spacing)


def test_plan_then_pretrain(tmp_path, monkeypatch):
    from dg_tta_amd.run import DGTTAProgram
    raw, pre, res, root = tmp_path / "raw", tmp_path / "pre", tmp_path / "res", tmp_path / "dgroot"
    src = raw / "Dataset813_Raw"
    (src / "imagesTr").mkdir(parents=True)
    (src / "labelsTr").mkdir()
    for i in range(3):
        _write_case(src / "imagesTr", src / "labelsTr", f"ct{i:02d}", 40, 31 + i, (1.5, 1.5, 1.5))
    dataset_json = {"labels": {"background": 0, "organ": 1}, "file_ending": ".nii.gz", "channel_names": {"0": "CT"}, "numTraining": 3}
    json.dump(dataset_json, open(src / "dataset.json", "w"))
    root.mkdir()
    for k, v in {"nnUNet_raw": str(raw), "nnUNet_results": str(res), "nnUNet_preprocessed": str(pre), "DG_TTA_ROOT": str(root)}.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("DG_TTA_INTERNAL_AUGMENTATION", os.environ.get("DG_TTA_INTERNAL_AUGMENTATION", "false"))
    pretrain = ["dgtta", "pretrain", "813", "3d_fullres", "0", "-tr", "nnUNetTrainer_GIN_MIND", "--num_epochs", "1",
                "--iterations_per_epoch", "2", "--val_iterations", "1", "--device", DEV, "--seed", "7"]
    with pytest.raises(FileNotFoundError, match="no experiment planning"):
        DGTTAProgram(pretrain)

    DGTTAProgram(["dgtta", "plan", "813", "--device", DEV])
    plans = json.load(open(pre / "Dataset813_Raw" / "nnUNetPlans.json"))
    fingerprint = json.load(open(pre / "Dataset813_Raw" / "dataset_fingerprint.json"))
    assert fingerprint["shapes_after_crop"] == [[40, 40, 40]] * 3 and fingerprint["spacings"] == [[1.5, 1.5, 1.5]] * 3
    conf = plans["configurations"]["3d_fullres"]
    assert sorted(plans["configurations"]) == ["3d_fullres"] and conf["patch_size"] == [40, 40, 40] and conf["spacing"] == [1.5, 1.5, 1.5]
    assert conf["normalization_schemes"] == ["CTNormalization"] and conf["batch_size"] == 2
    assert plans["foreground_intensity_properties_per_channel"] == fingerprint["foreground_intensity_properties_per_channel"]

    DGTTAProgram(pretrain)
    folder = res / "Dataset813_Raw" / "nnUNetTrainer_GIN_MIND__nnUNetPlans__3d_fullres"
    assert (folder / "fold_0" / "checkpoint_final.pth").is_file()
    assert json.load(open(folder / "plans.json")) == plans
    ck = torch.load(folder / "fold_0" / "checkpoint_final.pth", map_location="cpu", weights_only=False)
    assert ck["current_epoch"] == 1 and np.isfinite(ck["logging"]["train_losses"]).all()
