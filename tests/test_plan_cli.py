"""`dgtta plan --device cpu` on three tiny synthetic NIfTI cases: the three files appear where `dgtta pretrain` looks for them,
load_dataset_files and the configuration resolver read them, the fingerprint's shapes and spacings are the cases', its
intensity block is numpy's on the pooled foreground, and a second run without --overwrite refuses."""
import json

import numpy as np
import pytest

SHAPE = (24, 20, 28)
SPACINGS = [(1.5, 1.25, 1.0), (2.0, 1.0, 1.0), (1.5, 1.5, 1.5)]          # (x, y, z) as the writer takes them
BORDER = ((3, 2), (0, 4), (5, 0))                                         # zero border of case 1 along (z, y, x): low, high


def _case(seed, border=None):
    rng = np.random.default_rng(seed)
    img = (rng.standard_normal(SHAPE) * 200 + 40).astype(np.float32)
    img[img == 0] = 1.0
    lab = np.zeros(SHAPE, dtype=np.uint8)
    lab[6:16, 5:14, 8:20] = 1
    lab[10:14, 8:12, 12:16] = 2
    if border is not None:
        keep = tuple(slice(lo, s - hi) for (lo, hi), s in zip(border, SHAPE))
        inner = np.zeros_like(img)
        inner[keep] = img[keep]
        img = inner
    return img, lab


@pytest.fixture()
def dataset(tmp_path, monkeypatch):
    from dg_tta_amd.tta.nifti_io import write_nifti
    raw, pre = tmp_path / "raw", tmp_path / "pre"
    src = raw / "Dataset811_Plan"
    (src / "imagesTr").mkdir(parents=True)
    (src / "labelsTr").mkdir()
    cases = []
    for i, spacing in enumerate(SPACINGS):
        img, lab = _case(20 + i, BORDER if i == 1 else None)
        write_nifti(src / "imagesTr" / f"case{i}_0000.nii.gz", img, spacing=spacing)
        write_nifti(src / "labelsTr" / f"case{i}.nii.gz", lab, spacing=spacing)
        cases.append((img, lab))
    dataset_json = {"labels": {"background": 0, "liver": 1, "lesion": 2}, "file_ending": ".nii.gz", "channel_names": {"0": "CT"},
                    "numTraining": 3}
    json.dump(dataset_json, open(src / "dataset.json", "w"))
    for k, v in {"nnUNet_raw": str(raw), "nnUNet_preprocessed": str(pre), "nnUNet_results": str(tmp_path / "res"),
                 "DG_TTA_ROOT": str(tmp_path / "root")}.items():
        monkeypatch.setenv(k, v)
    return pre / "Dataset811_Plan", dataset_json, cases


def test_plan_cli_on_the_host(dataset, capsys):
    from dg_tta_amd.pretraining.trainer import _configuration, load_dataset_files
    from dg_tta_amd.run import DGTTAProgram
    from dg_tta_amd.tta.nnunet_utils import unet_cfg_from_plans
    pre, dataset_json, cases = dataset
    with pytest.raises(FileNotFoundError, match="no experiment planning.*dgtta plan"):
        load_dataset_files("Dataset811_Plan")
    DGTTAProgram(["dgtta", "plan", "811", "--device", "cpu"])
    out = capsys.readouterr().out
    assert "plan: 3d_fullres:" in out and "`2d`" in out
    for name in ("dataset_fingerprint.json", "nnUNetPlans.json", "dataset.json"):
        assert (pre / name).is_file(), name
    assert json.load(open(pre / "dataset.json")) == dataset_json

    fingerprint = json.load(open(pre / "dataset_fingerprint.json"))
    assert sorted(fingerprint) == ["foreground_intensity_properties_per_channel", "median_relative_size_after_cropping",
                                   "shapes_after_crop", "spacings"]
    cropped = tuple(s - lo - hi for (lo, hi), s in zip(BORDER, SHAPE))
    assert fingerprint["shapes_after_crop"] == [list(SHAPE), list(cropped), list(SHAPE)]
    assert fingerprint["spacings"] == [[float(np.float32(s)) for s in sp[::-1]] for sp in SPACINGS]
    assert fingerprint["median_relative_size_after_cropping"] == 1.0
    pooled = np.concatenate([img[lab > 0] for img, lab in cases]).astype(np.float64)
    block = fingerprint["foreground_intensity_properties_per_channel"]["0"]
    assert block["min"] == pooled.min() and block["max"] == pooled.max()
    assert block["mean"] == pytest.approx(pooled.mean(), rel=1e-13) and block["std"] == pytest.approx(pooled.std(), rel=1e-12)
    for key, q in (("percentile_00_5", 0.5), ("median", 50), ("percentile_99_5", 99.5)):
        assert block[key] == pytest.approx(np.percentile(pooled, q), rel=1e-12)

    plans, dj, pre_dir, _ = load_dataset_files("Dataset811_Plan")
    assert dj == dataset_json and pre_dir == pre and plans["dataset_name"] == "Dataset811_Plan"
    assert plans["foreground_intensity_properties_per_channel"] == fingerprint["foreground_intensity_properties_per_channel"]
    conf = _configuration(plans, "3d_fullres")
    assert conf["normalization_schemes"] == ["CTNormalization"] and conf["batch_size"] >= 2
    assert all(p % 2 ** n == 0 for p, n in zip(conf["patch_size"], conf["num_pool_per_axis"]))
    cfg, patch = unet_cfg_from_plans(plans, dj, "3d_fullres", in_channels=1)
    assert patch == conf["patch_size"] and cfg["num_classes"] == 3

    before = (pre / "nnUNetPlans.json").read_bytes()
    with pytest.raises(SystemExit, match="--overwrite"):
        DGTTAProgram(["dgtta", "plan", "811", "--device", "cpu"])
    assert (pre / "nnUNetPlans.json").read_bytes() == before
    DGTTAProgram(["dgtta", "plan", "811", "--device", "cpu", "--overwrite", "--cache_gib", "0"])
    assert (pre / "nnUNetPlans.json").read_bytes() == before


def test_an_unrunnable_channel_is_refused_before_a_voxel_is_read(dataset):
    from dg_tta_amd.run import DGTTAProgram
    pre, dataset_json, _ = dataset
    raw = pre.parents[1] / "raw" / "Dataset811_Plan"
    json.dump(dict(dataset_json, channel_names={"0": "rescale_to_0_1"}), open(raw / "dataset.json", "w"))
    (raw / "labelsTr" / "case0.nii.gz").write_bytes(b"not an image")       # reading a case would fail with another error
    with pytest.raises(SystemExit, match="rescale_to_0_1"):
        DGTTAProgram(["dgtta", "plan", "811", "--device", "cpu"])
    assert not pre.exists() or not any(pre.iterdir())


def test_a_nan_in_the_foreground_names_the_case(dataset):
    from dg_tta_amd.planning.fingerprint import extract_fingerprint
    from dg_tta_amd.tta.nifti_io import write_nifti
    pre, dataset_json, cases = dataset
    raw = pre.parents[1] / "raw" / "Dataset811_Plan"
    img, lab = cases[2]
    bad = img.copy()
    bad[0, 0, 0] = np.nan                                          # background: no error
    write_nifti(raw / "imagesTr" / "case2_0000.nii.gz", bad, spacing=SPACINGS[2])
    extract_fingerprint(raw, dataset_json, device="cpu")
    bad[8, 8, 10] = np.inf                                         # foreground
    write_nifti(raw / "imagesTr" / "case2_0000.nii.gz", bad, spacing=SPACINGS[2])
    with pytest.raises(ValueError, match="case2"):
        extract_fingerprint(raw, dataset_json, device="cpu")
