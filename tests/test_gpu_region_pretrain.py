"""GPU, end to end: a REGION-based dataset through `dgtta plan` and `dgtta pretrain ... --validate`, for the stock nnUNetTrainer
and for nnUNetTrainer_GIN_MIND.  The dataset is synthetic and single-channel: nested ellipsoids, labels 1 > 2 > 3 painted in
order, read as the regions whole = [1, 2, 3], core = [2, 3], centre = 3 with regions_class_order [1, 2, 3]; three 40^3 cases and
the 32^3 four-stage plans of tests/test_gpu_pretrain.py (which say batch_dice: true), batch 2, 2 epochs x 3 iterations, seeded.
No threshold on how well two epochs learn: whether the loss learns is what tests/test_gpu_region_loss.py establishes."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]
STOCK, DG = "nnUNetTrainer", "nnUNetTrainer_GIN_MIND"
DATASET = {"labels": {"background": 0, "whole": [1, 2, 3], "core": [2, 3], "centre": 3}, "regions_class_order": [1, 2, 3],
           "file_ending": ".nii.gz", "channel_names": {"0": "CT"}, "numTraining": 3}
KEYS = {"(1, 2, 3)", "(2, 3)", "3"}
NAME = "Dataset820_Regions"


def _write_case(folder_img, folder_lab, name, size, seed):
    from dg_tta_amd.tta.nifti_io import write_nifti
    rng = np.random.RandomState(seed)
    c = size / 2 + rng.uniform(-3, 3, size=3)
    g = np.stack(np.meshgrid(*(np.arange(size),) * 3, indexing="ij"), axis=-1)
    lab = np.zeros((size,) * 3, dtype=np.int16)
    for value, radii in ((1, rng.uniform(13, 16, 3)), (2, rng.uniform(8, 10, 3)), (3, rng.uniform(3.5, 5, 3))):
        lab[(((g - c) / radii) ** 2).sum(-1) < 1] = value
    img = (lab * 80.0 + rng.standard_normal(lab.shape) * 25.0 - 100.0).astype(np.float32)
    write_nifti(folder_img / f"{name}_0000.nii.gz", img, spacing=(1.5, 1.5, 1.5))
    write_nifti(folder_lab / f"{name}.nii.gz", lab, spacing=(1.5, 1.5, 1.5))


def _small_plans():
    plans = json.load(open(ROOT / "dg_tta_amd" / "__resources__" / "model_skeleton" / "plans.json"))
    conf = plans["configurations"]["3d_fullres"]
    assert conf["batch_dice"] is True
    conf.update(patch_size=[32, 32, 32], batch_size=2, n_conv_per_stage_encoder=[2, 2, 2, 2], n_conv_per_stage_decoder=[2, 2, 2],
                pool_op_kernel_sizes=[[1, 1, 1], [2, 2, 2], [2, 2, 2], [2, 2, 2]], conv_kernel_sizes=[[3, 3, 3]] * 4,
                num_pool_per_axis=[3, 3, 3])
    return plans


class _Env:
    def __init__(self, root):
        self.root = root

    def use(self, mp, tag, trainer=STOCK):
        for k, v in {"nnUNet_raw": self.root / "raw", "nnUNet_results": self.root / f"res_{tag}", "nnUNet_preprocessed": self.root / "pre",
                     "DG_TTA_ROOT": self.root / "dgroot"}.items():
            mp.setenv(k, str(v))
        mp.setenv("DG_TTA_INTERNAL_AUGMENTATION", "false")
        return self.root / f"res_{tag}" / NAME / f"{trainer}__nnUNetPlans__3d_fullres" / "fold_0"


def _pretrain(trainer, *extra, epochs=2):
    from dg_tta_amd.run import DGTTAProgram
    DGTTAProgram(["dgtta", "pretrain", "820", "3d_fullres", "0", "-tr", trainer, "--num_epochs", str(epochs), "--iterations_per_epoch", "3",
                  "--val_iterations", "1", "--device", DEV, "--seed", "7", *extra])


def _ck(fold_dir, name="checkpoint_final.pth"):
    return torch.load(fold_dir / name, map_location="cpu", weights_only=False)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    """The raw dataset, `dgtta plan` on it (a region dataset must plan), then the small plans in the planner's place."""
    from dg_tta_amd.run import DGTTAProgram
    root = tmp_path_factory.mktemp("region_pretrain")
    src = root / "raw" / NAME
    (src / "imagesTr").mkdir(parents=True)
    (src / "labelsTr").mkdir()
    (root / "dgroot").mkdir()
    for i in range(3):
        _write_case(src / "imagesTr", src / "labelsTr", f"ct{i:02d}", 40, 41 + i)
    json.dump(DATASET, open(src / "dataset.json", "w"))
    e = _Env(root)
    with pytest.MonkeyPatch.context() as mp:
        e.use(mp, "plan")
        DGTTAProgram(["dgtta", "plan", "820", "--device", DEV])
    pre = root / "pre" / NAME
    planned = json.load(open(pre / "nnUNetPlans.json"))
    assert planned["configurations"]["3d_fullres"]["patch_size"] == [40, 40, 40]
    assert json.load(open(pre / "dataset.json")) == DATASET
    json.dump(_small_plans(), open(pre / "nnUNetPlans.json", "w"))
    json.dump([{"train": ["ct00", "ct01"], "val": ["ct02"]}], open(pre / "splits_final.json", "w"))
    return e


@pytest.fixture(scope="module")
def stock_run(env):
    """`dgtta pretrain -tr nnUNetTrainer --dice plans --validate` once; the validation batches that reached ops.region_counts and
    the losses that reached the log are kept -> (fold folder, [(logits, target, counts)] per epoch)."""
    from dg_tta_amd import ops
    seen = []
    real = ops.region_counts

    def spy(logits, labels, table):
        counts = real(logits, labels, table)
        seen.append((logits.detach().clone(), labels.detach().clone(), table.clone(), counts.clone()))
        return counts
    with pytest.MonkeyPatch.context() as mp:
        fold_dir = env.use(mp, "plans")
        mp.setattr(ops, "region_counts", spy)
        _pretrain(STOCK, "--dice", "plans", "--validate")
    return fold_dir, seen


def test_head_has_one_output_per_region_at_every_scale(env, stock_run):
    from dg_tta_amd.pretraining.trainer import build_network
    net, patch = build_network(_small_plans(), DATASET, "3d_fullres", STOCK)
    assert patch == [32, 32, 32] and len(net.decoder.seg_layers) == 3 and all(s.out_channels == 3 for s in net.decoder.seg_layers)
    ck = _ck(stock_run[0])
    heads = [k for k in ck["network_weights"] if "seg_layers" in k and k.endswith("weight")]
    assert len(heads) == 3 and all(ck["network_weights"][k].shape[0] == 3 for k in heads)
    assert ck["regions_class_order"] == [1, 2, 3] and ck["inference_allowed_mirroring_axes"] == [0, 1, 2]
    assert ck["current_epoch"] == 2


def test_losses_are_finite_and_the_logged_pseudo_dice_is_the_region_counts_one(stock_run):
    import region_ref
    from dg_tta_amd import ops
    fold_dir, seen = stock_run
    log = _ck(fold_dir)["logging"]
    assert len(log["train_losses"]) == len(log["val_losses"]) == len(log["mean_fg_dice"]) == 2 and len(seen) == 2
    assert np.isfinite(log["train_losses"]).all() and np.isfinite(log["val_losses"]).all()
    for epoch, (logits, target, table, counts) in enumerate(seen):
        assert tuple(logits.shape) == (2, 3, 32, 32, 32) and tuple(counts.shape) == (3, 3)
        again = ops.region_counts(logits, target, table)
        assert torch.equal(again, counts)
        lg = logits.float().permute(0, 2, 3, 4, 1).reshape(2, -1, 3).permute(0, 2, 1).cpu().numpy()
        tab = table.cpu().numpy().view(np.uint32)
        assert tab.tolist() == [0, 1, 3, 7]
        assert np.array_equal(counts.cpu().numpy(), region_ref.region_counts(lg, target.reshape(2, -1).cpu().numpy(), tab))
        tp, fp, fn = counts.cpu().numpy().astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            dice = 2 * tp / (2 * tp + fp + fn)
        want = float(np.mean(dice[~np.isnan(dice)])) if (~np.isnan(dice)).any() else float("nan")
        got = log["mean_fg_dice"][epoch]
        assert (np.isnan(want) and np.isnan(got)) or got == pytest.approx(want, rel=1e-12, abs=0)


def test_validation_writes_region_maps_and_a_summary_keyed_by_region(env, stock_run):
    fold_dir, _ = stock_run
    val = fold_dir / "validation"
    assert sorted(p.name for p in val.iterdir()) == ["ct02.npy", "summary.json"]
    pred = np.load(val / "ct02.npy")
    assert pred.dtype == np.uint8 and pred.shape == (40, 40, 40) and set(np.unique(pred).tolist()) <= {0, 1, 2, 3}
    summary = json.load(open(val / "summary.json"))
    assert set(summary["mean"]) == KEYS and set(summary["metric_per_case"][0]["metrics"]) == KEYS
    with np.load(env.root / "pre" / NAME / "nnUNetPlans_3d_fullres" / "ct02.npz") as z:
        ref = np.where(z["seg"][0] < 0, 0, z["seg"][0])
    for key, region in (("(1, 2, 3)", (1, 2, 3)), ("(2, 3)", (2, 3)), ("3", (3,))):
        m = summary["metric_per_case"][0]["metrics"][key]
        p, r = np.isin(pred, region), np.isin(ref, region)
        tp, fp, fn = int((p & r).sum()), int((p & ~r).sum()), int((~p & r).sum())
        assert (m["TP"], m["FP"], m["FN"], m["TN"], m["n_pred"], m["n_ref"]) == (tp, fp, fn, pred.size - tp - fp - fn, int(p.sum()), int(r.sum()))
        assert r.sum() > 0 and m["Dice"] == pytest.approx(2 * tp / (2 * tp + fp + fn), rel=1e-15, abs=0)


def test_same_seed_same_checkpoint_and_batch_dice_takes_the_pooled_path(env, stock_run, monkeypatch):
    fold_dir, _ = stock_run
    a = _ck(fold_dir)
    again = env.use(monkeypatch, "again")
    _pretrain(STOCK, "--dice", "plans")
    b = _ck(again)
    assert list(a["network_weights"]) == list(b["network_weights"])
    assert all(torch.equal(a["network_weights"][k], b["network_weights"][k]) for k in a["network_weights"])
    assert a["logging"]["train_losses"] == b["logging"]["train_losses"] and a["logging"]["val_losses"] == b["logging"]["val_losses"]
    assert not (again / "validation").exists()
    # per sample (the default): the same draws, another Dice term - the loss differs from the first epoch on (B = 2)
    sample = env.use(monkeypatch, "sample")
    _pretrain(STOCK)
    c = _ck(sample)
    assert np.isfinite(c["logging"]["train_losses"]).all() and c["logging"]["train_losses"][0] != a["logging"]["train_losses"][0]
    assert c["logging"]["val_losses"][0] != a["logging"]["val_losses"][0]


def test_continue_training_resumes(env, monkeypatch):
    fold_dir = env.use(monkeypatch, "resume")
    _pretrain(STOCK, epochs=1)
    assert _ck(fold_dir)["current_epoch"] == 1
    _pretrain(STOCK, "--c", epochs=2)
    ck = _ck(fold_dir)
    assert ck["current_epoch"] == 2 and len(ck["logging"]["train_losses"]) == 2 and np.isfinite(ck["logging"]["train_losses"]).all()
    assert ck["regions_class_order"] == [1, 2, 3]


def test_dg_trainer_trains_validates_and_tta_refuses(env, monkeypatch):
    from dg_tta_amd.run import DGTTAProgram
    fold_dir = env.use(monkeypatch, "dg", DG)
    _pretrain(DG, "--validate")
    ck = _ck(fold_dir)
    assert np.isfinite(ck["logging"]["train_losses"]).all() and np.isfinite(ck["logging"]["val_losses"]).all()
    assert ck["regions_class_order"] == [1, 2, 3] and ck["inference_allowed_mirroring_axes"] is None
    heads = [k for k in ck["network_weights"] if "seg_layers" in k and k.endswith("weight")]
    assert len(heads) == 3 and all(ck["network_weights"][k].shape[0] == 3 for k in heads)
    summary = json.load(open(fold_dir / "validation" / "summary.json"))
    assert set(summary["mean"]) == KEYS
    assert set(np.unique(np.load(fold_dir / "validation" / "ct02.npy")).tolist()) <= {0, 1, 2, 3}
    # a region model is not adapted: prepare_tta says why, before it writes anything
    tgt = env.root / "raw" / "Dataset821_Target"
    (tgt / "imagesTs").mkdir(parents=True, exist_ok=True)
    json.dump({"labels": {"background": 0, "centre": 1}}, open(tgt / "dataset.json", "w"))
    with pytest.raises(NotImplementedError, match="region-based model.*masked softmax"):
        DGTTAProgram(["dgtta", "prepare_tta", "820", "821", "--pretrainer", DG])
    assert not (env.root / "dgroot" / "plans").exists()
