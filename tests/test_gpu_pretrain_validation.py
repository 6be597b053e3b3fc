"""GPU: the end of a pre-trained fold - `--dice plans` (the plans' batch_dice in the loss), checkpoint_best.pth and the final
validation (`--validate` / `--val`) - on a tiny synthetic source dataset built the way tests/test_gpu_pretrain.py builds its own:
three 48^3 cases and one of 24^3 (smaller than the 32^3 patch), a four-stage network, batch 2, 2 epochs x 2 iterations, seeded.
The trainer is nnUNetTrainer_GIN: with the internal augmentation off its prediction draws no device noise and is repeatable."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]
TRAINER = "nnUNetTrainer_GIN"
VAL = ["ct02", "small"]
RUN = dict(num_epochs=2, iterations_per_epoch=2, val_iterations=1, device=DEV, seed=7)


def _write_case(folder_img, folder_lab, name, size, seed, spacing=(1.5, 1.5, 1.5)):
    from dg_tta_amd.synthetic import synthetic_case
    from dg_tta_amd.tta.nifti_io import write_nifti
    case = synthetic_case(size=size, k=3, seed=seed)
    img = (case[0] * 300.0).numpy().astype(np.float32)                # CT-like range for the plans' CTNormalization
    lab = torch.cat([(case[1:].sum(0, keepdim=True) < 1).float(), case[1:]]).argmax(0).numpy().astype(np.int16)
    write_nifti(folder_img / f"{name}_0000.nii.gz", img, spacing=spacing)
    write_nifti(folder_lab / f"{name}.nii.gz", lab, spacing=spacing)


def _plans(batch_dice=True):
    """The skeleton's plans (which say batch_dice: true) with a 32^3 patch and four stages; batch_dice None drops the key."""
    plans = json.load(open(ROOT / "dg_tta_amd" / "__resources__" / "model_skeleton" / "plans.json"))
    conf = plans["configurations"]["3d_fullres"]
    assert conf["batch_dice"] is True
    conf.update(patch_size=[32, 32, 32], batch_size=2, n_conv_per_stage_encoder=[2, 2, 2, 2], n_conv_per_stage_decoder=[2, 2, 2],
                pool_op_kernel_sizes=[[1, 1, 1], [2, 2, 2], [2, 2, 2], [2, 2, 2]], conv_kernel_sizes=[[3, 3, 3]] * 4,
                num_pool_per_axis=[3, 3, 3])
    if batch_dice is None:
        del conf["batch_dice"]
    return plans


class _Env:
    """The nnU-Net folders of one run: the dataset is shared, every run has its own results folder."""

    def __init__(self, root):
        self.root = root
        self.plans_file = root / "pre" / "Dataset802_Source" / "nnUNetPlans.json"

    def use(self, mp, tag):
        for k, v in {"nnUNet_raw": self.root / "raw", "nnUNet_results": self.root / f"res_{tag}", "nnUNet_preprocessed": self.root / "pre"}.items():
            mp.setenv(k, str(v))
        mp.setenv("DG_TTA_INTERNAL_AUGMENTATION", "false")
        return self.root / f"res_{tag}" / "Dataset802_Source" / f"{TRAINER}__nnUNetPlans__3d_fullres" / "fold_0"


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    root = tmp_path_factory.mktemp("pretrain_validation")
    src = root / "raw" / "Dataset802_Source"
    (src / "imagesTr").mkdir(parents=True)
    (src / "labelsTr").mkdir()
    for i in range(3):
        _write_case(src / "imagesTr", src / "labelsTr", f"ct{i:02d}", 48, 11 + i)
    _write_case(src / "imagesTr", src / "labelsTr", "small", 24, 21)
    json.dump({"labels": {"background": 0, "liver": 1, "spleen": 2, "kidney": 3}, "file_ending": ".nii.gz",
               "channel_names": {"0": "CT"}, "numTraining": 4}, open(src / "dataset.json", "w"))
    pre = root / "pre" / "Dataset802_Source"
    pre.mkdir(parents=True)
    json.dump(_plans(), open(pre / "nnUNetPlans.json", "w"))
    json.dump([{"train": ["ct00", "ct01"], "val": VAL}], open(pre / "splits_final.json", "w"))
    return _Env(root)


@pytest.fixture(scope="module")
def plans_run(env):
    """train_fold(dice="plans", final_validation=True) once for the tests below -> (fold folder, what it printed)."""
    import contextlib
    import io
    from dg_tta_amd.pretraining import trainer
    out = io.StringIO()
    with pytest.MonkeyPatch.context() as mp:
        fold_dir = env.use(mp, "plans")
        with contextlib.redirect_stdout(out):
            final = trainer.train_fold("802", "3d_fullres", 0, TRAINER, dice="plans", final_validation=True, **RUN)
    assert final == fold_dir / "checkpoint_final.pth"
    return fold_dir, out.getvalue()


def _log(fold_dir, name="checkpoint_final.pth"):
    return torch.load(fold_dir / name, map_location="cpu", weights_only=False)


def test_validation_writes_label_maps_and_a_summary_that_numpy_reproduces(env, plans_run):
    fold_dir, printed = plans_run
    from dg_tta_amd.pretraining.trainer import BATCH_DICE_NOTE
    assert BATCH_DICE_NOTE not in printed                                        # the plans are obeyed: nothing to warn about
    val = fold_dir / "validation"
    assert sorted(p.name for p in val.iterdir()) == ["ct02.npy", "small.npy", "summary.json"]
    assert (fold_dir / "checkpoint_best.pth").is_file() and (fold_dir / "checkpoint_latest.pth").is_file()
    summary = json.load(open(val / "summary.json"))
    assert set(summary) == {"metric_per_case", "mean", "foreground_mean"} and len(summary["metric_per_case"]) == 2
    data_dir = env.root / "pre" / "Dataset802_Source" / "nnUNetPlans_3d_fullres"
    dice = {lab: [] for lab in range(4)}
    for name, entry in zip(VAL, summary["metric_per_case"]):
        pred = np.load(val / f"{name}.npy")
        with np.load(data_dir / f"{name}.npz") as z:
            seg = z["seg"][0]
        ref = np.where(seg < 0, 0, seg)
        assert pred.dtype == np.uint8 and pred.shape == ref.shape == ((24,) * 3 if name == "small" else (48,) * 3)
        assert pred.max() <= 3 and Path(entry["prediction_file"]).name == f"{name}.npy" and Path(entry["reference_file"]).name == f"{name}.npz"
        assert set(entry["metrics"]) == {"0", "1", "2", "3"}
        for lab in range(4):
            m = entry["metrics"][str(lab)]
            p, r = pred == lab, ref == lab
            tp, fp, fn = int((p & r).sum()), int((p & ~r).sum()), int((~p & r).sum())
            assert (m["TP"], m["FP"], m["FN"], m["TN"], m["n_pred"], m["n_ref"]) == (tp, fp, fn, pred.size - tp - fp - fn, int(p.sum()), int(r.sum()))
            if tp + fp + fn == 0:
                assert m["Dice"] != m["Dice"]                                    # NaN: absent from both
            else:
                assert m["Dice"] == pytest.approx(2 * tp / (2 * tp + fp + fn), rel=1e-15, abs=0)
                dice[lab].append(2 * tp / (2 * tp + fp + fn))
    for lab in range(4):
        if dice[lab]:
            assert summary["mean"][str(lab)]["Dice"] == pytest.approx(np.mean(dice[lab]), rel=1e-14, abs=0)
    if all(dice[lab] for lab in (1, 2, 3)):
        assert summary["foreground_mean"]["Dice"] == pytest.approx(np.mean([np.mean(dice[lab]) for lab in (1, 2, 3)]), rel=1e-14, abs=0)
    assert "pretrain: validated small" in printed


def test_val_alone_reproduces_every_label_map_byte_for_byte(env, plans_run, monkeypatch):
    from dg_tta_amd.run import DGTTAProgram
    fold_dir, _ = plans_run
    val = fold_dir / "validation"
    before = {n: (val / n).read_bytes() for n in ("ct02.npy", "small.npy")}
    summary = (val / "summary.json").read_text()
    weights = (fold_dir / "checkpoint_final.pth").read_bytes()
    for n in before:
        (val / n).unlink()
    env.use(monkeypatch, "plans")
    DGTTAProgram(["dgtta", "pretrain", "802", "3d_fullres", "0", "-tr", TRAINER, "--device", DEV, "--val"])
    assert {n: (val / n).read_bytes() for n in before} == before
    assert (val / "summary.json").read_text() == summary
    assert (fold_dir / "checkpoint_final.pth").read_bytes() == weights            # nothing was trained
    assert len((fold_dir / "training_log.txt").read_text().splitlines()) == 2


def test_val_without_a_trained_fold_says_so(env, monkeypatch):
    from dg_tta_amd.pretraining import trainer
    env.use(monkeypatch, "nothing_here")
    with pytest.raises(FileNotFoundError, match="checkpoint_final.pth not found"):
        trainer.validate_fold("802", "3d_fullres", 0, TRAINER, device=DEV)


def test_best_checkpoint_is_the_epoch_the_logged_average_names(plans_run):
    from dg_tta_amd.pretraining.trainer import rebuild_ema
    fold_dir, _ = plans_run
    final, best = _log(fold_dir), _log(fold_dir, "checkpoint_best.pth")
    log = final["logging"]
    assert set(log) == {"train_losses", "val_losses", "mean_fg_dice", "lrs", "ema_fg_dice"} and len(log["ema_fg_dice"]) == 2
    series, top = rebuild_ema(log["mean_fg_dice"])
    assert np.array_equal(np.array(series), np.array(log["ema_fg_dice"]), equal_nan=True) and top is not None
    epoch = next(i for i, v in enumerate(log["ema_fg_dice"]) if v == top)      # the first epoch that reached the best average
    assert best["current_epoch"] == epoch + 1 and len(best["logging"]["ema_fg_dice"]) == epoch + 1
    assert best["logging"]["ema_fg_dice"][-1] == top and set(best) == set(final)
    same = all(torch.equal(v, final["network_weights"][k]) for k, v in best["network_weights"].items())
    assert same == (epoch == 1)                   # the last epoch's weights are the final ones, an earlier epoch's are not


def test_defaults_train_per_sample_say_so_and_write_no_validation(env, plans_run, monkeypatch, capsys):
    """dice="sample" under plans that say batch_dice: true: the note, no validation/, and losses that are those of
    ops.deep_supervision_loss without the keyword - the same seeded run under `dice="plans"` with plans WITHOUT the key logs the
    same losses bit for bit, the run that obeyed batch_dice: true does not; one fixed batch on the final weights, both ways."""
    from dg_tta_amd import ops
    from dg_tta_amd.pretraining import trainer
    fold_b = env.use(monkeypatch, "defaults")
    trainer.train_fold("802", "3d_fullres", 0, TRAINER, **RUN)
    assert trainer.BATCH_DICE_NOTE in capsys.readouterr().out
    assert not (fold_b / "validation").exists() and (fold_b / "checkpoint_best.pth").is_file()
    log_b = _log(fold_b)["logging"]

    original = env.plans_file.read_text()
    try:                                          # `--dice plans` with plans that have no batch_dice key trains per sample
        json.dump(_plans(batch_dice=None), open(env.plans_file, "w"))
        fold_c = env.use(monkeypatch, "no_key")
        trainer.train_fold("802", "3d_fullres", 0, TRAINER, dice="plans", **RUN)
        assert trainer.BATCH_DICE_NOTE not in capsys.readouterr().out
    finally:
        env.plans_file.write_text(original)
    log_c = _log(fold_c)["logging"]
    for key in ("train_losses", "val_losses", "mean_fg_dice", "ema_fg_dice", "lrs"):
        assert np.array_equal(np.array(log_b[key]), np.array(log_c[key]), equal_nan=True), key
    log_a = _log(plans_run[0])["logging"]
    assert log_a["train_losses"] != log_b["train_losses"] and log_a["val_losses"] != log_b["val_losses"]
    assert log_a["train_losses"][0] != log_b["train_losses"][0]                  # from the first epoch on: same draws, another loss

    ck = _log(fold_b)
    net, patch = trainer.build_network(ck["init_args"]["plans"], ck["init_args"]["dataset_json"], "3d_fullres", TRAINER, seed=7)
    net.load_state_dict(ck["network_weights"])
    net = net.to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    imgs = torch.randn((2, 1, *patch), generator=g).to(DEV)
    target = torch.randint(0, 3, (2, *patch), generator=g).to(DEV)
    target[0, :4] = 3                                                            # class 3 in sample 0 only
    with torch.no_grad():
        outs = net(imgs)
        plain, _ = ops.deep_supervision_loss(outs, target)
        off, _ = ops.deep_supervision_loss(outs, target, batch_dice=False)          # what the loop calls under dice="sample"
        pooled, _ = ops.deep_supervision_loss(outs, target, batch_dice=True)
    assert torch.equal(off, plain) and not torch.equal(plain, pooled)


def test_continue_from_a_checkpoint_written_before_the_best_rule(env, monkeypatch):
    """--c on checkpoints whose log has no `ema_fg_dice` and a fold without checkpoint_best.pth: the series is rebuilt from
    mean_fg_dice, one more epoch runs, and the best file appears only if that epoch's average exceeds the rebuilt best."""
    from dg_tta_amd.pretraining import trainer
    fold_dir = env.use(monkeypatch, "old")
    trainer.train_fold("802", "3d_fullres", 0, TRAINER, **RUN)
    for name in ("checkpoint_latest.pth", "checkpoint_final.pth"):
        ck = _log(fold_dir, name)
        del ck["logging"]["ema_fg_dice"]
        torch.save(ck, fold_dir / name)
    (fold_dir / "checkpoint_best.pth").unlink()
    old = _log(fold_dir)["logging"]
    _, best = trainer.rebuild_ema(old["mean_fg_dice"])
    trainer.train_fold("802", "3d_fullres", 0, TRAINER, continue_training=True, **dict(RUN, num_epochs=3))
    ck = _log(fold_dir)
    log = ck["logging"]
    assert ck["current_epoch"] == 3 and log["mean_fg_dice"][:2] == old["mean_fg_dice"] and len(log["mean_fg_dice"]) == 3
    series, _ = trainer.rebuild_ema(log["mean_fg_dice"])
    assert np.array_equal(np.array(series), np.array(log["ema_fg_dice"]), equal_nan=True)
    assert (fold_dir / "checkpoint_best.pth").is_file() == trainer.is_new_best(series[2], best)
