"""GPU: the baseline chain on the command line - `dgtta pretrain -tr nnUNetTrainer` (mirrored training batches, a checkpoint
that allows mirroring) -> `dgtta prepare_tta` -> `dgtta run_tta`, whose prediction is the mirrored sliding-window prediction of
the adapted parameters; the plan key "inference_use_mirroring": false switches the mirrored passes off."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from test_gpu_pretrain import _small_plans, _write_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAINER = "nnUNetTrainer"


def test_stock_trainer_pretrain_prepare_run_cli_chain(tmp_path, monkeypatch, capsys):
    from dg_tta_amd.run import DGTTAProgram
    from dg_tta_amd.tta.config_log_utils import load_current_modifier_functions
    from dg_tta_amd.tta.image_io import read_image
    from dg_tta_amd.tta.inference import run_inference
    from dg_tta_amd.tta.model_utils import get_model_from_network
    from dg_tta_amd.tta.nnunet_utils import load_network, preprocess_fromfile
    from dg_tta_amd.tta.torch_utils import generate_label_mapping
    from dg_tta_amd.utils import get_internal_augmentation_enabled
    raw, pre, res, root = tmp_path / "raw", tmp_path / "pre", tmp_path / "res", tmp_path / "dgroot"
    src = raw / "Dataset802_Source"
    (src / "imagesTr").mkdir(parents=True)
    (src / "labelsTr").mkdir()
    for i in range(3):
        _write_case(src / "imagesTr", src / "labelsTr", f"ct{i:02d}", 48, 11 + i)
    dataset_json = {"labels": {"background": 0, "liver": 1, "spleen": 2, "kidney": 3}, "file_ending": ".nii.gz",
                    "channel_names": {"0": "CT"}, "numTraining": 3}
    json.dump(dataset_json, open(src / "dataset.json", "w"))
    (pre / "Dataset802_Source").mkdir(parents=True)
    json.dump(_small_plans(), open(pre / "Dataset802_Source" / "nnUNetPlans.json", "w"))
    root.mkdir()
    for k, v in {"nnUNet_raw": str(raw), "nnUNet_results": str(res), "nnUNet_preprocessed": str(pre), "DG_TTA_ROOT": str(root)}.items():
        monkeypatch.setenv(k, v)
    pretrain = ["dgtta", "pretrain", "802", "3d_fullres", "0", "-tr", TRAINER, "--num_epochs", "1", "--iterations_per_epoch", "2",
                "--val_iterations", "1", "--device", DEV, "--seed", "7"]
    DGTTAProgram(pretrain)
    said = capsys.readouterr().out
    assert "mirroring IS applied" in said and "[0, 1, 2]" in said
    assert not get_internal_augmentation_enabled()              # no hooks: nothing switched the internal augmentation on
    folder = res / "Dataset802_Source" / f"{TRAINER}__nnUNetPlans__3d_fullres"
    final = folder / "fold_0" / "checkpoint_final.pth"
    ck = torch.load(final, map_location="cpu", weights_only=False)
    assert ck["trainer_name"] == TRAINER and ck["inference_allowed_mirroring_axes"] == [0, 1, 2]
    assert ck["network_weights"]["encoder.stages.0.0.convs.0.conv.weight"].shape[1] == 1      # one image channel
    predictor, patch, network, _ = load_network(final, "cpu")
    assert predictor.allowed_mirroring_axes == (0, 1, 2) and patch == [32, 32, 32] and not network._forward_pre_hooks

    # with --seed, a second run gives the same weights (the mirror draws come from the seeded stream)
    monkeypatch.setenv("nnUNet_results", str(tmp_path / "res2"))
    DGTTAProgram(pretrain)
    ck2 = torch.load(tmp_path / "res2" / "Dataset802_Source" / f"{TRAINER}__nnUNetPlans__3d_fullres" / "fold_0" / "checkpoint_final.pth",
                     map_location="cpu", weights_only=False)
    assert all(torch.equal(v, ck2["network_weights"][k]) for k, v in ck["network_weights"].items())
    monkeypatch.setenv("nnUNet_results", str(res))

    # a bare state dict says nothing about mirroring; more than one image channel is refused for the stock trainer
    bare = tmp_path / "bare" / f"{TRAINER}__nnUNetPlans__3d_fullres" / "fold_0"
    bare.mkdir(parents=True)
    for name in ("plans.json", "dataset.json"):
        (bare.parent / name).write_text((folder / name).read_text())
    torch.save(ck["network_weights"], bare / "checkpoint_final.pth")
    assert load_network(bare / "checkpoint_final.pth", "cpu")[0].allowed_mirroring_axes is None
    json.dump(dict(dataset_json, channel_names={"0": "T1", "1": "T2"}), open(bare.parent / "dataset.json", "w"))
    with pytest.raises(NotImplementedError, match="image channels"):
        load_network(bare / "checkpoint_final.pth", "cpu")

    # adapt the baseline model to a target dataset and predict it with mirroring
    tgt = raw / "Dataset803_Target"
    (tgt / "imagesTs").mkdir(parents=True)
    (tgt / "labelsTs").mkdir()
    _write_case(tgt / "imagesTs", tgt / "labelsTs", "mr01", 40, 5)
    json.dump({"labels": {"background": 0, "liver": 1, "spleen": 2, "my_organ": 3}}, open(tgt / "dataset.json", "w"))
    common = ["802", "803", "--pretrainer", TRAINER, "--pretrainer_config", "3d_fullres", "--pretrainer_fold", "0"]
    DGTTAProgram(["dgtta", "prepare_tta"] + common)
    pair = "Pretrained_Dataset802_Source_at_Dataset803_Target"
    plan_dir = root / "plans" / pair / f"{TRAINER}__3d_fullres" / "fold_0"
    plan = json.load(open(plan_dir / "tta_plan.json"))
    assert Path(plan["pretrained_weights_filepath"]) == final and "inference_use_mirroring" not in plan
    plan.update(epochs=2, start_tta_at_epoch=0, patches_to_be_accumulated=2, ensemble_count=1)
    json.dump(plan, open(plan_dir / "tta_plan.json", "w"), indent=4)
    results = root / "results" / pair / f"{TRAINER}__3d_fullres" / "fold_0"

    def run(name):
        DGTTAProgram(["dgtta", "run_tta"] + common + ["--device", DEV, "--dtype", "fp16", "--run_name", name])
        out = results / name / "tta_outputTs"
        seg, _ = read_image(out / "mr01.nii.gz")
        state = torch.load(out / "mr01__ensemble_idx_0_tta_parameters.pt", map_location="cpu")[0]
        return torch.as_tensor(np.asarray(seg).astype(np.int64)), state

    seg_m, state_m = run("mirrored")
    plan["inference_use_mirroring"] = False
    json.dump(plan, open(plan_dir / "tta_plan.json", "w"), indent=4)
    seg_p, state_p = run("plain")
    assert seg_m.shape == (40, 40, 40) and set(seg_m.unique().tolist()) <= {0, 1, 2}

    # the same predictions from the saved parameters, through run_inference
    predictor, patch, network, _ = load_network(final, DEV, act_dtype=torch.float16)
    mapping = generate_label_mapping(json.load(open(plan_dir / "Dataset802_Source_label_mapping.json")),
                                     json.load(open(plan_dir / "Dataset803_Target_label_mapping.json")))
    model = get_model_from_network(network, load_current_modifier_functions(plan_dir)).to(DEV)
    sample = preprocess_fromfile(tgt / "imagesTs" / "mr01_0000.nii.gz", None, "tta_outputTs/mr01", predictor)
    image = sample["data"][:1]
    assert tuple(image.shape[1:]) == tuple(seg_m.shape)          # same spacing, nothing cropped: one geometry
    want_m = run_inference(image, model, [state_m], patch, mapping, plan["optimized_labels"], mirror_axes=predictor.allowed_mirroring_axes)
    want_p = run_inference(image, model, [state_p], patch, mapping, plan["optimized_labels"], mirror_axes=None)
    assert torch.equal(seg_m, want_m) and torch.equal(seg_p, want_p)
    assert not get_internal_augmentation_enabled()              # neither run_tta nor load_network left the global switch on
    # (for the record only - a model of two training steps may well predict one class everywhere)
    other = run_inference(image, model, [state_m], patch, mapping, plan["optimized_labels"], mirror_axes=None)
    print(f"mirrored and unmirrored predictions of the same parameters agree on {float((other == want_m).float().mean()):.4f} of the voxels")
