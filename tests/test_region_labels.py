"""CPU: the label model of dg_tta_amd/labels.py - parsing of region-based dataset.json files, their refusals, the membership
table, unchanged answers for label-based files - and the refusal of prepare_tta / run_tta on a region-based model."""
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from dg_tta_amd import labels as L

ROOT = Path(__file__).resolve().parents[1]
KITS = {"labels": {"background": 0, "kidney_and_masses": [1, 2, 3], "masses": [2, 3], "tumor": 2}, "regions_class_order": [1, 3, 2]}


def test_parsing_file_order_and_ints_as_one_tuples():
    m = L.label_model(KITS)
    assert m.has_regions and m.num_outputs == 3 and L.num_network_outputs(KITS) == 3
    assert m.foreground_regions == ((1, 2, 3), (2, 3), (2,)) and m.region_names == ["kidney_and_masses", "masses", "tumor"]
    assert m.regions_class_order == (1, 3, 2)
    # the file's order decides, not the label values; tuples and one-entry lists are read like lists and ints
    ds = {"labels": {"background": 0, "c": 5, "a": (1, 5), "b": [2]}, "regions_class_order": [5, 1, 2]}
    m = L.label_model(ds)
    assert m.foreground_regions == ((5,), (1, 5), (2,)) and m.names == ["c", "a", "b"]
    assert L.has_regions(ds) and not L.has_regions({"labels": {"background": 0, "a": 1, "b": [2]}})


def test_table_bits():
    m = L.label_model(KITS)
    assert m.table.dtype == np.uint32 and m.table.tolist() == [0b000, 0b001, 0b111, 0b011]
    t = L.membership_table(((5,), (1, 5), (2,)))
    assert t.tolist() == [0, 0b010, 0b100, 0, 0, 0b011]
    # a regions_class_order value above every label value is a value a predicted map can hold: the table covers it
    ds = {"labels": {"background": 0, "a": [1, 2], "b": 2}, "regions_class_order": [1, 7]}
    assert L.label_model(ds).table.tolist() == [0, 1, 3, 0, 0, 0, 0, 0]
    t32 = L.membership_table(tuple((k + 1,) for k in range(32)))
    assert t32[32] == np.uint32(1) << np.uint32(31) and t32.dtype == np.uint32
    with pytest.raises(ValueError, match="1024"):
        L.membership_table(((1, 1024),))
    assert L.membership_table(((1, 1023),)).size == 1024


@pytest.mark.parametrize("change,exc,match", [
    (lambda d: d.pop("regions_class_order"), ValueError, "regions_class_order"),
    (lambda d: d.update(regions_class_order=[1, 2]), ValueError, "regions_class_order"),
    (lambda d: d.update(regions_class_order=[1, 2, 3, 4]), ValueError, "regions_class_order"),
    (lambda d: d.update(regions_class_order=[1, 0, 2]), ValueError, "regions_class_order"),
    (lambda d: d.update(regions_class_order=[1, 2.5, 2]), ValueError, "regions_class_order"),
    (lambda d: d["labels"].update(background=1), ValueError, "background"),
    (lambda d: d["labels"].pop("background"), ValueError, "background"),
    (lambda d: d["labels"].update(ignore=4), NotImplementedError, "ignore"),
    (lambda d: d["labels"].update(tumor=-2), ValueError, "tumor"),
    (lambda d: d["labels"].update(tumor=[2, "x"]), ValueError, "tumor"),
])
def test_refusals(change, exc, match):
    ds = json.loads(json.dumps(KITS))
    change(ds)
    with pytest.raises(exc, match=match):
        L.label_model(ds)


def test_more_than_32_regions_are_refused():
    ds = {"labels": {"background": 0, "all": [1, 2], **{f"r{k}": k for k in range(1, 33)}}, "regions_class_order": list(range(1, 34))}
    with pytest.raises(ValueError, match="32"):
        L.label_model(ds)
    ds["labels"].pop("r32")
    ds["regions_class_order"].pop()
    assert L.label_model(ds).num_outputs == 32


def test_label_based_files_answer_as_before():
    skel = ROOT / "dg_tta_amd" / "__resources__" / "model_skeleton"
    plans, ds = json.load(open(skel / "plans.json")), json.load(open(skel / "dataset.json"))
    m = L.label_model(ds)
    assert not m.has_regions and m.num_outputs == len(ds["labels"]) == 105 and m.regions_class_order is None and m.table is None
    assert m.names == list(ds["labels"])
    from dg_tta_amd.tta import nnunet_utils as nu
    assert nu.unet_cfg_from_plans(plans, ds, "3d_fullres", 12)[0]["num_classes"] == 105
    # an ignore label or a missing regions_class_order troubles nobody without regions: len(labels), as before
    assert L.num_network_outputs({"labels": {"background": 0, "a": 1, "ignore": 2}}) == 3
    assert L.num_network_outputs({"labels": {"background": 0, "a": [1], "b": 2}}) == 3
    L.refuse_region_tta(ds, "x")
    # and a region file sizes the head by its regions
    small = json.loads(json.dumps(plans))
    assert nu.unet_cfg_from_plans(small, KITS, "3d_fullres", 1)[0]["num_classes"] == 3


def _nnunet_tree(tmp_path, monkeypatch):
    raw = tmp_path / "raw"
    for name, ds in (("Dataset900_Regions", KITS), ("Dataset803_Target", {"labels": {"background": 0, "tumor": 1}})):
        (raw / name / "imagesTs").mkdir(parents=True)
        json.dump(ds, open(raw / name / "dataset.json", "w"))
    np.save(raw / "Dataset803_Target" / "imagesTs" / "caseA_0000.npy", np.zeros((1, 8, 8, 8), np.float32))
    root = tmp_path / "dgroot"
    root.mkdir()
    for k, v in {"nnUNet_raw": str(raw), "nnUNet_results": str(tmp_path / "res"), "nnUNet_preprocessed": str(tmp_path / "pre"),
                 "DG_TTA_ROOT": str(root)}.items():
        monkeypatch.setenv(k, v)
    folder = tmp_path / "res" / "Dataset900_Regions" / "nnUNetTrainer_GIN__nnUNetPlans__3d_fullres"
    (folder / "fold_0").mkdir(parents=True)
    json.dump(KITS, open(folder / "dataset.json", "w"))
    (folder / "fold_0" / "checkpoint_final.pth").write_bytes(b"never read")
    return root, folder


def _files(root):
    return sorted(str(p.relative_to(root)) for p in root.rglob("*"))


def test_prepare_tta_refuses_a_region_model_before_writing(tmp_path, monkeypatch):
    root, _ = _nnunet_tree(tmp_path, monkeypatch)
    from dg_tta_amd.run import DGTTAProgram
    before = _files(tmp_path)
    with pytest.raises(NotImplementedError, match="region-based model.*masked softmax"):
        DGTTAProgram(["dgtta", "prepare_tta", "900", "803", "--pretrainer", "nnUNetTrainer_GIN"])
    assert _files(tmp_path) == before


def test_run_tta_refuses_a_region_model_before_writing(tmp_path, monkeypatch):
    root, folder = _nnunet_tree(tmp_path, monkeypatch)
    from dg_tta_amd.tta.tta import tta_main
    config = {"pretrained_weights_filepath": str(folder / "fold_0" / "checkpoint_final.pth")}
    before = _files(tmp_path)
    with pytest.raises(NotImplementedError, match="region-based model.*masked softmax"):
        tta_main("run", config, tmp_path, root / "results", {}, None, "cuda")
    # an injected network bundle is judged by its predictor's dataset.json
    bundle = (SimpleNamespace(dataset_json=KITS), [8, 8, 8], None, [])
    with pytest.raises(NotImplementedError, match="region-based model"):
        tta_main("run", {}, tmp_path, root / "results", {}, None, "cuda", network_bundle=bundle)
    assert _files(tmp_path) == before
    # the command line refuses as well, from the plan's weights path
    from dg_tta_amd.run import DGTTAProgram
    from dg_tta_amd.tta.config_log_utils import get_tta_folders
    _, plan_dir, _, _, _ = get_tta_folders(900, 803, "nnUNetTrainer_GIN", "3d_fullres", 0)
    plan_dir.mkdir(parents=True)
    json.dump(config, open(plan_dir / "tta_plan.json", "w"))
    before = _files(tmp_path)
    with pytest.raises(NotImplementedError, match="region-based model"):
        DGTTAProgram(["dgtta", "run_tta", "900", "803", "--pretrainer", "nnUNetTrainer_GIN"])
    assert _files(tmp_path) == before
