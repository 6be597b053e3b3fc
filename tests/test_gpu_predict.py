"""GPU, end to end: `dgtta predict` - fold ensembles of label and region models on a raw NIfTI case, exported to the case's original
geometry - against a CPU reference: the engine's own run_case output (tests/test_preprocessing.py tests it) through
oracle.inference.ensemble_logits, resampled linearly with oracle.preprocessing.resample_data_or_seg, then the restatement
tests/region_export_ref.py (regions) or the argmax (labels).

delta = 2e-4 of the largest logit is what test_ensemble_sliding_window_matches_cpu_restatement holds the ensemble logits to (and
what the fixture holds this file's own networks to).  Labels are compared wherever the decision margin - every |l_i| for regions,
the top-2 gap for labels - exceeds 4 delta; at most 5 % of the voxels inside the crop box may be excluded.  The oracle restatement
on the CPU excludes 0.8 % (regions) and 0.5 % (labels) for unit-normal data of this construction (28 x 20 x 30 resampled to
42 x 20 x 45).  For this file's own case (30 x 26 x 18 resampled to 45 x 39 x 27), preprocessed and predicted by the oracle on the
CPU, the excluded share is 0.63 % (regions, two folds), 0.61 % (regions, fold 0), 0.35 % (labels, two folds); every test prints
the share it finds.

Model folders are written here without training: plans from the skeleton narrowed to two stages (features 32 / 40, 16^3 patch,
spacing 1.5 mm, a permuting transpose_forward), oracle.unet networks with seeds 1 and 2 as fold_0 / fold_1."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import region_export_ref as xref      # noqa: E402
from test_gpu_region_pretrain import DATASET as REGION_DATASET, NAME as LOOP_NAME, _small_plans as _loop_plans, \
    _write_case as _write_loop_case      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]
STOCK, DG = "nnUNetTrainer", "nnUNetTrainer_GIN_MIND"
REGIONS, LABELS, WIDE = "Dataset840_PredictRegions", "Dataset841_PredictLabels", "Dataset842_PredictWide"
LABEL_DATASET = {"labels": {"background": 0, "liver": 1, "spleen": 2, "kidney": 3}, "file_ending": ".nii.gz", "channel_names": {"0": "CT"}}
ORDER = REGION_DATASET["regions_class_order"]
PATCH = [16, 16, 16]
NET = dict(features=(32, 40), strides=(1, 2), n_conv_enc=(2, 2), n_conv_dec=(2,))
RAW_SHAPE = (42, 30, 45)


def _plans():
    plans = json.load(open(ROOT / "dg_tta_amd" / "__resources__" / "model_skeleton" / "plans.json"))
    conf = plans["configurations"]["3d_fullres"]
    conf.update(patch_size=list(PATCH), n_conv_per_stage_encoder=[2, 2], n_conv_per_stage_decoder=[2], UNet_base_num_features=32,
                unet_max_num_features=40, pool_op_kernel_sizes=[[1, 1, 1], [2, 2, 2]], conv_kernel_sizes=[[3, 3, 3]] * 2,
                num_pool_per_axis=[1, 1, 1])
    assert conf["spacing"] == [1.5, 1.5, 1.5]
    plans["transpose_forward"], plans["transpose_backward"] = [2, 0, 1], [1, 2, 0]
    return plans


def _oracle_net(num_classes, seed, in_channels=1):
    from oracle import unet as ounet
    return ounet.perturb_affine(ounet.init_he(ounet.PlainConvUNetOracle(dict(NET, in_channels=in_channels, num_classes=num_classes)), seed),
                                seed + 1)


def _write_model(results, dataset_name, dataset_json, nets, trainer=STOCK, axes=None):
    folder = results / dataset_name / f"{trainer}__nnUNetPlans__3d_fullres"
    folder.mkdir(parents=True)
    json.dump(_plans(), open(folder / "plans.json", "w"))
    json.dump(dataset_json, open(folder / "dataset.json", "w"))
    for k, net in enumerate(nets):
        (folder / f"fold_{k}").mkdir()
        torch.save({"network_weights": net.state_dict(), "trainer_name": trainer, "inference_allowed_mirroring_axes": axes},
                   folder / f"fold_{k}" / "checkpoint_final.pth")
    return folder


def _resampled_reference(members, data, props, plans):
    """[(C, *tgt) float64 per member]: oracle sliding-window logits of each member on the preprocessed case, resampled linearly to
    the shape the case had before resampling."""
    from oracle import inference as oinf, preprocessing as op
    tgt = [int(v) for v in props["shape_after_cropping_and_before_resampling"]]
    do_sep, axis = op.separate_z(list(plans["configurations"]["3d_fullres"]["spacing"]), props["spacing"])
    assert not do_sep
    out = []
    for m in members:
        l = oinf.ensemble_logits([m], torch.from_numpy(data), PATCH).double().numpy()
        out.append(op.resample_data_or_seg(l, tgt, False, axis, 1, do_sep, 0))
    return out


class _World:
    pass


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Two model folders (region, label), one raw case, its preprocessed form and the CPU logits of every member, once."""
    from dg_tta_amd.tta.nifti_io import write_nifti
    from dg_tta_amd.tta.preprocessing import run_case
    w = _World()
    w.root = tmp_path_factory.mktemp("predict")
    w.results = w.root / "results"
    w.region_nets = [_oracle_net(3, 1), _oracle_net(3, 2)]
    w.label_nets = [_oracle_net(4, 1), _oracle_net(4, 2)]
    w.region_folder = _write_model(w.results, REGIONS, REGION_DATASET, w.region_nets)
    w.label_folder = _write_model(w.results, LABELS, LABEL_DATASET, w.label_nets)
    rng = np.random.default_rng(5)
    img = (rng.standard_normal(RAW_SHAPE) * 300.0 + 40.0).astype(np.float32)
    img[:3], img[:, -3:] = 0.0, 0.0                            # zero faces: the crop box is a proper one
    w.images = w.root / "images"
    w.images.mkdir()
    w.image = w.images / "case7_0000.nii.gz"
    write_nifti(w.image, img, spacing=(1.0, 1.0, 1.0))
    w.plans = _plans()
    w.data, _, w.props = run_case([w.image], None, w.plans, "3d_fullres", DEV)
    w.data = np.ascontiguousarray(w.data, dtype=np.float32)
    assert w.data.shape[0] == 1 and min(w.data.shape[1:]) >= 16
    assert [b - a for a, b in w.props["bbox_used_for_cropping"]] == [45, 39, 27]          # (x, z, y) after transpose_forward
    assert tuple(w.props["shape_after_cropping_and_before_resampling"]) != tuple(w.data.shape[1:])
    w.region_ref = _resampled_reference(w.region_nets, w.data, w.props, w.plans)
    w.label_ref = _resampled_reference(w.label_nets, w.data, w.props, w.plans)
    w.inside = np.zeros(w.props["shape_before_cropping"], bool)
    w.inside[tuple(slice(int(a), int(b)) for a, b in w.props["bbox_used_for_cropping"])] = True
    w.inside = w.inside.transpose(w.plans["transpose_backward"])
    assert w.inside.shape == RAW_SHAPE and 0 < w.inside.sum() < w.inside.size
    return w


def _predict(w, mp, dataset, out, *extra, folds=("0", "1"), images=None):
    from dg_tta_amd.run import DGTTAProgram
    mp.setenv("nnUNet_results", str(w.results))
    mp.setenv("DG_TTA_INTERNAL_AUGMENTATION", "false")       # (restored afterwards: load_network switches the global on)
    DGTTAProgram(["dgtta", "predict", "-i", str(images or w.images), "-o", str(out), "-d", dataset, "-c", "3d_fullres", "-f", *folds,
                  "--device", DEV, *extra])
    return out


def _pasted(w, arr):
    """[*tgt] or [K, *tgt] -> the raw geometry: pasted into the zero volume, transposed back."""
    tgt = tuple(int(v) for v in w.props["shape_after_cropping_and_before_resampling"])
    arr = np.asarray(arr)
    lead = arr.shape[:arr.ndim - 3]
    seg, probs = xref.paste_full(np.zeros(tgt), arr.reshape(-1, *tgt), w.props["shape_before_cropping"], w.props["bbox_used_for_cropping"],
                                 w.plans["transpose_backward"])
    return probs.reshape(*lead, *seg.shape)


def _region_reference(w, members):
    """(label map, probabilities [R, ...], safe mask, delta) in the raw geometry for the mean of `members`' resampled logits."""
    l = sum(w.region_ref[m] for m in members) / len(members)
    R = l.shape[0]
    lab, p = xref.region_export(l.reshape(R, -1).T, ORDER, 1.0)
    delta = 2e-4 * np.abs(l).max()
    safe = (np.abs(l) > 4 * delta).all(axis=0)
    return _pasted(w, lab.reshape(l.shape[1:])).astype(np.int64), _pasted(w, p.reshape(l.shape)), _pasted(w, safe).astype(bool), delta


def _label_reference(w, members):
    l = sum(w.label_ref[m] for m in members) / len(members)
    top2 = np.sort(l, axis=0)[-2:]
    delta = 2e-4 * np.abs(l).max()
    return _pasted(w, l.argmax(0)).astype(np.int64), _pasted(w, top2[1] - top2[0] > 4 * delta).astype(bool), delta


def _check_file(w, path, dtype=np.uint8):
    from dg_tta_amd.tta.image_io import read_image
    seg, hdr = read_image(path)
    raw, raw_hdr = read_image(w.image)
    assert seg.shape == raw.shape == RAW_SHAPE and seg.dtype == dtype
    assert tuple(hdr["pixdim"][:3]) == tuple(raw_hdr["pixdim"][:3]) == (1.0, 1.0, 1.0)
    return np.asarray(seg).astype(np.int64)


def _compare(w, seg, want, safe, what):
    excluded = 1.0 - safe[w.inside].mean()
    print(f"{what}: {excluded:.4f} of the voxels inside the box lie within 4 delta of a decision; "
          f"{float((seg != want)[w.inside].mean()):.4f} differ in all")
    assert excluded <= 0.05
    assert np.array_equal(seg[safe], want[safe]) and (seg[~w.inside] == 0).all()


def test_engine_logits_of_this_case_are_within_delta_of_the_oracle(world, monkeypatch):
    """What licenses delta for this file's networks and case: the ensemble-mean logits re-formed from the feature accumulators, in
    the preprocessed geometry, against oracle.inference.ensemble_logits - the bound of test_ensemble_sliding_window_matches_cpu_restatement."""
    from dg_tta_amd.tta import inference as pinf
    from dg_tta_amd.tta.nnunet_utils import load_network
    from oracle import inference as oinf
    monkeypatch.setenv("DG_TTA_INTERNAL_AUGMENTATION", "false")      # (restored afterwards)
    _, patch, net, _ = load_network(world.region_folder / "fold_0" / "checkpoint_final.pth", DEV)
    data = torch.from_numpy(world.data)
    with torch.no_grad():
        feats = pinf.predict_ensemble_features(data, net.to(DEV), [m.state_dict() for m in world.region_nets], patch)
    got = (feats.logits() / feats.nsum[..., None] / 2)[tuple(feats.crop)].permute(3, 0, 1, 2).cpu()
    ref = oinf.ensemble_logits(world.region_nets, data, PATCH)
    err = float((got - ref).abs().max()) / float(ref.abs().max())
    print(f"ensemble logits against the oracle: {err:.2e} of the largest logit")
    assert err < 2e-4


def test_region_model_fold_ensemble(world, tmp_path, monkeypatch):
    out = _predict(world, monkeypatch, "840", tmp_path / "out")
    assert sorted(p.name for p in out.iterdir()) == ["case7.nii.gz", "dataset.json", "plans.json", "predict_args.json"]
    assert json.load(open(out / "dataset.json")) == REGION_DATASET and json.load(open(out / "plans.json")) == world.plans
    args = json.load(open(out / "predict_args.json"))
    assert args["folds"] == [0, 1] and args["use_mirroring"] is True and args["checkpoint_name"] == "checkpoint_final.pth"
    seg = _check_file(world, out / "case7.nii.gz")
    assert set(np.unique(seg).tolist()) <= {0, *ORDER} and len(np.unique(seg)) > 2
    want, _, safe, _ = _region_reference(world, [0, 1])
    _compare(world, seg, want, safe, "region model, folds 0 1")
    # fold 0 alone: the one-member reference, and another map than the ensemble's
    one = _check_file(world, _predict(world, monkeypatch, "840", tmp_path / "one", folds=("0",)) / "case7.nii.gz")
    want1, _, safe1, _ = _region_reference(world, [0])
    _compare(world, one, want1, safe1, "region model, fold 0")
    assert not np.array_equal(one, seg)


def test_label_model_fold_ensemble(world, tmp_path, monkeypatch):
    out = _predict(world, monkeypatch, "841", tmp_path / "out")
    seg = _check_file(world, out / "case7.nii.gz")
    assert set(np.unique(seg).tolist()) <= {0, 1, 2, 3} and len(np.unique(seg)) > 2
    want, safe, _ = _label_reference(world, [0, 1])
    _compare(world, seg, want, safe, "label model, folds 0 1")
    # probabilities of a label model: every class, with the class names, beside the same label file
    soft = _predict(world, monkeypatch, "841", tmp_path / "soft", "--save_probabilities")
    assert (soft / "case7.nii.gz").read_bytes() == (out / "case7.nii.gz").read_bytes()
    with np.load(soft / "case7.npz") as z:
        assert sorted(z.files) == ["class_names", "probabilities"] and list(z["class_names"]) == list(LABEL_DATASET["labels"])
        p = z["probabilities"]
    assert p.dtype == np.float16 and p.shape == (4, *RAW_SHAPE)
    assert (p[0][~world.inside] == 1).all() and (p[1:][:, ~world.inside] == 0).all()
    assert float(np.abs(p.astype(np.float32).sum(0) - 1).max()) < 4 * 2.0 ** -11


def test_region_probabilities_beside_an_unchanged_label_file(world, tmp_path, monkeypatch):
    plain = _predict(world, monkeypatch, "840", tmp_path / "plain")
    soft = _predict(world, monkeypatch, "840", tmp_path / "soft", "--save_probabilities")
    assert (soft / "case7.nii.gz").read_bytes() == (plain / "case7.nii.gz").read_bytes()      # byte for byte
    with np.load(soft / "case7.npz") as z:
        assert sorted(z.files) == ["probabilities", "region_names", "regions_class_order"]
        assert list(z["region_names"]) == ["whole", "core", "centre"] and z["regions_class_order"].tolist() == ORDER
        p = z["probabilities"]
    assert p.dtype == np.float16 and p.shape == (3, *RAW_SHAPE) and (p[:, ~world.inside] == 0).all()
    _, want_p, _, delta = _region_reference(world, [0, 1])
    err = np.abs(p.astype(np.float64) - want_p)[:, world.inside]
    bound = xref.prob_bound(want_p, np.float16)[:, world.inside] + delta / 4
    print(f"region probabilities: max err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


def test_mirroring_follows_the_checkpoint_and_disable_tta_switches_it_off(world, tmp_path, monkeypatch):
    from dg_tta_amd.tta import inference as pinf
    ck = torch.load(world.region_folder / "fold_0" / "checkpoint_final.pth", map_location="cpu", weights_only=False)
    torch.save(dict(ck, inference_allowed_mirroring_axes=[0, 1, 2]), world.region_folder / "fold_0" / "checkpoint_mirror.pth")
    seen = []
    real = pinf.predict_ensemble
    monkeypatch.setattr(pinf, "predict_ensemble", lambda *a, **k: (seen.append(k.get("mirror_axes", "absent")), real(*a, **k))[1])
    common = ("-chk", "checkpoint_mirror.pth")
    a = _check_file(world, _predict(world, monkeypatch, "840", tmp_path / "m", *common, folds=("0",)) / "case7.nii.gz")
    b = _check_file(world, _predict(world, monkeypatch, "840", tmp_path / "p", *common, "--disable_tta", folds=("0",)) / "case7.nii.gz")
    c = _check_file(world, _predict(world, monkeypatch, "840", tmp_path / "q", *common, "--disable_mirroring", folds=("0",)) / "case7.nii.gz")
    assert seen == [(0, 1, 2), None, None]
    assert not np.array_equal(a, b) and np.array_equal(b, c)
    want1, _, safe1, _ = _region_reference(world, [0])                  # without the mirrors it is the plain one-member prediction
    _compare(world, b, want1, safe1, "mirror checkpoint with --disable_tta")
    # folds that disagree on the axes are refused
    torch.save(dict(ck, inference_allowed_mirroring_axes=[0, 1, 2]), world.region_folder / "fold_0" / "checkpoint_odd.pth")
    torch.save(ck, world.region_folder / "fold_1" / "checkpoint_odd.pth")
    with pytest.raises(ValueError, match="inference_allowed_mirroring_axes"):
        _predict(world, monkeypatch, "840", tmp_path / "odd", "-chk", "checkpoint_odd.pth")
    assert not (tmp_path / "odd").exists()


def _members(folder, folds, mp):
    from dg_tta_amd.tta.nnunet_utils import load_network
    mp.setenv("DG_TTA_INTERNAL_AUGMENTATION", "true")        # (restored afterwards: load_network switches the global on)
    loaded = [load_network(folder / f"fold_{k}" / "checkpoint_final.pth", DEV) for k in folds]
    mp.setenv("DG_TTA_INTERNAL_AUGMENTATION", "false")
    return loaded[0][0], loaded[0][2].to(DEV), [l[3][0] for l in loaded]


def test_array_cases_are_predicted_in_the_preprocessed_geometry(world, tmp_path, monkeypatch):
    from dg_tta_amd.tta.inference import run_inference
    arrays = tmp_path / "arrays"
    arrays.mkdir()
    np.save(arrays / "pre_0000.npy", world.data)
    out = _predict(world, monkeypatch, "840", tmp_path / "out", images=arrays)
    got = np.load(out / "pre.npy")
    assert got.dtype == np.uint8 and got.shape == world.data.shape[1:] and not (out / "pre.nii.gz").exists()
    _, net, members = _members(world.region_folder, (0, 1), monkeypatch)
    want = run_inference(torch.from_numpy(world.data), net, members, PATCH, regions_class_order=ORDER).numpy()
    assert np.array_equal(got, want) and len(np.unique(got)) > 2


def test_dg_trainer_folder_predicts_with_its_hooks_and_the_augmentation_off(world, tmp_path, monkeypatch):
    from dg_tta_amd.tta.inference import run_inference
    from dg_tta_amd.utils import get_internal_augmentation_enabled
    folder = _write_model(world.results, LABELS, LABEL_DATASET, [_oracle_net(4, 3, in_channels=12)], trainer=DG)
    arrays = tmp_path / "arrays"
    arrays.mkdir()
    np.save(arrays / "pre.npy", world.data)
    torch.manual_seed(11)                                     # (the MIND noise of the hook is drawn on the device generator)
    out = _predict(world, monkeypatch, "841", tmp_path / "out", "-tr", DG, folds=("0",), images=arrays)
    assert not get_internal_augmentation_enabled()
    got = np.load(out / "pre.npy")
    predictor, net, members = _members(folder, (0,), monkeypatch)
    assert predictor.trainer_name == DG and len(net._forward_pre_hooks) == 2 and predictor.allowed_mirroring_axes is None
    assert net.encoder.stages[0][0].convs[0].conv.weight.shape[1] == 12                   # 12 channels after the hook
    torch.manual_seed(11)
    want = run_inference(torch.from_numpy(world.data), net, members, PATCH).numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want) and len(np.unique(got)) > 1


def test_continue_prediction_leaves_existing_files_alone(world, tmp_path, monkeypatch):
    import shutil
    images = tmp_path / "images"
    images.mkdir()
    shutil.copyfile(world.image, images / "case7_0000.nii.gz")
    out = tmp_path / "out"
    out.mkdir()
    (out / "case7.nii.gz").write_bytes(b"kept")
    os.utime(out / "case7.nii.gz", (1_000_000_000, 1_000_000_000))
    shutil.copyfile(world.image, images / "case8_0000.nii.gz")
    _predict(world, monkeypatch, "840", out, "--continue_prediction", folds=("0",), images=images)
    assert (out / "case7.nii.gz").read_bytes() == b"kept" and (out / "case7.nii.gz").stat().st_mtime == 1_000_000_000
    seg = _check_file(world, out / "case8.nii.gz")
    assert len(np.unique(seg)) > 2
    # with probabilities asked for, a case without its .npz is predicted again
    _predict(world, monkeypatch, "840", out, "--continue_prediction", "--save_probabilities", folds=("0",), images=images)
    assert (out / "case7.npz").is_file() and (out / "case8.npz").is_file()
    assert np.array_equal(_check_file(world, out / "case7.nii.gz"), seg)


def test_refusals_come_before_any_output(world, tmp_path, monkeypatch):
    multi = tmp_path / "multi"
    multi.mkdir()
    for ch in ("0000", "0001"):
        (multi / f"case7_{ch}.nii.gz").write_bytes(world.image.read_bytes())
    out = tmp_path / "out"
    with pytest.raises(NotImplementedError, match="image channels"):
        _predict(world, monkeypatch, "840", out, images=multi)
    assert not out.exists()
    arrays = tmp_path / "arrays"
    arrays.mkdir()
    np.save(arrays / "two.npy", np.concatenate([world.data, world.data]))      # an array case with two channels: the same refusal
    with pytest.raises(NotImplementedError, match="image channels"):
        _predict(world, monkeypatch, "840", out, images=arrays)
    assert not out.exists()
    with pytest.raises(SystemExit) as e:
        _predict(world, monkeypatch, "840", out, folds=("0", "1", "2"))
    assert str(world.region_folder / "fold_2" / "checkpoint_final.pth") in str(e.value) and not out.exists()
    wide = dict(LABEL_DATASET, labels={"background": 0, **{f"c{i}": i for i in range(1, 33)}})
    folder = world.results / WIDE / f"{STOCK}__nnUNetPlans__3d_fullres"
    (folder / "fold_0").mkdir(parents=True)
    json.dump(wide, open(folder / "dataset.json", "w"))
    (folder / "fold_0" / "checkpoint_final.pth").write_bytes(b"")      # (never opened: the refusal comes first)
    with pytest.raises(ValueError, match="at most 32 classes"):
        _predict(world, monkeypatch, "842", out, "--save_probabilities", folds=("0",))
    assert not out.exists()


def test_plan_pretrain_predict_closes_the_loop(tmp_path, monkeypatch):
    """`dgtta plan`, one epoch of `dgtta pretrain` on the three 40^3 region cases of tests/test_gpu_region_pretrain.py, then
    `dgtta predict -f 0` on imagesTr.  No learning threshold: two iterations learn nothing worth measuring."""
    from dg_tta_amd.run import DGTTAProgram
    from dg_tta_amd.tta.image_io import read_image
    src = tmp_path / "raw" / LOOP_NAME
    (src / "imagesTr").mkdir(parents=True)
    (src / "labelsTr").mkdir()
    (tmp_path / "dgroot").mkdir()
    for i in range(3):
        _write_loop_case(src / "imagesTr", src / "labelsTr", f"ct{i:02d}", 40, 41 + i)
    json.dump(REGION_DATASET, open(src / "dataset.json", "w"))
    for k, v in {"nnUNet_raw": tmp_path / "raw", "nnUNet_results": tmp_path / "res", "nnUNet_preprocessed": tmp_path / "pre",
                 "DG_TTA_ROOT": tmp_path / "dgroot"}.items():
        monkeypatch.setenv(k, str(v))
    monkeypatch.setenv("DG_TTA_INTERNAL_AUGMENTATION", "false")
    DGTTAProgram(["dgtta", "plan", "820", "--device", DEV])
    pre = tmp_path / "pre" / LOOP_NAME
    json.dump(_loop_plans(), open(pre / "nnUNetPlans.json", "w"))      # (the 32^3 plans of that file in the planner's place)
    json.dump([{"train": ["ct00", "ct01"], "val": ["ct02"]}], open(pre / "splits_final.json", "w"))
    DGTTAProgram(["dgtta", "pretrain", "820", "3d_fullres", "0", "-tr", STOCK, "--num_epochs", "1", "--iterations_per_epoch", "2",
                  "--val_iterations", "1", "--device", DEV, "--seed", "7"])
    out = tmp_path / "predicted"
    DGTTAProgram(["dgtta", "predict", "-i", str(src / "imagesTr"), "-o", str(out), "-d", "820", "-c", "3d_fullres", "-f", "0", "--device", DEV])
    assert sorted(p.name for p in out.iterdir() if p.name.endswith(".nii.gz")) == ["ct00.nii.gz", "ct01.nii.gz", "ct02.nii.gz"]
    for i in range(3):
        seg, hdr = read_image(out / f"ct{i:02d}.nii.gz")
        lab, lab_hdr = read_image(src / "labelsTr" / f"ct{i:02d}.nii.gz")
        assert seg.shape == lab.shape == (40, 40, 40) and seg.dtype == np.uint8
        assert tuple(hdr["pixdim"][:3]) == tuple(lab_hdr["pixdim"][:3]) and np.array_equal(hdr["affine"], lab_hdr["affine"])
        assert set(np.unique(seg).tolist()) <= {0, 1, 2, 3}
