"""Host side of `dgtta predict` (no GPU): the case list, the argument parser, the model folder and the refusals that must come
before anything is read or written."""
import json

import numpy as np
import pytest


def _touch(folder, *names):
    folder.mkdir(parents=True, exist_ok=True)
    for n in names:
        (folder / n).write_bytes(b"")


def test_list_cases_strips_the_channel_suffix_and_sorts(tmp_path):
    from dg_tta_amd.predict import list_cases
    _touch(tmp_path, "b_case_0000.nii.gz", "a_case_0000.nrrd", "plain.mha", "arr_0000.npy", "zed.npz", "notes.txt", "weights.pt",
           "c.case.v2_0000.nii")
    (tmp_path / "sub_0000.nii.gz").mkdir()                    # a folder is no case
    cases = list_cases(tmp_path)
    assert [c for c, _ in cases] == ["a_case", "arr", "b_case", "c.case.v2", "plain", "zed"]      # sorted by file name
    assert [f.name for _, f in cases] == ["a_case_0000.nrrd", "arr_0000.npy", "b_case_0000.nii.gz", "c.case.v2_0000.nii", "plain.mha",
                                          "zed.npz"]
    assert list_cases(tmp_path / "sub_0000.nii.gz") == []
    with pytest.raises(FileNotFoundError):
        list_cases(tmp_path / "nowhere")


def test_list_cases_refuses_a_second_channel_and_a_doubled_case(tmp_path):
    from dg_tta_amd.predict import list_cases
    _touch(tmp_path / "multi", "ct_0000.nii.gz", "ct_0001.nii.gz")
    with pytest.raises(NotImplementedError, match="image channels"):
        list_cases(tmp_path / "multi")
    _touch(tmp_path / "lonely", "ct_0003.npy")
    with pytest.raises(NotImplementedError, match="image channels"):
        list_cases(tmp_path / "lonely")
    _touch(tmp_path / "twice", "ct_0000.nii.gz", "ct.nii.gz")
    with pytest.raises(ValueError, match="same case"):
        list_cases(tmp_path / "twice")


def test_parser_defaults_are_nnunetv2_predicts():
    from dg_tta_amd.run import DGTTAProgram
    p = DGTTAProgram._predict_parser()
    a = p.parse_args(["-i", "in", "-o", "out", "-d", "820", "-c", "3d_fullres"])
    assert (a.input_folder, a.output_folder, a.dataset_id, a.configuration) == ("in", "out", "820", "3d_fullres")
    assert (a.trainer, a.plans, a.folds, a.checkpoint_name) == ("nnUNetTrainer", "nnUNetPlans", ["0", "1", "2", "3", "4"],
                                                                "checkpoint_final.pth")
    assert (a.disable_mirroring, a.save_probabilities, a.continue_prediction, a.device, a.dtype) == (False, False, False, "cuda", "fp32")
    base = ["-i", "in", "-o", "out", "-d", "820", "-c", "3d_fullres"]
    assert p.parse_args(base + ["-f", "all"]).folds == ["all"]
    assert p.parse_args(base + ["-f", "0", "3"]).folds == ["0", "3"]
    assert p.parse_args(base + ["--disable_tta"]).disable_mirroring is True
    assert p.parse_args(base + ["--disable_mirroring"]).disable_mirroring is True
    b = p.parse_args(base + ["-tr", "nnUNetTrainer_GIN_MIND", "-p", "myPlans", "-chk", "checkpoint_best.pth", "--save_probabilities",
                             "--continue_prediction", "--dtype", "fp16", "--device", "cuda:1"])
    assert (b.trainer, b.plans, b.checkpoint_name, b.save_probabilities, b.continue_prediction, b.dtype, b.device) == \
        ("nnUNetTrainer_GIN_MIND", "myPlans", "checkpoint_best.pth", True, True, "fp16", "cuda:1")
    for gone in (["-npp", "2"], ["-nps", "2"], ["-num_parts", "2"], ["-part_id", "0"], ["-prev_stage_predictions", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + gone)
    for missing in (base[2:], base[:2] + base[4:], base[:4] + base[6:], base[:6]):
        with pytest.raises(SystemExit):
            p.parse_args(missing)


def _model_folder(root, folds):
    from dg_tta_amd.predict import model_folder_of
    folder = model_folder_of("Dataset830_Host", "3d_fullres")
    assert folder == root / "results" / "Dataset830_Host" / "nnUNetTrainer__nnUNetPlans__3d_fullres"
    for k in folds:
        (folder / f"fold_{k}").mkdir(parents=True)
        (folder / f"fold_{k}" / "checkpoint_final.pth").write_bytes(b"")
    json.dump({"labels": {"background": 0, "a": 1}}, open(folder / "dataset.json", "w"))
    return folder


def test_a_missing_fold_is_reported_by_file_name_before_anything_is_read(tmp_path, monkeypatch):
    from dg_tta_amd.predict import checkpoint_files, model_folder_of, predict_from_model_folder
    from dg_tta_amd.run import DGTTAProgram
    monkeypatch.setenv("nnUNet_results", str(tmp_path / "results"))
    monkeypatch.setenv("DG_TTA_ROOT", str(tmp_path))
    folder = _model_folder(tmp_path, [0, "all"])
    assert model_folder_of("830", "3d_lowres", "nnUNetTrainer_GIN", "otherPlans").name == "nnUNetTrainer_GIN__otherPlans__3d_lowres"
    assert [f.parent.name for f in checkpoint_files(folder, [0, "all"])] == ["fold_0", "fold_all"]
    missing = str(folder / "fold_3" / "checkpoint_final.pth")
    with pytest.raises(FileNotFoundError) as e:
        checkpoint_files(folder, [0, 3])
    assert missing in str(e.value)
    with pytest.raises(FileNotFoundError, match="checkpoint_best.pth"):
        checkpoint_files(folder, [0], "checkpoint_best.pth")
    out = tmp_path / "out"
    with pytest.raises(FileNotFoundError) as e:        # the input folder does not even exist: the fold is looked at first
        predict_from_model_folder(folder, tmp_path / "no_input", out, folds=(0, 3))
    assert missing in str(e.value) and not out.exists()
    with pytest.raises(SystemExit) as e:
        DGTTAProgram(["dgtta", "predict", "-i", str(tmp_path / "no_input"), "-o", str(out), "-d", "830", "-c", "3d_fullres", "-f", "0", "3"])
    assert missing in str(e.value) and not out.exists()
    with pytest.raises(SystemExit, match="neither a number nor 'all'"):
        DGTTAProgram(["dgtta", "predict", "-i", "x", "-o", str(out), "-d", "830", "-c", "3d_fullres", "-f", "best"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict_from_model_folder(folder, tmp_path / "no_input", out, folds=(0,), device="cpu")
    assert not out.exists()


def test_dgtta_without_arguments_lists_predict(capsys):
    from dg_tta_amd.run import DGTTAProgram
    with pytest.raises(SystemExit):
        DGTTAProgram(["dgtta"])
    text = capsys.readouterr()
    assert "predict" in text.err + text.out and "run_tta" in text.err + text.out
    with pytest.raises(SystemExit):
        DGTTAProgram(["dgtta", "predict", "-h"])
    helped = capsys.readouterr().out
    assert "--disable_tta" in helped and "--disable_mirroring" in helped and "nothing to do with DG-TTA" in " ".join(helped.split())


def test_label_dtype_is_the_smallest_unsigned_type():
    from dg_tta_amd.predict import _label_dtype
    assert _label_dtype(3) is np.uint8 and _label_dtype(255) is np.uint8 and _label_dtype(256) is np.uint16
    assert _label_dtype(65535) is np.uint16 and _label_dtype(65536) is np.uint32


def test_array_cases_with_several_channels_are_refused(tmp_path):
    from dg_tta_amd.predict import _refuse_array_channels
    np.save(tmp_path / "one.npy", np.zeros((1, 4, 5, 6), np.float32))
    np.save(tmp_path / "flat.npy", np.zeros((4, 5, 6), np.float32))
    np.savez(tmp_path / "one.npz", data=np.zeros((1, 4, 5, 6), np.float32))
    for name in ("one.npy", "flat.npy", "one.npz"):
        _refuse_array_channels(tmp_path / name)
    _refuse_array_channels(tmp_path / "never_opened_0000.nii.gz")
    np.save(tmp_path / "two.npy", np.zeros((2, 4, 5, 6), np.float32))
    np.savez(tmp_path / "two.npz", data=np.zeros((3, 4, 5, 6), np.float32))
    for name in ("two.npy", "two.npz"):
        with pytest.raises(NotImplementedError, match="image channels"):
            _refuse_array_channels(tmp_path / name)


def test_paste_label_map_picks_the_type_from_the_largest_label():
    from dg_tta_amd.tta.inference import _paste_label_map
    props = {"shape_before_cropping": (3, 3, 3), "bbox_used_for_cropping": [[1, 3], [0, 2], [1, 3]]}
    plans = {"transpose_backward": [2, 0, 1]}
    for top, dtype in ((3, np.uint8), (254, np.uint8), (255, np.uint16), (65535, np.uint16), (65536, np.uint32), (70000, np.uint32)):
        out = _paste_label_map(np.full((2, 2, 2), top, np.int32), 3, props, plans, max_label=top)
        assert out.dtype == dtype and out.shape == (3, 3, 3) and int(out.max()) == top and (out != 0).sum() == 8
    assert _paste_label_map(np.ones((2, 2, 2), np.int32), 300, props, plans).dtype == np.uint16      # class ids: C - 1 decides
    assert _paste_label_map(np.ones((2, 2, 2), np.int32), 4, props, plans).dtype == np.uint8
