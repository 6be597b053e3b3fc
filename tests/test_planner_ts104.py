"""The planner against nnU-Net's own output.  tests/golden/ts104_dataset_fingerprint.json and ts104_nnUNetPlans.json are the
dataset_fingerprint.json and plans.json that ship, as data, in the model folders of the DG-TTA reference
(dg_tta/__resources__/dummy_results/*/; the six folders hold the same bytes): what nnU-Net 2.2.1's ExperimentPlanner wrote for
Dataset505_TS104 (650 training cases, 105 labels, one CT channel).  Copied unchanged.  dataset.json is the model skeleton's,
which carries numTraining, the labels and the channel name.

plan_experiment(fingerprint, dataset_json) must reproduce the 3-D part of those plans: every compared number by value
(242.5 == 242.5, 182 == 182.0), `spacing` to relative 1e-12 (1.5 * 1.03^8: eight double multiplications whose order may
differ from nnU-Net's, a few ulp at most).  `2d` is not planned here and not compared."""
import json
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"

CONFIG_KEYS = ["patch_size", "batch_size", "median_image_size_in_voxels", "normalization_schemes", "use_mask_for_norm",
               "UNet_class_name", "UNet_base_num_features", "n_conv_per_stage_encoder", "n_conv_per_stage_decoder", "num_pool_per_axis",
               "pool_op_kernel_sizes", "conv_kernel_sizes", "unet_max_num_features", "resampling_fn_data", "resampling_fn_seg",
               "resampling_fn_data_kwargs", "resampling_fn_seg_kwargs", "resampling_fn_probabilities",
               "resampling_fn_probabilities_kwargs", "batch_dice"]


@pytest.fixture(scope="module")
def ts104():
    fingerprint = json.load(open(GOLDEN / "ts104_dataset_fingerprint.json"))
    expected = json.load(open(GOLDEN / "ts104_nnUNetPlans.json"))
    dataset_json = json.load(open(ROOT / "dg_tta_amd" / "__resources__" / "model_skeleton" / "dataset.json"))
    assert dataset_json["numTraining"] == 650 and len(dataset_json["labels"]) == 105 and dataset_json["channel_names"] == {"0": "CT"}
    assert len(fingerprint["spacings"]) == len(fingerprint["shapes_after_crop"]) == 650
    from dg_tta_amd.planning.planner import plan_experiment
    return fingerprint, dataset_json, expected, plan_experiment(fingerprint, dataset_json)


def test_top_level_keys(ts104):
    fingerprint, _, expected, plans = ts104
    for key in ("transpose_forward", "transpose_backward", "original_median_spacing_after_transp", "original_median_shape_after_transp",
                "experiment_planner_used", "label_manager", "image_reader_writer", "plans_name", "dataset_name"):
        assert plans[key] == expected[key], key
    assert plans["foreground_intensity_properties_per_channel"] == fingerprint["foreground_intensity_properties_per_channel"]
    assert plans["foreground_intensity_properties_per_channel"] == expected["foreground_intensity_properties_per_channel"]
    assert sorted(plans["configurations"]) == ["3d_cascade_fullres", "3d_fullres", "3d_lowres"]          # no `2d`


@pytest.mark.parametrize("configuration", ["3d_fullres", "3d_lowres"])
def test_configuration(ts104, configuration):
    _, _, expected, plans = ts104
    got, want = plans["configurations"][configuration], expected["configurations"][configuration]
    for key in CONFIG_KEYS:
        assert got[key] == want[key], (configuration, key, got[key], want[key])
    assert got.get("next_stage") == want.get("next_stage")
    assert got["spacing"] == pytest.approx(want["spacing"], rel=1e-12, abs=0)
    assert got["data_identifier"] == want["data_identifier"] and got["preprocessor_name"] == want["preprocessor_name"]
    assert set(got) == set(want)


def test_cascade(ts104):
    _, _, expected, plans = ts104
    assert plans["configurations"]["3d_cascade_fullres"] == expected["configurations"]["3d_cascade_fullres"]
    assert plans["configurations"]["3d_lowres"]["spacing"][0] == pytest.approx(1.9001551220814243, rel=1e-12)
    assert plans["configurations"]["3d_lowres"]["median_image_size_in_voxels"] == [182, 180, 191]


def test_plans_are_json(ts104):
    plans = ts104[3]
    assert json.loads(json.dumps(plans)) == plans
