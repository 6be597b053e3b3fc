"""Properties every plan of dg_tta_amd/planning/planner.py must have, on three synthetic fingerprints: an anisotropic one
(about [5, 0.78, 0.78] mm, median [40, 512, 512]; the target-spacing branch the TS104 fixture never reaches), a tiny isotropic
one (median 40^3) and a large one that triggers `3d_lowres` and the cascade."""
import json

import numpy as np
import pytest

from dg_tta_amd.planning.planner import fullres_target_spacing, get_pool_and_conv_props, plan_experiment
from dg_tta_amd.tta.nnunet_utils import unet_cfg_from_plans

INTENSITY = {"0": {"max": 3000.0, "mean": 50.0, "median": 40.0, "min": -1000.0, "percentile_00_5": -900.0, "percentile_99_5": 1200.0,
                   "std": 300.0}}


def _fingerprint(shapes, spacings, relative=1.0):
    return {"foreground_intensity_properties_per_channel": INTENSITY, "median_relative_size_after_cropping": relative,
            "shapes_after_crop": [list(map(int, s)) for s in shapes], "spacings": [list(map(float, s)) for s in spacings]}


def _dataset_json(n, channel="CT", labels=4):
    return {"labels": {("background" if i == 0 else f"organ{i}"): i for i in range(labels)}, "file_ending": ".nii.gz",
            "channel_names": {"0": channel}, "numTraining": n}


def _cases():
    rng = np.random.default_rng(3)
    n = 30
    aniso = _fingerprint([[40 + int(d), 512, 512] for d in rng.integers(-6, 7, n)],
                         [[5.0 + 0.25 * float(d), 0.78 + 0.01 * float(e), 0.78 + 0.01 * float(e)]
                          for d, e in zip(rng.integers(-2, 3, n), rng.integers(-2, 3, n))])
    tiny = _fingerprint([[40 + int(d), 40, 40 - int(d)] for d in rng.integers(-2, 3, n)], [[1.5, 1.5, 1.5]] * n)
    large = _fingerprint([[600 + 8 * int(d), 512, 512] for d in rng.integers(-5, 6, n)], [[1.0, 0.8, 0.8]] * n)
    return {"anisotropic": (aniso, _dataset_json(n)), "tiny": (tiny, _dataset_json(n)), "large": (large, _dataset_json(n, labels=12))}


CASES = _cases()


def _configurations(plans):
    return {k: v for k, v in plans["configurations"].items() if "inherits_from" not in v}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_properties(name):
    fingerprint, dataset_json = CASES[name]
    plans = plan_experiment(fingerprint, dataset_json)
    assert sorted(plans["transpose_forward"]) == [0, 1, 2]
    assert [plans["transpose_forward"][i] for i in plans["transpose_backward"]] == [0, 1, 2]
    assert "3d_fullres" in plans["configurations"] and "2d" not in plans["configurations"]
    for cname, conf in _configurations(plans).items():
        pools, kernels = conf["pool_op_kernel_sizes"], conf["conv_kernel_sizes"]
        assert len(pools) == len(kernels) == len(conf["n_conv_per_stage_encoder"]) == len(conf["n_conv_per_stage_decoder"]) + 1
        assert pools[0] == [1, 1, 1], "stage 0 is unpooled"
        assert all(p in (1, 2) for pool in pools for p in pool)
        assert all(k in ([1, 3, 3], [3, 3, 3]) for k in kernels), kernels
        assert conf["num_pool_per_axis"] == [sum(p[a] == 2 for p in pools) for a in range(3)]
        for size, n in zip(conf["patch_size"], conf["num_pool_per_axis"]):
            assert size % 2 ** n == 0 and size // 2 ** n >= 4, (cname, conf["patch_size"], conf["num_pool_per_axis"])
        assert conf["batch_size"] >= 2
        assert all(p <= int(np.ceil(m / 2 ** n) * 2 ** n) for p, m, n in
                   zip(conf["patch_size"], conf["median_image_size_in_voxels"], conf["num_pool_per_axis"]))
    for cname in plans["configurations"]:
        cfg, patch = unet_cfg_from_plans(plans, dataset_json, cname, in_channels=1)
        assert cfg["num_classes"] == len(dataset_json["labels"]) and len(patch) == 3
    assert json.loads(json.dumps(plans)) == plans
    assert plan_experiment(fingerprint, dataset_json) == plans, "the planner is deterministic"


def test_anisotropic_plan():
    fingerprint, dataset_json = CASES["anisotropic"]
    target = fullres_target_spacing(fingerprint)
    spacings = np.array(fingerprint["spacings"])
    assert target[0] == pytest.approx(np.percentile(spacings[:, 0], 10)) and target[0] >= target[1:].max()
    assert list(target[1:]) == list(np.median(spacings, 0)[1:])
    conf = plan_experiment(fingerprint, dataset_json)["configurations"]["3d_fullres"]
    assert conf["conv_kernel_sizes"][0] == [1, 3, 3] and conf["pool_op_kernel_sizes"][1] == [1, 2, 2]
    assert conf["num_pool_per_axis"][0] < conf["num_pool_per_axis"][1]


def test_lowres_only_when_the_patch_is_small():
    tiny = plan_experiment(*CASES["tiny"])
    assert sorted(tiny["configurations"]) == ["3d_fullres"] and tiny["configurations"]["3d_fullres"]["batch_dice"] is False
    large = plan_experiment(*CASES["large"])
    assert sorted(large["configurations"]) == ["3d_cascade_fullres", "3d_fullres", "3d_lowres"]
    full, low = large["configurations"]["3d_fullres"], large["configurations"]["3d_lowres"]
    assert full["batch_dice"] is True and low["batch_dice"] is False and low["next_stage"] == "3d_cascade_fullres"
    assert large["configurations"]["3d_cascade_fullres"] == {"inherits_from": "3d_fullres", "previous_stage": "3d_lowres"}
    assert np.prod(full["patch_size"]) / np.prod(full["median_image_size_in_voxels"]) < 0.25
    assert np.prod(low["patch_size"]) / np.prod(low["median_image_size_in_voxels"]) >= 0.25
    assert all(a >= b for a, b in zip(low["spacing"], full["spacing"]))


def test_pool_and_conv_props_of_a_known_patch():
    num_pool, pools, kernels, patch, div = get_pool_and_conv_props([1.5, 1.5, 1.5], [112, 112, 128])
    assert num_pool == [4, 4, 4] and patch == [112, 112, 128] and div == [16, 16, 16] and kernels == [[3, 3, 3]] * 5
    num_pool, pools, kernels, patch, div = get_pool_and_conv_props([5.0, 0.78, 0.78], [20, 250, 250])
    assert kernels[0] == [1, 3, 3] and pools[1] == [1, 2, 2] and all(p % d == 0 for p, d in zip(patch, div))


def test_normalization_table():
    fingerprint, _ = CASES["tiny"]
    for channel, scheme in (("CT", "CTNormalization"), ("ct", "CTNormalization"), ("noNorm", "NoNormalization"), ("T1", "ZScoreNormalization")):
        conf = plan_experiment(fingerprint, _dataset_json(30, channel))["configurations"]["3d_fullres"]
        assert conf["normalization_schemes"] == [scheme] and conf["use_mask_for_norm"] == [False]
    cropped = dict(fingerprint, median_relative_size_after_cropping=0.5)
    assert plan_experiment(cropped, _dataset_json(30, "T1"))["configurations"]["3d_fullres"]["use_mask_for_norm"] == [True]
    assert plan_experiment(cropped, _dataset_json(30, "CT"))["configurations"]["3d_fullres"]["use_mask_for_norm"] == [False]


@pytest.mark.parametrize("channel", ["rescale_to_0_1", "rgb_to_0_1", "", 7])
def test_a_channel_whose_scheme_cannot_run_is_refused(channel):
    """Not "any unknown name": a name nnU-Net does not know is z-scored, as nnU-Net does (test_normalization_table).  Refused
    are the names nnU-Net maps to a scheme preprocessing.normalize does not run, and values that are no names at all - instead
    of plans whose first preprocessing call fails."""
    fingerprint, _ = CASES["tiny"]
    with pytest.raises(ValueError, match="channel"):
        plan_experiment(fingerprint, _dataset_json(30, channel))
