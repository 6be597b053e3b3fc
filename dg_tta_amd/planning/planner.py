"""Experiment planner: dataset fingerprint -> nnUNetPlans.json, the job of nnU-Net 2.2.1's ExperimentPlanner [3P nnunetv2==2.2.1:
experiment_planning/experiment_planners/default_experiment_planner.py, network_topology.py; dynamic_network_architectures:
PlainConvUNet.compute_conv_feature_map_size].  nnunetv2 is not installed here: restated from its published behaviour.

PINNED: tests/test_planner_ts104.py feeds the fingerprint nnU-Net wrote for Dataset505_TS104 (650 cases) and compares the
`3d_fullres`, `3d_lowres` and `3d_cascade_fullres` configurations with the plans nnU-Net wrote from it, field by field.
UNPINNED (that isotropic CT fixture never reaches them): the anisotropic target-spacing branch, the normalisation-scheme table
for names other than CT, use_mask_for_norm.  Left out: the `2d` configuration (the engine has no 2-D kernels), the ResEnc
planners, the `architecture` schema of nnU-Net >= 2.4.  `3d_lowres` and the cascade are planned and written; training the
cascade is not built.  Host only: numpy on a few thousand numbers."""
from copy import deepcopy

import numpy as np

from ..tta.preprocessing import compute_new_shape

BASE_NUM_FEATURES = 32
MAX_NUM_FEATURES_3D = 320
MIN_FEATURE_MAP_EDGE = 4
BLOCKS_PER_STAGE = 2                    # encoder and decoder
VRAM_REFERENCE_VALUE_3D = 560000000
REFERENCE_BATCH_SIZE_3D = 2
VRAM_TARGET_GB, VRAM_REFERENCE_GB = 8, 8
MIN_BATCH_SIZE = 2
MAX_DATASET_SHARE_PER_BATCH = 0.05
LOWRES_THRESHOLD = 0.25
LOWRES_SPACING_STEP = 1.03
ANISOTROPY_THRESHOLD = 3

# channel name (lower case) -> scheme, as nnU-Net maps it; any other name is z-scored.  preprocessing.normalize runs the three
# schemes of RUNNABLE_SCHEMES; a name that asks for another one is refused by the planner, not by the first preprocessing call.
CHANNEL_NAME_TO_SCHEME = {"ct": "CTNormalization", "nonorm": "NoNormalization", "zscore": "ZScoreNormalization",
                          "rescale_to_0_1": "RescaleTo01Normalization", "rgb_to_0_1": "RGBTo01Normalization"}
RUNNABLE_SCHEMES = ("CTNormalization", "NoNormalization", "ZScoreNormalization")
MASKED_SCHEMES = ("ZScoreNormalization",)       # schemes that leave the voxels outside the non-zero mask at zero

_RESAMPLING = {
    "resampling_fn_data": "resample_data_or_seg_to_shape",
    "resampling_fn_seg": "resample_data_or_seg_to_shape",
    "resampling_fn_data_kwargs": {"is_seg": False, "order": 3, "order_z": 0, "force_separate_z": None},
    "resampling_fn_seg_kwargs": {"is_seg": True, "order": 1, "order_z": 0, "force_separate_z": None},
    "resampling_fn_probabilities": "resample_data_or_seg_to_shape",
    "resampling_fn_probabilities_kwargs": {"is_seg": False, "order": 1, "order_z": 0, "force_separate_z": None},
}


def channel_schemes(dataset_json):
    """The normalisation scheme per channel of dataset.json's channel_names (`modality` in old files); ValueError for a
    dataset.json the planner cannot plan.  Needs no fingerprint: `dgtta plan` calls it before it reads a voxel."""
    if not isinstance(dataset_json.get("labels"), dict) or len(dataset_json["labels"]) < 2:
        raise ValueError("plan_experiment: dataset.json needs `labels` with the background and at least one more label")
    names = dataset_json.get("channel_names", dataset_json.get("modality"))
    if not isinstance(names, dict) or not names:
        raise ValueError("plan_experiment: dataset.json has no channel_names")
    schemes = []
    for c in range(len(names)):
        if str(c) not in names or not isinstance(names[str(c)], str) or not names[str(c)].strip():
            raise ValueError(f"plan_experiment: channel_names {names} must name the channels '0' .. '{len(names) - 1}'")
        name = names[str(c)]
        scheme = CHANNEL_NAME_TO_SCHEME.get(name.casefold(), "ZScoreNormalization")
        if scheme not in RUNNABLE_SCHEMES:
            raise ValueError(f"plan_experiment: channel {c} is named {name!r}, for which nnU-Net plans {scheme}; the preprocessing "
                             f"here runs {', '.join(RUNNABLE_SCHEMES)} only")
        schemes.append(scheme)
    return schemes


def normalization_schemes(fingerprint, dataset_json):
    """(schemes, use_mask_for_norm) per channel."""
    schemes = channel_schemes(dataset_json)
    small = fingerprint["median_relative_size_after_cropping"] < (3 / 4.0)
    return schemes, [bool(small and s in MASKED_SCHEMES) for s in schemes]


def fullres_target_spacing(fingerprint):
    """Per-axis median spacing; the coarse axis of a strongly anisotropic dataset takes the 10th percentile of its spacings."""
    spacings = np.vstack(fingerprint["spacings"]).astype(np.float64)
    sizes = np.vstack(fingerprint["shapes_after_crop"]).astype(np.float64)
    target = np.percentile(spacings, 50, 0)
    target_size = np.percentile(sizes, 50, 0)
    worst = int(np.argmax(target))
    others = [i for i in range(len(target)) if i != worst]
    other_spacings = [target[i] for i in others]
    other_sizes = [target_size[i] for i in others]
    if target[worst] > ANISOTROPY_THRESHOLD * max(other_spacings) and target_size[worst] * ANISOTROPY_THRESHOLD < min(other_sizes):
        coarse = np.percentile(spacings[:, worst], 10)
        if coarse < max(other_spacings):            # never finer than in plane
            coarse = max(max(other_spacings), coarse) + 1e-5
        target[worst] = coarse
    return target


def get_pool_and_conv_props(spacing, patch_size, min_edge=MIN_FEATURE_MAP_EDGE):
    """(num_pool_per_axis, pool_op_kernel_sizes, conv_kernel_sizes, padded patch, divisors) of a patch at a spacing."""
    dim = len(spacing)
    cur_spacing = [float(s) for s in spacing]
    cur_size = [float(s) for s in patch_size]
    pools, kernels = [[1] * dim], []
    num_pool = [0] * dim
    kernel = [1] * dim
    while True:
        valid = [i for i in range(dim) if cur_size[i] >= 2 * min_edge]
        if not valid:
            break
        finest = min(cur_spacing[i] for i in valid)
        valid = [i for i in valid if cur_spacing[i] / finest < 2]
        if len(valid) == 1 and cur_size[valid[0]] < 3 * min_edge:
            break
        if not valid:
            break
        for d in range(dim):
            if kernel[d] != 3 and cur_spacing[d] / min(cur_spacing) < 2:
                kernel[d] = 3
        pool = [1] * dim
        for v in valid:
            pool[v] = 2
            num_pool[v] += 1
            cur_spacing[v] *= 2
            cur_size[v] = float(np.ceil(cur_size[v] / 2))
        pools.append(pool)
        kernels.append(list(kernel))
    kernels.append([3] * dim)
    div = [2 ** n for n in num_pool]
    padded = [int(s) if s % d == 0 else int(s + d - s % d) for s, d in zip(patch_size, div)]
    return num_pool, pools, kernels, padded, div


def feature_map_estimate(patch_size, pools, features, num_classes, n_conv=BLOCKS_PER_STAGE):
    """PlainConvUNet(deep_supervision=True).compute_conv_feature_map_size(patch_size): the count nnU-Net takes for the memory of
    a configuration.  Encoder: every conv of a stage at the stage's output size; decoder, per skip: its convs, the transposed
    conv and the stage's segmentation head at the skip's size."""
    size = [int(s) for s in patch_size]
    skips, total = [], 0
    for stage, pool in enumerate(pools):
        size = [s // p for s, p in zip(size, pool)]
        total += n_conv * features[stage] * int(np.prod(size, dtype=np.int64))
        skips.append(list(size))
    for stage in range(len(pools) - 1):
        voxels = int(np.prod(skips[stage], dtype=np.int64))
        total += n_conv * features[stage] * voxels + features[stage] * voxels + num_classes * voxels
    return total


def plan_configuration(spacing, median_shape, data_identifier, approximate_n_voxels, schemes, use_mask, num_classes):
    """One 3-D configuration at `spacing` for a dataset whose median case has `median_shape` voxels."""
    spacing = np.array(spacing, dtype=np.float64)
    if not (spacing > 0).all():
        raise ValueError(f"plan_experiment: spacing {spacing.tolist()} must be positive")
    median = np.array(median_shape, dtype=np.float64)
    tmp = 1 / spacing
    initial = [round(float(i)) for i in tmp * (256 ** 3 / np.prod(tmp)) ** (1 / 3)]
    initial = np.array([min(i, j) for i, j in zip(initial, median)])
    reference = VRAM_REFERENCE_VALUE_3D * (VRAM_TARGET_GB / VRAM_REFERENCE_GB)

    def props(patch):
        num_pool, pools, kernels, patch, div = get_pool_and_conv_props(spacing, patch)
        feats = [min(MAX_NUM_FEATURES_3D, BASE_NUM_FEATURES * 2 ** i) for i in range(len(pools))]
        return num_pool, pools, kernels, np.array(patch), div, feature_map_estimate(patch, pools, feats, num_classes)

    num_pool, pools, kernels, patch, div, estimate = props(initial)
    while estimate > reference:
        axis = int(np.argsort(patch / median)[-1])
        tentative = patch.copy()
        tentative[axis] -= div[axis]
        div = get_pool_and_conv_props(spacing, tentative)[4]      # the divisor the axis has at the reduced size
        patch[axis] -= div[axis]
        num_pool, pools, kernels, patch, div, estimate = props(patch)
    batch = round((reference / estimate) * REFERENCE_BATCH_SIZE_3D)
    cap = round(approximate_n_voxels * MAX_DATASET_SHARE_PER_BATCH / np.prod(patch, dtype=np.float64))
    batch = max(min(batch, cap), MIN_BATCH_SIZE)
    stages = len(pools)
    plan = {
        "data_identifier": data_identifier,
        "preprocessor_name": "DefaultPreprocessor",
        "batch_size": int(batch),
        "patch_size": [int(p) for p in patch],
        "median_image_size_in_voxels": [int(m) if isinstance(m, (int, np.integer)) else float(m) for m in median_shape],
        "spacing": [float(s) for s in spacing],
        "normalization_schemes": list(schemes),
        "use_mask_for_norm": list(use_mask),
        "UNet_class_name": "PlainConvUNet",
        "UNet_base_num_features": BASE_NUM_FEATURES,
        "n_conv_per_stage_encoder": [BLOCKS_PER_STAGE] * stages,
        "n_conv_per_stage_decoder": [BLOCKS_PER_STAGE] * (stages - 1),
        "num_pool_per_axis": [int(n) for n in num_pool],
        "pool_op_kernel_sizes": [list(p) for p in pools],
        "conv_kernel_sizes": [list(k) for k in kernels],
        "unet_max_num_features": MAX_NUM_FEATURES_3D,
    }
    plan.update(deepcopy(_RESAMPLING))
    return plan


def plan_experiment(fingerprint, dataset_json, plans_name="nnUNetPlans", dataset_name=None):
    """The plans dict nnU-Net 2.2.1's ExperimentPlanner writes for this fingerprint and dataset.json, without its `2d` entry.
    fingerprint: the dict of dataset_fingerprint.json; its intensity block is passed through unchanged."""
    for key in ("spacings", "shapes_after_crop", "median_relative_size_after_cropping", "foreground_intensity_properties_per_channel"):
        if key not in fingerprint:
            raise ValueError(f"plan_experiment: the fingerprint has no {key!r}")
    spacings, shapes = fingerprint["spacings"], fingerprint["shapes_after_crop"]
    if len(spacings) == 0 or len(spacings) != len(shapes) or any(len(s) != 3 for s in list(spacings) + list(shapes)):
        raise ValueError("plan_experiment: one 3-D spacing and shape per training case expected")
    schemes, use_mask = normalization_schemes(fingerprint, dataset_json)
    num_classes = len(dataset_json["labels"])
    num_training = int(dataset_json.get("numTraining", len(spacings)))

    target = fullres_target_spacing(fingerprint)
    forward = [int(np.argmax(target))] + [i for i in range(3) if i != int(np.argmax(target))]
    backward = [forward.index(i) for i in range(3)]
    target_t = target[forward]
    new_shapes = [compute_new_shape(shape, spacing, target) for spacing, shape in zip(spacings, shapes)]
    median_t = np.median(np.array(new_shapes), 0)[forward]
    if median_t[0] == 1:
        raise NotImplementedError("plan_experiment: the median case is one slice thick; nnU-Net plans `2d` only, which is not built here")
    approximate_n_voxels = float(np.prod(median_t, dtype=np.float64) * num_training)

    def identifier(configuration):
        return f"{plans_name}_{configuration}"

    fullres = plan_configuration(target_t, median_t, identifier("3d_fullres"), approximate_n_voxels, schemes, use_mask, num_classes)
    fullres_spacing = np.array(fullres["spacing"])
    median_voxels = np.prod(median_t, dtype=np.float64)
    patch_voxels = np.prod(fullres["patch_size"], dtype=np.float64)
    lowres, lowres_spacing = None, fullres_spacing.copy()
    while patch_voxels / median_voxels < LOWRES_THRESHOLD:
        finer = (max(lowres_spacing) / lowres_spacing) > 2
        if finer.any():
            lowres_spacing[finer] *= LOWRES_SPACING_STEP
        else:
            lowres_spacing *= LOWRES_SPACING_STEP
        scaled = fullres_spacing / lowres_spacing * median_t
        median_voxels = np.prod(scaled, dtype=np.float64)
        lowres = plan_configuration(lowres_spacing, [round(float(i)) for i in scaled], identifier("3d_lowres"),
                                    float(median_voxels * num_training), schemes, use_mask, num_classes)
        patch_voxels = np.prod(lowres["patch_size"], dtype=np.int64)

    median_spacing = np.median(np.vstack(spacings).astype(np.float64), 0)[forward]
    median_shape = np.median(np.vstack(shapes).astype(np.float64), 0)[forward]
    plans = {
        "dataset_name": dataset_name if dataset_name is not None else dataset_json.get("name", "Dataset"),
        "plans_name": plans_name,
        "original_median_spacing_after_transp": [float(i) for i in median_spacing],
        "original_median_shape_after_transp": [int(round(float(i))) for i in median_shape],
        "image_reader_writer": "SimpleITKIO",
        "transpose_forward": forward,
        "transpose_backward": backward,
        "configurations": {},
        "experiment_planner_used": "ExperimentPlanner",
        "label_manager": "LabelManager",
        "foreground_intensity_properties_per_channel": deepcopy(fingerprint["foreground_intensity_properties_per_channel"]),
    }
    if lowres is not None:
        lowres["batch_dice"] = False
        lowres["next_stage"] = "3d_cascade_fullres"
        fullres["batch_dice"] = True
        plans["configurations"]["3d_lowres"] = lowres
        plans["configurations"]["3d_fullres"] = fullres
        plans["configurations"]["3d_cascade_fullres"] = {"inherits_from": "3d_fullres", "previous_stage": "3d_lowres"}
    else:
        fullres["batch_dice"] = False
        plans["configurations"]["3d_fullres"] = fullres
    return plans
