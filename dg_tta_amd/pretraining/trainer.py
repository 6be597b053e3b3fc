"""`dgtta pretrain`: source-domain training of a DG trainer's network on this engine, from a dataset folder to
`nnUNet_results/<Dataset>/<trainer>__nnUNetPlans__<configuration>/fold_<k>/checkpoint_final.pth` - the file
`dgtta prepare_tta <numeric id>` looks for (tta/config_log_utils.py) and `load_network` reads.  The reference dispatches
this step into `nnUNetv2_train` (dg_tta/run.py pretrain); nnunetv2 is not needed here.  What nnU-Net's trainer does around
the network is restated from memory of nnunetv2 2.2 (UNPINNED): SGD with Nesterov momentum 0.99, weight decay 3e-5,
gradient-norm clipping at 12 (optim.HipSGD, csrc/sgd.hip), polynomial learning rate from 1e-2 stepped per epoch
(optim.PolyLRScheduler), 250 training + 50 validation iterations per epoch, 33 % of a batch centred on foreground,
DC+CE loss with deep supervision (ops.deep_supervision_loss), online pseudo-Dice from the validation batches.

THE DICE TERM: `dice="sample"` (the default, `--dice sample`) takes it per sample, whatever the plans' `batch_dice` says - when
they say true, BATCH_DICE_NOTE is printed at the start.  `dice="plans"` (`--dice plans`) obeys the resolved configuration's
`batch_dice` (plans_batch_dice: `inherits_from` is followed, a missing key is false): true pools the Dice sums over the batch
before the ratio (csrc/dice_ce.hip; nnU-Net's MemoryEfficientSoftDiceLoss(batch_dice=True) from memory, UNPINNED), in the training
and in the validation loss of every epoch alike.

THE BEST CHECKPOINT: after every epoch the moving average of the pseudo-Dice (ema_step: the first finite value, then
0.9 ema + 0.1 value; a NaN epoch leaves it alone) is logged under `ema_fg_dice`, and when it exceeds every earlier one
checkpoint_best.pth is written beside checkpoint_latest.pth / checkpoint_final.pth (nnU-Net's rule from memory, UNPINNED).
A checkpoint written before the key existed continues: the series is rebuilt from `mean_fg_dice` (rebuild_ema).

THE FINAL VALIDATION (`final_validation=True`, `--validate`; `validate_fold`, `--val` for a fold trained earlier): every validation
case of the fold (fold "all": its training cases, as nnU-Net does) is predicted from its preprocessed `data` with the network
load_network builds from checkpoint_final.pth - the trainer's hooks registered, the internal augmentation off - through the
sliding-window path of tta/inference.py with the checkpoint's mirror axes, argmax over all classes, one case at a time.
fold_<k>/validation/ receives <case>.npy (the label map in the PREPROCESSED geometry, smallest unsigned integer type that holds
the labels) and summary.json in the layout of tta/evaluation.py, against the `seg` of the case's .npz with -1 read as background.
nnU-Net evaluates in the case's original geometry against gt_segmentations/; training here writes no per-case geometry
properties, so the comparison stays in the preprocessed geometry.

REDUCED AUGMENTATION: the DG trainers' own augmentation runs (GIN / MIND forward pre-hooks; for the *_MultiRes trainers
SimulateDiscreteLowResolutionTransform with the reference's arguments, nnUNetTrainer_GIN_MIND_MultiRes.py:61-67), mirroring
is off as those trainers set it, but nnU-Net's rotation / scaling and noise / blur / brightness / contrast / gamma
transforms are NOT applied.  `augmentation="spatial"` (`--augmentation spatial`) adds the rotation / scaling
(pretraining/spatial.py, csrc/spatial_aug.hip); the intensity transforms stay missing.  `augmentation="full"`
(`--augmentation full`) adds both: the rotation / scaling and nnU-Net's noise / blur / brightness / contrast / low-resolution /
gamma chain (pretraining/intensity.py, csrc/intensity_aug.hip), with the *_MultiRes trainers' discrete low-resolution transform
in the chain's low-resolution slot, where the reference puts it.  What `full` still lacks against nnU-Net: elastic deformation
(nnU-Net's default switches it off too); mirroring is off for the DG trainers, as they set it.

THE STOCK TRAINER: `nnUNetTrainer` (TRAINERS = DG_TRAINERS + it) is the baseline the DG trainers are compared with: one image
channel, no hooks, no internal augmentation - and nnU-Net's MirrorTransform (from memory of nnunetv2 2.2 / batchgenerators,
UNPINNED) as the LAST transform of every training batch, after the intensity stages, whatever `augmentation` says: for every batch
item and every axis of trainer_mirror_axes(trainer_name) = (0, 1, 2), independently, image and label are flipped with probability
0.5 (draw_mirror_masks states the draws; one ops.mirror_batch launch, csrc/mirror.hip).  Validation batches are never mirrored.
Its checkpoint carries inference_allowed_mirroring_axes = [0, 1, 2], which sliding-window inference obeys (tta/inference.py); a DG
trainer's carries None, draws nothing for mirroring and runs the code it ran before.  Multi-channel data stays out.  Experiment planning is out of
scope: nnUNetPlans.json must exist.  Random streams are not part of a checkpoint: a continued run draws differently from
an uninterrupted one.

REGION-BASED DATASETS (dg_tta_amd/labels.py: a dataset.json whose label values are lists, plus `regions_class_order`; nnU-Net's
second label model, from memory of nnunetv2 2.2.1, UNPINNED): the head has one sigmoid output per region and no background
channel, the loss is DC+BCE with deep supervision (ops.deep_supervision_region_loss, csrc/region_loss.hip: the kernels read the
integer label map and the membership table, no region target tensor is built), the pseudo-Dice is 2 TP / (2 TP + FP + FN) per
region of the prediction logit > 0 (ops.region_counts) and `mean_fg_dice` / `ema_fg_dice` are its mean over the regions, every
region is a class of the foreground oversampling, the checkpoint records `regions_class_order`, and the final validation writes
the region label map (0, then regions_class_order[i] where output i is positive, in order) and a summary keyed by region.  The
stock trainer and the six DG trainers alike: the hooks do not care what the head means.  `--dice plans` pools the Dice sums of
a region over the batch.  A new image is labelled in its original geometry by `dgtta predict` (dg_tta_amd/predict.py).  Left out:
the ignore label, more than 32 regions, test-time adaptation (prepare_tta / run_tta refuse)."""
import json
import os
import re
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

from .. import ops
from ..labels import label_model
from ..optim import HipSGD, PolyLRScheduler
from ..synthetic import he_init_
from ..tta.config_log_utils import maybe_convert_to_dataset_name, nnunet_path
from ..tta.nnunet_utils import unet_cfg_from_plans
from ..tta.torch_utils import _resident, as_label_map_case, get_batch, release_resident, resident_spline
from ..unet import HipPlainConvUNet
from ..utils import disable_internal_augmentation, numpy_rng
from .discrete_downsampling import SimulateDiscreteLowResolutionTransform
from .hooks import register_dg_hooks, trainer_mirror_axes, trainer_spec
from .intensity import IntensityAugmentation
from .spatial import SpatialAugmentation, patch_start, sampling_map

DG_TRAINERS = tuple(f"nnUNetTrainer_{n}{m}" for m in ("", "_MultiRes") for n in ("GIN", "MIND", "GIN_MIND"))
TRAINERS = DG_TRAINERS + ("nnUNetTrainer",)
INITIAL_LR = 1e-2
OVERSAMPLE_FOREGROUND = 0.33
MAX_LOCATIONS_PER_CLASS = 10000
SAVE_EVERY = 50
RESIDENT_CASES = 64          # cases kept in HBM by get_batch's volume cache; trimmed at epoch ends
REDUCED_AUGMENTATION_NOTE = (
    "pretrain: REDUCED AUGMENTATION - the trainer's own GIN / MIND hooks (and, for *_MultiRes, the discrete low-resolution "
    "transform) run, mirroring is off as the DG trainers set it; nnU-Net's rotation / scaling and noise / blur / brightness / "
    "contrast / gamma transforms are not applied by this engine.")
SPATIAL_AUGMENTATION_NOTE = (
    "pretrain: SPATIAL AUGMENTATION - nnU-Net's rotation / scaling is applied (cubic B-spline image, order-1 labels; "
    "pretraining/spatial.py) beside the trainer's own GIN / MIND hooks (and, for *_MultiRes, the discrete low-resolution "
    "transform), mirroring is off as the DG trainers set it; nnU-Net's noise / blur / brightness / contrast / gamma "
    "transforms are not applied by this engine.")
FULL_AUGMENTATION_NOTE = (
    "pretrain: FULL AUGMENTATION - nnU-Net's rotation / scaling (cubic B-spline image, order-1 labels; pretraining/spatial.py) "
    "and its intensity chain - Gaussian noise, Gaussian blur, brightness, contrast, simulated low resolution, inverted gamma, "
    "gamma (pretraining/intensity.py) - are applied to the training batches beside the trainer's own GIN / MIND hooks; for "
    "*_MultiRes the discrete low-resolution transform takes the chain's low-resolution slot.  Not applied: elastic deformation "
    "and mirroring (off as the DG trainers set it).")
AUGMENTATIONS = ("reduced", "spatial", "full")
MAX_AUG_ITEMS = 16           # items per ops.sample_patches_aug launch
DICE_MODES = ("sample", "plans")
BATCH_DICE_NOTE = (
    "pretrain: PER-SAMPLE DICE - the plans of this configuration say batch_dice: true, which is NOT honoured: the Dice term of the "
    "loss is taken per sample (nnU-Net would pool its sums over the batch).  `--dice plans` (train_fold(dice=\"plans\")) obeys the "
    "plans.")
EMA_DECAY = 0.9


# ------------------------------------------------------------------------------------------------ host logic (no GPU)
def is_forced_foreground(j, batch_size, oversample=OVERSAMPLE_FOREGROUND):
    """nnU-Net's oversampling rule: batch item j is centred on foreground when j >= round(B * (1 - oversample))."""
    return not j < round(batch_size * (1 - oversample))


def make_splits(case_names, n_splits=5, seed=12345):
    """Seeded n-fold split of the sorted case names: numpy RandomState(seed).permutation, cut into n_splits nearly equal
    parts; part k is the validation set of fold k.  NOT sklearn's KFold(shuffle=True) that nnU-Net uses: the folds of an
    nnU-Net run on the same data differ (copy its splits_final.json to reproduce them).  The validation sets partition
    the cases; with fewer cases than folds the last folds have none."""
    names = sorted(case_names)
    perm = np.random.RandomState(seed).permutation(len(names))
    splits = []
    for part in np.array_split(perm, n_splits):
        val = {names[i] for i in part.tolist()}
        splits.append({"train": [n for n in names if n not in val], "val": sorted(val)})
    return splits


def fold_folder_name(fold):
    return f"fold_{fold}"


def class_locations(seg, max_per_class=MAX_LOCATIONS_PER_CLASS, seed=1234, regions=None):
    """{class id > 0: int array [n, 3] of (D, H, W) voxels}, at most max_per_class per class, drawn once per case with a
    seeded generator (nnU-Net samples them at preprocessing time in the same way).
    regions (tuples of label values, a region-based dataset): every region present in the case is a class, keyed by its tuple -
    its voxels are those of isin(seg, region), drawn region by region in the given order from the one generator."""
    if regions is not None:
        arr = np.asarray(seg)
        rs = np.random.RandomState(seed)
        out = {}
        for region in regions:
            idx = np.flatnonzero(np.isin(arr.reshape(-1), list(region)))
            if idx.size == 0:
                continue
            if idx.size > max_per_class:
                idx = idx[rs.choice(idx.size, max_per_class, replace=False)]
            out[tuple(int(x) for x in region)] = np.stack(np.unravel_index(idx, arr.shape), axis=1)
        return out
    flat = np.asarray(seg).reshape(-1)
    order = np.argsort(flat, kind="stable")
    vals, starts = np.unique(flat[order], return_index=True)
    ends = list(starts[1:]) + [flat.size]
    rs = np.random.RandomState(seed)
    out = {}
    for v, a, b in zip(vals.tolist(), starts.tolist(), ends):
        if v <= 0:
            continue
        idx = order[a:b]
        if idx.size > max_per_class:
            idx = idx[rs.choice(idx.size, max_per_class, replace=False)]
        out[int(v)] = np.stack(np.unravel_index(idx, np.asarray(seg).shape), axis=1)
    return out


def draw_center(locations, rng):
    """A random voxel of a random foreground class present in the case; None when the case has no foreground (the patch
    is then drawn at random, as nnU-Net does)."""
    classes = sorted(locations)
    if not classes:
        return None
    loc = locations[classes[int(rng.randint(len(classes)))]]
    return tuple(int(x) for x in loc[int(rng.randint(len(loc)))])


def plans_batch_dice(plans, configuration):
    """The resolved configuration's `batch_dice` (`inherits_from` followed), false when the key is absent."""
    return bool(_configuration(plans, configuration).get("batch_dice", False))


def ema_step(ema, value, decay=EMA_DECAY):
    """nnU-Net's moving average of the pseudo-Dice (from memory, unpinned).  ema: the average so far, None (or NaN) before the first
    finite value; value: this epoch's mean_fg_dice.  The first finite value starts the average, a NaN value leaves it unchanged."""
    if ema is not None and not np.isfinite(ema):
        ema = None
    if not np.isfinite(value):
        return ema
    return float(value) if ema is None else decay * ema + (1.0 - decay) * float(value)


def is_new_best(ema, best):
    """checkpoint_best.pth is written when the average strictly exceeds the best so far (None: there is none yet)."""
    return ema is not None and np.isfinite(ema) and (best is None or ema > best)


def rebuild_ema(mean_fg_dice):
    """(series, best) from a log's mean_fg_dice - what a run logs under `ema_fg_dice` (NaN before the first finite value) and the
    best average it saw (None if none): how a checkpoint without the key is continued."""
    series, ema, best = [], None, None
    for v in mean_fg_dice:
        ema = ema_step(ema, v)
        series.append(float("nan") if ema is None else ema)
        if is_new_best(ema, best):
            best = ema
    return series, best


def best_of(series):
    """The best average of a logged `ema_fg_dice` series: its largest finite entry, None without one."""
    finite = [v for v in series if np.isfinite(v)]
    return max(finite) if finite else None


def _configuration(plans, configuration):
    conf = plans["configurations"][configuration]
    while "inherits_from" in conf:
        parent = dict(plans["configurations"][conf["inherits_from"]])
        parent.update({k: v for k, v in conf.items() if k != "inherits_from"})
        conf = parent
    return conf


def load_dataset_files(dataset_name):
    """(plans, dataset_json, preprocessed dataset folder, raw dataset folder or None)."""
    pre = Path(nnunet_path("nnUNet_preprocessed")) / dataset_name
    raw = Path(os.environ["nnUNet_raw"]) / dataset_name if os.environ.get("nnUNet_raw") else None
    plans_file = pre / "nnUNetPlans.json"
    if not plans_file.is_file():
        raise FileNotFoundError(
            f"{plans_file} not found: `dgtta pretrain` trains from existing plans and does no experiment planning.  Put the "
            f"nnUNetPlans.json of this dataset there (nnUNetv2_plan_and_preprocess writes it; the plans.json of a model trained "
            f"on comparable data, with its patch size and spacing, works too), or run `dgtta plan` on the raw dataset.")
    with open(plans_file) as f:
        plans = json.load(f)
    for folder in (pre, raw):
        if folder is not None and (folder / "dataset.json").is_file():
            with open(folder / "dataset.json") as f:
                return plans, json.load(f), pre, raw
    raise FileNotFoundError(f"dataset.json found neither in {pre} nor in {raw}")


def find_cases(data_dir, raw, file_ending):
    """{case name: (npz path, raw image file or None, raw label file or None)} from the preprocessed folder and imagesTr."""
    cases = {}
    if data_dir.is_dir():
        for p in sorted(data_dir.glob("*.npz")):
            cases[p.name[:-4]] = (p, None, None)
    if raw is not None and (raw / "imagesTr").is_dir():
        for p in sorted((raw / "imagesTr").iterdir()):
            m = re.match(r"(.*)_0000" + re.escape(file_ending) + "$", p.name)
            if m and m.group(1) not in cases:
                cases[m.group(1)] = (data_dir / f"{m.group(1)}.npz", p, raw / "labelsTr" / f"{m.group(1)}{file_ending}")
    return cases


# ------------------------------------------------------------------------------------------------ cases
class _Case:
    def __init__(self, name, data, seg, regions=None):
        seg = np.where(seg < 0, 0, seg)                 # nnU-Net's "outside the non-zero mask" label (-1) trains as background
        self.name = name
        self.tensor = as_label_map_case(torch.from_numpy(np.ascontiguousarray(data[0], dtype=np.float32)),
                                        torch.from_numpy(np.ascontiguousarray(seg[0], dtype=np.float32)))
        self.locations = class_locations(seg[0], regions=regions)


def load_case(name, entry, plans, configuration, device, regions=None):
    """Reads <case>.npz (keys `data` [C, D, H, W], `seg` [1, D, H, W]); a missing file is made from the raw image + label
    with tta/preprocessing.run_case and written first, so there is one code path.  (nnU-Net's per-case .pkl of geometry
    properties is not written: training does not read it.)"""
    npz, img, lbl = entry
    if not npz.is_file():
        if img is None or not Path(lbl).is_file():
            raise FileNotFoundError(f"case {name}: neither {npz} nor a raw image + label pair")
        from ..tta.preprocessing import run_case
        data, seg, _ = run_case([img], lbl, plans, configuration, device)
        npz.parent.mkdir(parents=True, exist_ok=True)
        np.savez_compressed(npz, data=data.astype(np.float32), seg=seg)
    with np.load(npz) as z:
        data, seg = z["data"], z["seg"]
    if data.shape[0] != 1:
        raise NotImplementedError(f"case {name}: {data.shape[0]} image channels; the DG trainers' hooks and the stock "
                                  f"nnUNetTrainer as built here take one")
    return _Case(name, data, seg, regions)


def build_network(plans, dataset_json, configuration, trainer_name, act_dtype=torch.float32, seed=7):
    """The network `train_fold` starts from: topology from the plans, the trainer's input channels, nnU-Net's He
    initialisation drawn from `seed`, deep supervision on.  No hooks registered."""
    in_ch, _ = trainer_spec(trainer_name)
    cfg, patch = unet_cfg_from_plans(plans, dataset_json, configuration, in_ch)
    net = he_init_(HipPlainConvUNet(cfg, act_dtype=act_dtype, deep_supervision=True), seed=seed)
    return net, patch


def _plan_batch(cases, batch_size, patch, spatial, rng):
    """The draws of one augmented batch, in stream order: the case picks, then per item its centre (draw_center for a
    forced-foreground item, else - or when the case has no foreground - a uniformly drawn voxel) and its spatial draw.
    Returns [(case, centre, A or None)]."""
    picks = [cases[int(i)] for i in rng.choice(len(cases), batch_size)]
    plan = []
    for j, case in enumerate(picks):
        center = draw_center(case.locations, rng) if is_forced_foreground(j, batch_size) else None
        if center is None:
            center = tuple(int(rng.randint(n)) for n in case.tensor.shape[-3:])
        plan.append((case, center, spatial.draw(patch, rng)))
    return plan


def _sample_spatial(cases, batch_size, patch, device, spatial):
    """Items whose draw is None are the integer crop of get_batch(..., centers=); all others of the batch leave ONE
    ops.sample_patches_aug launch (16 items per launch, should a batch be larger)."""
    plan = _plan_batch(cases, batch_size, patch, spatial, numpy_rng())
    imgs, labels, aug = [None] * batch_size, [None] * batch_size, []
    for j, (case, center, a) in enumerate(plan):
        if a is None:
            im, lb = get_batch([case.tensor], [0], patch, None, device, centers=[center])
            imgs[j], labels[j] = im[0][0], lb[0]
        else:
            aug.append(j)
    for k in range(0, len(aug), MAX_AUG_ITEMS):
        chunk = aug[k:k + MAX_AUG_ITEMS]
        coefs, labs, maps = [], [], []
        for j in chunk:
            case, center, a = plan[j]
            coefs.append(resident_spline(case.tensor, device))
            labs.append(_resident(case.tensor, device)[2])
            maps.append(sampling_map(a, patch_start(center, case.tensor.shape[-3:], patch), patch))
        im, lb = ops.sample_patches_aug(coefs, labs, maps, patch, order=3)
        for i, j in enumerate(chunk):
            imgs[j], labels[j] = im[i], lb[i][None, None]
    return imgs, labels, [p[0] for p in plan]


def _sample(cases, batch_size, patch, device, multires, spatial=None, *, intensity=None):
    """One batch.  intensity: an IntensityAugmentation whose chain runs on the stacked images after the sampling; the
    *_MultiRes transform then runs inside it (stage 5) instead of after the sampling."""
    with torch.no_grad():
        if spatial is not None:
            imgs, labels, picks = _sample_spatial(cases, batch_size, patch, device, spatial)
        else:
            rng = numpy_rng()
            picks = [cases[int(i)] for i in rng.choice(len(cases), batch_size)]
            imgs, labels = [], []
            for j, case in enumerate(picks):
                center = draw_center(case.locations, rng) if is_forced_foreground(j, batch_size) else None
                im, lb = get_batch([case.tensor], [0], patch, None, device, centers=[center])
                imgs.append(im[0][0])                          # [1, D, H, W]
                labels.append(lb[0])
        if intensity is not None:
            plan = intensity.draw(batch_size, patch, discrete_lowres=multires)
            return intensity.apply(torch.stack(imgs), plan), torch.cat(labels, dim=0)[:, 0], picks
        if multires is not None:
            multires(data=imgs)
    return torch.stack(imgs), torch.cat(labels, dim=0)[:, 0], picks


def draw_mirror_masks(batch_size, axes, rng):
    """nnU-Net's MirrorTransform draws for one training batch: for every item and every allowed axis, independently, a flip with
    probability 0.5.  Draws (numpy_rng(), in this order): item-major, axis 0 first, one rng.uniform() per (item, axis) of `axes`,
    flipped when the draw is < 0.5 - len(axes) * batch_size draws, and NONE when axes is None (a DG trainer's stream does not
    move).  Returns one mask per item: bit a set = axis a flipped (ops.mirror_batch)."""
    if axes is None:
        return [0] * batch_size
    return [sum(1 << a for a in axes if rng.uniform() < 0.5) for _ in range(batch_size)]


def _mirror(imgs, target, axes):
    """The last transform of the training chain (after the intensity stages): one ops.mirror_batch launch for the batch; nothing
    is drawn or launched for a trainer without mirror axes.  The deep-supervision targets are read from the full-resolution
    label map inside ops.deep_supervision_loss, so flipping that map is enough."""
    if axes is None:
        return imgs, target
    masks = draw_mirror_masks(imgs.shape[0], axes, numpy_rng())
    if not any(masks):
        return imgs, target
    with torch.no_grad():
        return ops.mirror_batch(imgs, target, masks)


# ------------------------------------------------------------------------------------------------ the loop
def train_fold(dataset, configuration, fold, trainer_name, num_epochs=1000, iterations_per_epoch=250, val_iterations=50,
               device="cuda", act_dtype=torch.float32, continue_training=False, seed=None, augmentation="reduced", dice="sample",
               final_validation=False):
    """Trains one fold and writes the model folder (module docstring).  dataset: numeric id or folder name; fold: 0..4 or
    "all".  augmentation: "reduced" (module docstring), "spatial" (adds nnU-Net's rotation / scaling to the training
    batches, pretraining/spatial.py; validation batches are never augmented), "full" (the rotation / scaling plus nnU-Net's
    intensity chain, pretraining/intensity.py), or the objects to draw from: a SpatialAugmentation, an IntensityAugmentation
    or a (SpatialAugmentation, IntensityAugmentation) pair.  dice: "sample" or "plans" (module docstring, THE DICE TERM).
    final_validation: validate_fold runs once checkpoint_final.pth is written.  Returns the path of checkpoint_final.pth."""
    if dice not in DICE_MODES:
        raise ValueError(f"dice {dice!r}: one of {', '.join(DICE_MODES)} expected")
    spatial = intensity = None
    if isinstance(augmentation, SpatialAugmentation):
        spatial = augmentation
    elif isinstance(augmentation, IntensityAugmentation):
        intensity = augmentation
    elif isinstance(augmentation, (tuple, list)) and len(augmentation) == 2 and isinstance(augmentation[0], SpatialAugmentation) \
            and isinstance(augmentation[1], IntensityAugmentation):
        spatial, intensity = augmentation
    elif isinstance(augmentation, str) and augmentation in AUGMENTATIONS:
        if augmentation != "reduced":
            spatial = SpatialAugmentation()
        if augmentation == "full":
            intensity = IntensityAugmentation()
    else:
        raise ValueError(f"augmentation {augmentation!r}: one of {', '.join(AUGMENTATIONS)} expected")
    if trainer_name not in TRAINERS:
        raise ValueError(f"trainer {trainer_name}: one of {', '.join(TRAINERS)} expected")
    mirror_axes = trainer_mirror_axes(trainer_name)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("dg_tta_amd trains on the MI355X only (no CPU fallback)")
    f = _resolve_fold(dataset, configuration, fold, trainer_name)
    plans, dataset_json, out_dir, fold_dir = f.plans, f.dataset_json, f.out_dir, f.fold_dir
    batch_dice = dice == "plans" and plans_batch_dice(plans, configuration)
    if dice == "sample" and plans_batch_dice(plans, configuration):
        print(BATCH_DICE_NOTE)
    fold_dir.mkdir(parents=True, exist_ok=True)
    with open(out_dir / "plans.json", "w") as fh:
        json.dump(plans, fh, indent=4)
    with open(out_dir / "dataset.json", "w") as fh:
        json.dump(dataset_json, fh, indent=4)
    final = _train(f, trainer_name, configuration, num_epochs, iterations_per_epoch, val_iterations, device, act_dtype,
                   continue_training, seed, spatial, intensity, mirror_axes, batch_dice)
    if final_validation:
        validate_fold(dataset, configuration, f.fold, trainer_name, device=device, act_dtype=act_dtype)
    return final


def validate_fold(dataset, configuration, fold, trainer_name, device="cuda", act_dtype=torch.float32):
    """The final validation of a trained fold (module docstring, THE FINAL VALIDATION): predicts every validation case with
    fold_<k>/checkpoint_final.pth and writes fold_<k>/validation/<case>.npy and summary.json.  Returns the summary dict."""
    from ..tta.evaluation import case_metrics, summarize_cases
    from ..tta.inference import run_inference
    from ..tta.nnunet_utils import load_network
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("dg_tta_amd validates on the MI355X only (no CPU fallback)")
    f = _resolve_fold(dataset, configuration, fold, trainer_name)
    final = f.fold_dir / "checkpoint_final.pth"
    if not final.is_file():
        raise FileNotFoundError(f"{final} not found: the final validation needs a fold that was trained to the end")
    predictor, patch, network, parameters = load_network(final, device, act_dtype=act_dtype)
    network = network.to(device)
    disable_internal_augmentation()                         # load_network switched it on, as tta_main finds it
    lm = label_model(predictor.dataset_json)
    order = lm.regions_class_order                          # None: a label-based model, argmax over its classes
    if order is not None:
        from ..tta.evaluation import region_key
        labels, top = [region_key(r) for r in lm.foreground_regions], max(order)
    else:
        labels = list(range(network.cfg["num_classes"]))
        top = network.cfg["num_classes"] - 1
    dtype = next(t for t in (np.uint8, np.uint16, np.uint32) if top <= np.iinfo(t).max)
    out = f.fold_dir / "validation"
    out.mkdir(parents=True, exist_ok=True)
    per_case = []
    for name in f.val_names:                                # one at a time: a case's volume and accumulator are gone before the next
        npz = f.entries[name][0]                            # (written by the training, which loads every validation case)
        with np.load(npz) as z:
            data, seg = z["data"], z["seg"][0]
        pred = run_inference(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)), network, parameters, patch,
                             mirror_axes=predictor.allowed_mirroring_axes, regions_class_order=order).numpy().astype(dtype)
        np.save(out / f"{name}.npy", pred)
        per_case.append({"metrics": case_metrics(pred, np.where(seg < 0, 0, seg), labels, device,
                                                 regions=lm.foreground_regions if order is not None else None),
                         "prediction_file": str(out / f"{name}.npy"), "reference_file": str(npz)})
        print(f"pretrain: validated {name}")
    return summarize_cases(per_case, labels, out / "summary.json")


def _resolve_fold(dataset, configuration, fold, trainer_name):
    """What a fold is made of: plans, dataset.json, the resolved configuration, the cases on disk, the split (written when the
    dataset has none) and the folders of the model."""
    fold = "all" if str(fold) == "all" else int(fold)
    dataset_name = maybe_convert_to_dataset_name(dataset)
    plans, dataset_json, pre, raw = load_dataset_files(dataset_name)
    conf = _configuration(plans, configuration)
    data_dir = pre / conf.get("data_identifier", f"{plans.get('plans_name', 'nnUNetPlans')}_{configuration}")
    entries = find_cases(data_dir, raw, dataset_json.get("file_ending", ".nii.gz"))
    if not entries:
        raise FileNotFoundError(f"no training case: neither *.npz in {data_dir} nor images in {raw}/imagesTr")
    splits_file = pre / "splits_final.json"
    if fold == "all":
        train_names = val_names = sorted(entries)
    else:
        if splits_file.is_file():
            with open(splits_file) as f:
                splits = json.load(f)
        else:
            splits = make_splits(sorted(entries))
            with open(splits_file, "w") as f:
                json.dump(splits, f, indent=4)
        if not 0 <= fold < len(splits):
            raise ValueError(f"fold {fold}: {splits_file} has {len(splits)} folds")
        train_names, val_names = splits[fold]["train"], splits[fold]["val"]
        if not val_names:
            print(f"pretrain: fold {fold} has no validation case ({len(entries)} cases): validating on the training cases")
            val_names = train_names
    missing = sorted((set(train_names) | set(val_names)) - set(entries))
    if missing:
        raise FileNotFoundError(f"{splits_file} names cases that are not in the dataset: {missing[:6]}")

    out_dir = Path(nnunet_path("nnUNet_results")) / dataset_name / f"{trainer_name}__nnUNetPlans__{configuration}"
    return SimpleNamespace(fold=fold, plans=plans, dataset_json=dataset_json, conf=conf, entries=entries, train_names=train_names,
                           val_names=val_names, out_dir=out_dir, fold_dir=out_dir / fold_folder_name(fold))


def _train(f, trainer_name, configuration, num_epochs, iterations_per_epoch, val_iterations, device, act_dtype, continue_training,
           seed, spatial, intensity, mirror_axes, batch_dice):
    """The training loop of train_fold on a resolved fold."""
    fold, plans, dataset_json, conf, entries = f.fold, f.plans, f.dataset_json, f.conf, f.entries
    train_names, val_names, fold_dir = f.train_names, f.val_names, f.fold_dir
    if seed is not None:
        torch.manual_seed(seed)
        torch.cuda.manual_seed(seed)
        np.random.seed(seed)
    net, patch = build_network(plans, dataset_json, configuration, trainer_name, act_dtype,
                               seed=seed if seed is not None else int(np.random.randint(2 ** 31 - 1)))
    batch_size = int(conf["batch_size"])
    num_classes = net.cfg["num_classes"]                    # (a region-based dataset: its R regions, no background channel)
    lm = label_model(dataset_json)
    table = ops.region_table(lm.table, device) if lm.has_regions else None

    def loss_of(outs, target):
        if table is not None:
            return ops.deep_supervision_region_loss(outs, target, table, batch_dice=batch_dice)
        return ops.deep_supervision_loss(outs, target, batch_dice=batch_dice)
    net = net.to(device)
    for p in net.parameters():
        p.requires_grad_(True)
    opt = HipSGD(net.parameters(), lr=INITIAL_LR, grad_scale=net.loss_scale)
    log = dict(train_losses=[], val_losses=[], mean_fg_dice=[], lrs=[], ema_fg_dice=[])
    start_epoch, best = 0, None
    if continue_training:
        src = next((p for p in (fold_dir / "checkpoint_latest.pth", fold_dir / "checkpoint_final.pth") if p.is_file()), None)
        if src is None:
            raise FileNotFoundError(f"continue_training: no checkpoint_latest.pth / checkpoint_final.pth in {fold_dir}")
        ck = torch.load(src, map_location="cpu", weights_only=False)
        net.load_state_dict(ck["network_weights"])
        opt.load_state_dict(ck["optimizer_state"])
        opt.grad_scale = float((ck.get("grad_scaler_state") or {}).get("scale", opt.grad_scale))
        start_epoch, log = int(ck["current_epoch"]), {k: list(ck["logging"][k]) for k in log if k in ck["logging"]}
        if "ema_fg_dice" in log:
            best = best_of(log["ema_fg_dice"])
        else:                                               # a checkpoint from before the best-checkpoint rule
            log["ema_fg_dice"], best = rebuild_ema(log["mean_fg_dice"])
        print(f"pretrain: continuing from {src} at epoch {start_epoch} (random streams are not restored)")
    sched = PolyLRScheduler(opt, INITIAL_LR, num_epochs)
    multires = None
    if trainer_name.endswith("_MultiRes"):
        multires = SimulateDiscreteLowResolutionTransform(zoom_range=(1 / 6, 1 / 4, 1 / 2), zoom_axes_invidually=True,
                                                          per_channel=False, p_per_channel=1.0, order_downsample=0,
                                                          order_upsample=3, p_per_sample=0.5, ignore_axes=None)

    loaded = {}

    def cases_of(names):
        for n in names:
            if n not in loaded:
                loaded[n] = load_case(n, entries[n], plans, configuration, device, lm.foreground_regions)
        return [loaded[n] for n in names]

    train_cases, val_cases = cases_of(train_names), cases_of(val_names)

    def save(name, epoch):
        extra = {} if lm.regions_class_order is None else {"regions_class_order": list(lm.regions_class_order)}
        torch.save({**extra, "network_weights": {k: v.detach().cpu() for k, v in net.state_dict().items()},
                    "optimizer_state": opt.state_dict(), "current_epoch": epoch, "trainer_name": trainer_name,
                    "init_args": dict(plans=plans, configuration=configuration, fold=fold, dataset_json=dataset_json),
                    "inference_allowed_mirroring_axes": None if mirror_axes is None else list(mirror_axes), "logging": log,
                    "grad_scaler_state": {"scale": opt.grad_scale}}, fold_dir / name)

    handles = register_dg_hooks(net, trainer_name)          # switches the internal augmentation on, as the trainers do
    recent = {}                                             # case name -> last epoch it was sampled in
    try:
        with open(fold_dir / "training_log.txt", "a") as logf:
            for epoch in range(start_epoch, num_epochs):
                t0 = time.time()
                lr = sched.step(epoch)
                net.train()
                tr_losses = []
                for _ in range(iterations_per_epoch):
                    if opt.resolve_overflow():             # (reads a flag only on the guarded fp16 path)
                        print(f"pretrain: gradient overflow, step skipped, loss scale -> {opt.grad_scale:g}")
                    imgs, target, picks = _sample(train_cases, batch_size, patch, device, multires, spatial, intensity=intensity)
                    imgs, target = _mirror(imgs, target, mirror_axes)
                    loss, _ = loss_of(net(imgs), target)
                    torch.autograd.backward(loss, grad_tensors=torch.full((), float(opt.grad_scale), dtype=torch.float32,
                                                                          device=device))
                    opt.step()
                    opt.zero_grad(set_to_none=True)
                    tr_losses.append(loss.detach())
                    recent.update((c.name, epoch) for c in picks)
                net.eval()
                va_losses, counts = [], torch.zeros((3, num_classes), dtype=torch.int64, device=device)
                with torch.no_grad():
                    for _ in range(val_iterations):
                        imgs, target, picks = _sample(val_cases, batch_size, patch, device, None)
                        outs = net(imgs)
                        loss, _ = loss_of(outs, target)
                        va_losses.append(loss)
                        counts += ops.region_counts(outs[0], target, table) if table is not None else ops.argmax_dice(outs[0], target)[1]
                        recent.update((c.name, epoch) for c in picks)
                # the one read-back of the epoch: mean losses and the per-class pseudo-Dice 2 TP / (2 TP + FP + FN) summed over
                # the validation batches (counts rows: predicted, reference, both)
                nan = torch.full((1,), float("nan"), dtype=torch.float64, device=device)
                if table is not None:                       # rows TP, FP, FN per region; every region is foreground
                    dice = 2.0 * counts[0].double() / (2 * counts[0] + counts[1] + counts[2]).double()
                else:
                    dice = 2.0 * counts[2, 1:].double() / (counts[0, 1:] + counts[1, 1:]).double()
                host = torch.cat([torch.stack(tr_losses).double().mean()[None] if tr_losses else nan,
                                  torch.stack(va_losses).double().mean()[None] if va_losses else nan, dice]).cpu()
                fg = host[2:][~torch.isnan(host[2:])]
                mean_dice = float(fg.mean()) if fg.numel() else float("nan")
                log["train_losses"].append(float(host[0]))
                log["val_losses"].append(float(host[1]))
                log["mean_fg_dice"].append(mean_dice)
                log["lrs"].append(lr)
                prev = log["ema_fg_dice"][-1] if log["ema_fg_dice"] else None
                ema = ema_step(prev, mean_dice)
                log["ema_fg_dice"].append(float("nan") if ema is None else ema)
                logf.write(f"epoch {epoch} lr {lr:.6g} train_loss {float(host[0]):.4f} val_loss {float(host[1]):.4f} "
                           f"pseudo_dice {mean_dice:.4f} loss_scale {opt.grad_scale:g} skipped_steps {opt.skipped_steps} "
                           f"time {time.time() - t0:.1f}s\n")
                logf.flush()
                if len(recent) > RESIDENT_CASES:            # the stream is drained here: trim the volume cache
                    old = sorted(recent, key=recent.get)[:len(recent) - RESIDENT_CASES]
                    release_resident([loaded[n].tensor for n in old])
                    for n in old:
                        del recent[n]
                if (epoch + 1) % SAVE_EVERY == 0 and epoch + 1 < num_epochs:
                    save("checkpoint_latest.pth", epoch + 1)
                if is_new_best(ema, best):
                    best = ema
                    save("checkpoint_best.pth", epoch + 1)
        opt.resolve_overflow()
        save("checkpoint_latest.pth", max(num_epochs, start_epoch))
        save("checkpoint_final.pth", max(num_epochs, start_epoch))
    finally:
        for h in handles:
            h.remove()
        disable_internal_augmentation()
        release_resident([c.tensor for c in loaded.values()])
    return fold_dir / "checkpoint_final.pth"
