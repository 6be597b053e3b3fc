"""`dgtta predict`: plain inference with a trained model folder - the counterpart of `nnUNetv2_predict` (nnunetv2 2.2.1
nnUNetPredictor.predict_from_files, restated from memory: UNPINNED).  A folder of new images goes through the engine's own
preprocessing (tta/preprocessing.run_case), the sliding-window ensemble over the folds' checkpoints (tta/inference.predict_ensemble,
mirroring as the checkpoint allows it) and the export to the case's original geometry (export_segmentation /
export_probabilities / export_region_probabilities); the label map is written with the case's own header.

Label models write the argmax over the model's classes, region models (dg_tta_amd/labels.py) the region label map with
`regions_class_order`'s labels.  There is no label mapping and no post-processing here (tta/postprocessing.py is there to be
called).  Limits: one image channel, one process on one GPU, at most 32 classes for the probabilities of a label model."""
import json
import shutil
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

from .labels import label_model
from .tta import image_io
from .tta.nnunet_utils import _CASE_RE

DEFAULT_FOLDS = (0, 1, 2, 3, 4)
DEFAULT_CHECKPOINT = "checkpoint_final.pth"
ARRAY_EXTENSIONS = (".npy", ".npz")
MAX_PROBABILITY_CLASSES = 32      # export_probabilities' stash: 1..32 selected classes


def _extension(path):
    ext = image_io.extension_of(path)
    if ext is not None:
        return ext
    name = Path(path).name.lower()
    return next((e for e in ARRAY_EXTENSIONS if name.endswith(e)), None)


def list_cases(input_folder):
    """[(case id, file)] of a folder of images, sorted by file name: every file image_io.is_image_file accepts or that ends in
    .npy / .npz; the case id is the name without extension and without a trailing `_0000`.  A case with any channel file other than
    `_0000` is a NotImplementedError (one image channel, as everywhere).  Host only."""
    input_folder = Path(input_folder)
    if not input_folder.is_dir():
        raise FileNotFoundError(f"{input_folder} is not a folder")
    cases, seen = [], {}
    for f in sorted(p for p in input_folder.iterdir() if p.is_file() and _extension(p) is not None):
        stem = f.name[: -len(_extension(f))]
        m = _CASE_RE.match(stem)
        if m and not stem.endswith("_0000"):
            raise NotImplementedError(f"{f}: a case with more than one channel file - several image channels are not built "
                                      f"(one image channel, `<case>_0000`)")
        case = m.group(1) if m else stem
        if case in seen:
            raise ValueError(f"{f} and {seen[case]} are the same case {case!r}")
        seen[case] = f
        cases.append((case, f))
    return cases


def _refuse_array_channels(path):
    """An array case is [X, Y, Z] or [1, X, Y, Z]: more channels are the NotImplementedError list_cases raises for channel files."""
    if image_io.is_image_file(path):
        return
    if str(path).lower().endswith(".npy"):
        shape = np.load(path, mmap_mode="r").shape
    else:
        with np.load(path) as z:
            shape = z["data"].shape
    if len(shape) not in (3, 4) or (len(shape) == 4 and shape[0] != 1):
        raise NotImplementedError(f"{path}: an array of shape {tuple(shape)} - several image channels are not built (one image "
                                  f"channel: [X, Y, Z] or [1, X, Y, Z])")


def model_folder_of(dataset, configuration, trainer="nnUNetTrainer", plans="nnUNetPlans"):
    """nnUNet_results/<Dataset>/<trainer>__<plans>__<configuration>."""
    from .tta.config_log_utils import maybe_convert_to_dataset_name, nnunet_path
    return Path(nnunet_path("nnUNet_results")) / maybe_convert_to_dataset_name(dataset) / f"{trainer}__{plans}__{configuration}"


def _fold_key(fold):
    return "all" if str(fold) == "all" else int(fold)


def checkpoint_files(model_folder, folds=DEFAULT_FOLDS, checkpoint_name=DEFAULT_CHECKPOINT):
    """fold_<k>/<checkpoint_name> of every fold; a missing one is a FileNotFoundError naming the file."""
    files = [Path(model_folder) / f"fold_{_fold_key(k)}" / checkpoint_name for k in folds]
    if not files:
        raise ValueError("predict: no fold given")
    for f in files:
        if not f.is_file():
            raise FileNotFoundError(f"{f} not found: every fold asked for (-f) needs its {checkpoint_name}")
    return files


def _load_members(files, device, act_dtype):
    """The first fold's network and predictor, one state dict per fold."""
    from .tta.nnunet_utils import load_network
    from .utils import disable_internal_augmentation
    predictor = network = patch = None
    members, axes = [], []
    for f in files:
        p, ps, net, params = load_network(f, device, act_dtype=act_dtype)
        disable_internal_augmentation()      # load_network switched it on, as tta_main finds it
        if network is None:
            predictor, patch, network = p, ps, net
        members.append(params[0])
        axes.append(p.allowed_mirroring_axes)
    if any(a != axes[0] for a in axes):
        raise ValueError(f"predict: the folds disagree on inference_allowed_mirroring_axes: "
                         f"{dict(zip([str(f) for f in files], axes))}")
    return predictor, patch, network.to(device), members


def _label_dtype(top):
    return next(t for t in (np.uint8, np.uint16, np.uint32) if top <= np.iinfo(t).max)


@torch.no_grad()
def predict_from_model_folder(model_folder, input_folder, output_folder, folds=DEFAULT_FOLDS, checkpoint_name=DEFAULT_CHECKPOINT,
                              device="cuda", act_dtype=torch.float32, use_mirroring=True, save_probabilities=False,
                              continue_prediction=False):
    """Predicts every case of input_folder with the ensemble of the folds' checkpoints and writes <output>/<case><ext> (the label
    map, with the case's own header, in the smallest unsigned integer type that holds the labels; `<case>.npy` in the preprocessed
    geometry for an array case) and, with save_probabilities, <output>/<case>.npz (`probabilities` float16 in the array geometry of
    the label file: [C, ...] with `class_names` for a label model, [R, ...] with `region_names` and `regions_class_order` for a
    region model).  continue_prediction skips a case whose files exist.  Returns the list of written label files."""
    from .tta.inference import (export_probabilities, export_region_probabilities, export_segmentation, predict_ensemble)
    from .tta.nnunet_utils import preprocess_fromfile
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("dg_tta_amd predicts on the MI355X only (no CPU fallback)")
    model_folder, output_folder = Path(model_folder), Path(output_folder)
    files = checkpoint_files(model_folder, folds, checkpoint_name)
    cases = list_cases(input_folder)
    for _, f in cases:
        _refuse_array_channels(f)
    with open(model_folder / "dataset.json") as f:
        lm = label_model(json.load(f))
    if save_probabilities and not lm.has_regions and lm.num_outputs > MAX_PROBABILITY_CLASSES:
        raise ValueError(f"predict: --save_probabilities of a label model takes at most {MAX_PROBABILITY_CLASSES} classes "
                         f"(this one has {lm.num_outputs})")
    predictor, patch, network, members = _load_members(files, device, act_dtype)
    order = lm.regions_class_order
    mirror_axes = predictor.allowed_mirroring_axes if use_mirroring else None
    dtype = _label_dtype(max(order) if order is not None else lm.num_outputs - 1)

    output_folder.mkdir(parents=True, exist_ok=True)
    for name in ("dataset.json", "plans.json"):
        shutil.copyfile(model_folder / name, output_folder / name)
    with open(output_folder / "predict_args.json", "w") as f:
        json.dump({"model_folder": str(model_folder), "input_folder": str(input_folder), "folds": [_fold_key(k) for k in folds],
                   "checkpoint_name": checkpoint_name, "use_mirroring": bool(use_mirroring), "save_probabilities":
                   bool(save_probabilities), "continue_prediction": bool(continue_prediction), "device": str(device),
                   "dtype": str(act_dtype)}, f, indent=4)

    written = []
    for case, image_file in cases:
        ext = _extension(image_file)
        out = output_folder / (case + (ext if image_io.is_image_file(image_file) else ".npy"))
        npz = output_folder / f"{case}.npz"
        if continue_prediction and out.is_file() and (npz.is_file() or not save_probabilities):
            print(f"predict: {case}: exists, skipped")
            continue
        sample = preprocess_fromfile(image_file, None, case, SimpleNamespace(plans=predictor.plans, device=device,
                                                                             configuration=predictor.configuration))
        props = sample["data_properties"]
        header = props.get("nifti_header")
        geometry = (props if header is not None else None, predictor.plans, predictor.configuration)
        acc, nsum, crop = predict_ensemble(sample["data"][:1], network, members, patch, mirror_axes=mirror_axes,
                                           regions=order is not None)
        soft = None
        if save_probabilities and order is not None:
            soft = export_region_probabilities(acc, nsum, crop, *geometry, members=len(members), regions_class_order=order)
        elif save_probabilities:
            soft = export_probabilities(acc, nsum, crop, *geometry, members=len(members), classes=list(range(lm.num_outputs)))
        seg = soft["segmentation"] if soft is not None else export_segmentation(acc, nsum, crop, *geometry,
                                                                                  regions_class_order=order)
        del acc, nsum, sample      # one case in HBM at a time
        seg = np.ascontiguousarray(seg.astype(dtype))
        if out.suffix == ".npy":
            np.save(out, seg)
        else:
            image_io.write_image(out, seg, header=header)
        if soft is not None:
            names = {"region_names": np.asarray(lm.region_names), "regions_class_order": np.asarray(order, dtype=np.int64)} \
                if order is not None else {"class_names": np.asarray(lm.names)}
            np.savez_compressed(npz, probabilities=soft["probabilities"].astype(np.float16), **names)
        written.append(out)
        print(f"predict: wrote {out}")
    return written
