"""The label model of a dataset.json - the one place that reads `dataset_json["labels"]` to decide what the network's outputs mean.

nnU-Net knows two label models (restated here from memory of nnunetv2 2.2.1's LabelManager, UNPINNED):

* LABELS: `labels` maps every name to one integer; the classes are mutually exclusive, the network has len(labels) softmax
  channels (background included), the loss is DC+CE (csrc/dice_ce.hip) and the label map is an argmax.  This is what every
  function here answers for a dataset without regions - exactly what the code computed before this module existed.
* REGIONS: some label value is a list with more than one entry, e.g. KiTS
      {"background": 0, "kidney_and_masses": [1, 2, 3], "masses": [2, 3], "tumor": 2}, "regions_class_order": [1, 3, 2].
  Every entry other than background is a REGION - a set of label values that may overlap with the others; an int k is the
  region (k,).  The network has R = number of regions sigmoid outputs and NO background channel, the loss is DC+BCE
  (csrc/region_loss.hip), and the label map is written region by region in the file's order: seg = 0, then
  seg[output_i > 0.5] = regions_class_order[i] - the last region in the order wins (csrc/region_map.hip).

The kernels never see a region target tensor: they read the integer label map and the MEMBERSHIP TABLE, uint32 [L] with
L = largest label value + 1: bit r of table[y] is set when label y belongs to region r.  Hence R <= 32 and L <= 1024.

Left out: the `ignore` label (NotImplementedError for a region dataset), R > 32, test-time adaptation of region models
(refuse_region_tta: the consistency loss is a masked softmax over mutually exclusive channels)."""
from types import SimpleNamespace

import numpy as np

MAX_REGIONS = 32
MAX_TABLE = 1024
ORDER_KEY = "regions_class_order"


def _is_region_value(v):
    return isinstance(v, (list, tuple)) and len(v) > 1


def has_regions(dataset_json):
    """True when any label value is a list / tuple with more than one entry."""
    return any(_is_region_value(v) for v in dataset_json["labels"].values())


def _as_region(name, v):
    vals = tuple(v) if isinstance(v, (list, tuple)) else (v,)
    if not vals or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 0 for x in vals):
        raise ValueError(f"labels[{name!r}] = {v!r}: a non-negative integer or a list of them expected")
    return tuple(int(x) for x in vals)


def label_model(dataset_json):
    """The label model of a dataset.json (module docstring) as a namespace:
      has_regions, num_outputs (channels of the segmentation head), names (of the outputs' classes / regions, background first
      for a label dataset), and for a region dataset also foreground_regions (tuple of label tuples, file order), region_names,
      regions_class_order (tuple of R positive ints), table (uint32 [L], membership_table).
    ValueError / NotImplementedError as the module docstring says; a dataset without regions is never refused."""
    labels = dataset_json["labels"]
    if not has_regions(dataset_json):
        return SimpleNamespace(has_regions=False, num_outputs=len(labels), names=list(labels), foreground_regions=None, region_names=None,
                               regions_class_order=None, table=None)
    if "ignore" in labels:
        raise NotImplementedError("labels: an `ignore` label in a region-based dataset is not built (the ignore label stays out)")
    if "background" not in labels or isinstance(labels["background"], (list, tuple)) or labels["background"] != 0:
        raise ValueError(f"labels: `background` must be 0 (got {labels.get('background')!r})")
    names = [n for n in labels if n != "background"]
    regions = tuple(_as_region(n, labels[n]) for n in names)
    R = len(regions)
    if R > MAX_REGIONS:
        raise ValueError(f"labels: {R} regions; at most {MAX_REGIONS} are built (one bit of the membership table each)")
    order = dataset_json.get(ORDER_KEY)
    if not isinstance(order, (list, tuple)) or len(order) != R or \
            any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x <= 0 for x in order):
        raise ValueError(f"{ORDER_KEY}: a region-based dataset needs `{ORDER_KEY}` with one positive integer per foreground "
                         f"region ({R}: {', '.join(names)}), got {order!r}")
    order = tuple(int(x) for x in order)
    return SimpleNamespace(has_regions=True, num_outputs=R, names=names, foreground_regions=regions, region_names=names,
                           regions_class_order=order, table=membership_table(regions, order))


def num_network_outputs(dataset_json):
    """Channels of the segmentation head: R for a region dataset, len(labels) otherwise."""
    return label_model(dataset_json).num_outputs


def membership_table(regions, also=()):
    """uint32 [L], L = largest label value (of the regions and of `also`: the values a predicted map can hold) + 1: bit r of
    entry y is set when label y belongs to regions[r]."""
    regions = [tuple(int(x) for x in r) for r in regions]
    if len(regions) > MAX_REGIONS:
        raise ValueError(f"{len(regions)} regions; at most {MAX_REGIONS} are built")
    L = max([x for r in regions for x in r] + [int(x) for x in also] + [0]) + 1
    if L > MAX_TABLE:
        raise ValueError(f"largest label value {L - 1}: the membership table holds values below {MAX_TABLE}")
    table = np.zeros(L, dtype=np.uint32)
    for r, members in enumerate(regions):
        for y in members:
            table[y] |= np.uint32(1) << np.uint32(r)
    return table


REGION_TTA_REFUSAL = (
    "test-time adaptation of a region-based model is not built: the consistency loss of DG-TTA is a masked softmax over mutually "
    "exclusive channels, the heads of a region model are independent sigmoids of overlapping regions, and the reference has no "
    "region path either.  `dgtta pretrain` and its validation handle region datasets; prepare_tta / run_tta do not.")


def refuse_region_tta(dataset_json, what):
    """NotImplementedError (REGION_TTA_REFUSAL) when dataset_json describes regions.  `what` names the caller and the model."""
    if dataset_json is not None and isinstance(dataset_json.get("labels"), dict) and has_regions(dataset_json):
        raise NotImplementedError(f"{what}: {REGION_TTA_REFUSAL}")


def refuse_region_tta_of_weights(weights_file, what):
    """refuse_region_tta for the dataset.json beside a checkpoint (<model folder>/fold_k/checkpoint_final.pth); a missing or
    unreadable file decides nothing - the loader reports that."""
    import json
    from pathlib import Path
    try:
        with open(Path(weights_file).parents[1] / "dataset.json") as f:
            dataset_json = json.load(f)
    except (OSError, ValueError, IndexError):
        return
    refuse_region_tta(dataset_json, what)
