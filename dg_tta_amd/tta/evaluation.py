"""Folder evaluation of predicted label maps — the step after ensemble inference (dg_tta/tta/tta.py:447-470), which the
reference delegates to nnU-Net's compute_metrics_on_folder_simple [3P nnunetv2==2.2.1, evaluation/evaluate_predictions.py].
Restated from the published algorithm (parity unpinned: nnunetv2 is not vendored with the reference): per case and label
TP / FP / FN / TN, Dice = 2TP/(2TP+FP+FN), IoU = TP/(TP+FP+FN) (NaN when the label is absent from both), n_pred, n_ref;
'mean' = nanmean over cases, 'foreground_mean' = mean over labels != 0.  The per-label counts come from the HIP
label-count kernel (dgtta_argmax_dice), the arithmetic on them is host-side.

Opt-in surface-distance metrics (`surface_metrics`; HD95, HD, ASSD, NSD in millimetres).  The reference computes none of them
(it delegates evaluation to nnU-Net, which reports overlap only): the definitions are the published ones, parity UNPINNED.
M = (map == label); the surface S(M) = voxels of M with at least one of the six face neighbours outside M, everything outside
the volume counting as outside; d_rp = for every voxel of S(ref) the Euclidean distance in physical units (index differences
times the per-axis spacing) to the nearest voxel of S(pred), d_pr the other direction;
  HD95 = numpy.percentile(concat(d_rp, d_pr), 95) (linear interpolation),  HD = max(concat),
  ASSD = (mean(d_rp) + mean(d_pr)) / 2,  NSD(tau) = (#{d_rp <= tau} + #{d_pr <= tau}) / (|S(ref)| + |S(pred)|).
A label absent from both maps gives NaN for all four (the Dice convention above); absent from exactly one: HD95 = HD = ASSD =
inf, NSD = 0.  'mean' stays the nanmean over cases, so one case's inf makes the label's mean inf.  Bounding boxes, surfaces and
the exact distance transform are HIP kernels (csrc/surface.hip); compaction, sqrt, sort and the order statistics touch the
surface voxels only and use torch."""
import json
from pathlib import Path

import numpy as np
import torch

from .. import ops
from .image_io import is_image_file, read_image


def load_label_map(path):
    p = str(path)
    if p.endswith(".npy"):
        return np.load(p)
    if is_image_file(p):
        return read_image(p)[0]
    raise ValueError(f"unsupported label map format: {p}")


def load_label_map_with_header(path):
    """(label map, header) - load_label_map that keeps the image header; None for `.npy`, which has none."""
    p = str(path)
    if p.endswith(".npy"):
        return np.load(p), None
    if is_image_file(p):
        return read_image(p)
    raise ValueError(f"unsupported label map format: {p}")


def array_spacing(header):
    """Spacing of the ARRAY axes [z, y, x] of a map read by read_image: header['pixdim'] is (x, y, z), so reversed; (1, 1, 1)
    without a header."""
    if header is None:
        return (1.0, 1.0, 1.0)
    return tuple(float(v) for v in header["pixdim"])[::-1]


SURFACE_KEYS = ["HD95", "HD", "ASSD", "NSD"]


def _to_device_map(a, device):
    return torch.as_tensor(np.ascontiguousarray(a).astype(np.int64)).to(device)


def surface_metrics(pred, ref, labels, spacing=(1.0, 1.0, 1.0), nsd_tolerance_mm=1.0, device="cuda"):
    """metrics[label] = {HD95, HD, ASSD, NSD} (module docstring) for two integer label maps [D,H,W] of equal shape; `spacing` =
    millimetres per voxel along the array axes.  Per label: the crop box of the label's voxels in either map (both surfaces lie
    inside it, so no nearest surface voxel is cut off), the two surfaces, two distance transforms, the distances at the other
    map's surface voxels.  Workspace and buffers are sized for the largest box and shared by the labels."""
    if tuple(pred.shape) != tuple(ref.shape) or len(pred.shape) != 3:
        raise ValueError(f"two 3-D maps of equal shape expected: prediction {tuple(pred.shape)} vs reference {tuple(ref.shape)}")
    p = pred.to(device).long().contiguous() if torch.is_tensor(pred) else _to_device_map(pred, device)
    r = ref.to(device).long().contiguous() if torch.is_tensor(ref) else _to_device_map(ref, device)
    labels = [int(l) for l in labels]
    boxes = ops.label_bboxes(p, r, max(labels) + 1).cpu().numpy().astype(np.int64)
    crop = {l: (*boxes[l, :3], *(boxes[l, 3:] - boxes[l, :3] + 1)) for l in labels if boxes[l, 0] <= boxes[l, 3]}
    out = {l: dict.fromkeys(SURFACE_KEYS, float("nan")) for l in labels}
    if not crop:
        return out
    nmax = max(int(c[3] * c[4] * c[5]) for c in crop.values())
    surf_p = torch.empty(nmax, dtype=torch.uint8, device=p.device)
    surf_r = torch.empty(nmax, dtype=torch.uint8, device=p.device)
    dist2 = torch.empty(nmax, dtype=torch.float32, device=p.device)
    ws = torch.empty(max(max(ops.edt_ws_bytes(*c[3:]) for c in crop.values()), 256), dtype=torch.uint8, device=p.device)
    tau = float(nsd_tolerance_mm)
    for l, box in crop.items():
        sp, sr = ops.label_surface(p, l, box, out=surf_p).bool(), ops.label_surface(r, l, box, out=surf_r).bool()
        d_rp = ops.edt_sq(surf_p[:sp.numel()].view(sp.shape), spacing, out=dist2, ws=ws)[sr].double().sqrt()
        d_pr = ops.edt_sq(surf_r[:sr.numel()].view(sr.shape), spacing, out=dist2, ws=ws)[sp].double().sqrt()
        n_r, n_p = d_rp.numel(), d_pr.numel()
        if n_r == 0 or n_p == 0:                # in exactly one map (a present label always has a surface)
            out[l] = {"HD95": float("inf"), "HD": float("inf"), "ASSD": float("inf"), "NSD": 0.0}
            continue
        both = torch.sort(torch.cat([d_rp, d_pr])).values
        pos = 0.95 * (n_r + n_p - 1)
        k = int(np.floor(pos))
        k1 = min(k + 1, n_r + n_p - 1)
        a, b, hd, m_rp, m_pr, close = torch.stack([both[k], both[k1], both[-1], d_rp.mean(), d_pr.mean(),
                                                   (both <= tau).sum().double()]).tolist()
        out[l] = {"HD95": a + (b - a) * (pos - k), "HD": hd, "ASSD": (m_rp + m_pr) / 2, "NSD": close / (n_r + n_p)}
    return out


def region_key(region):
    """The key of a region in a metrics dict, as nnU-Net writes it: the label itself for a one-label region, else the tuple of its
    labels (JSON: "3", "(2, 3)")."""
    region = (region,) if isinstance(region, (int, np.integer)) else tuple(int(x) for x in region)
    return int(region[0]) if len(region) == 1 else region


def _key(lab):
    return lab if isinstance(lab, tuple) else int(lab)


def region_case_metrics(pred, ref, regions, device="cuda"):
    """case_metrics per REGION instead of per label (region-based datasets, dg_tta_amd/labels.py): metrics[region_key(r)] = {Dice,
    IoU, FP, TP, FN, TN, n_pred, n_ref} of the masks isin(pred, r) and isin(ref, r).  regions: tuples of label values.  The masks
    come from a table lookup, the counts from the label-count kernel on the two binary maps."""
    if tuple(pred.shape) != tuple(ref.shape):
        raise ValueError(f"shape mismatch: prediction {tuple(pred.shape)} vs reference {tuple(ref.shape)}")
    regions = [tuple(int(x) for x in r) for r in regions]
    p = torch.as_tensor(np.ascontiguousarray(pred).astype(np.int64)).to(device).reshape(-1)
    r = torch.as_tensor(np.ascontiguousarray(ref).astype(np.int64)).to(device).reshape(-1)
    top = max([x for reg in regions for x in reg] + [int(p.max()), int(r.max()), 0]) + 1
    if int(p.min()) < 0 or int(r.min()) < 0:
        raise ValueError("region_case_metrics: negative label values")
    total = int(p.numel())
    out = {}
    for reg in regions:
        member = torch.zeros(top, dtype=torch.int64, device=p.device)
        member[list(reg)] = 1
        _, counts = ops.argmax_dice_from_labels(member[p], member[r], 2)        # rows: n_pred, n_ref, TP
        c = counts[:, 1].cpu().tolist()
        n_pred, n_ref, tp = int(c[0]), int(c[1]), int(c[2])
        fp, fn = n_pred - tp, n_ref - tp
        dice, iou = (float("nan"), float("nan")) if tp + fp + fn == 0 else (2 * tp / (2 * tp + fp + fn), tp / (tp + fp + fn))
        out[region_key(reg)] = {"Dice": dice, "IoU": iou, "FP": fp, "TP": tp, "FN": fn, "TN": total - tp - fp - fn, "n_pred": n_pred,
                                "n_ref": n_ref}
    return out


def case_metrics(pred, ref, labels, device="cuda", spacing=None, surface=False, nsd_tolerance_mm=1.0, regions=None):
    """metrics[label] = {Dice, IoU, FP, TP, FN, TN, n_pred, n_ref} for two integer label maps of equal shape; with `surface`
    also {HD95, HD, ASSD, NSD} at `spacing` (millimetres along the array axes; None = unit spacing).
    regions (tuples of label values; `labels` is then not read): the region form, region_case_metrics - overlap metrics only."""
    if regions is not None:
        if surface:
            raise NotImplementedError("case_metrics: surface metrics per region are not built")
        return region_case_metrics(pred, ref, regions, device)
    if tuple(pred.shape) != tuple(ref.shape):
        raise ValueError(f"shape mismatch: prediction {tuple(pred.shape)} vs reference {tuple(ref.shape)}")
    nlab = int(max(labels)) + 1
    p = torch.as_tensor(np.ascontiguousarray(pred).astype(np.int64)).to(device)
    r = torch.as_tensor(np.ascontiguousarray(ref).astype(np.int64)).to(device)
    _, counts = ops.argmax_dice_from_labels(p, r, nlab)        # rows: n_pred, n_ref, TP
    c = counts.cpu().numpy().astype(np.int64)
    total = int(p.numel())
    out = {}
    for lab in labels:
        n_pred, n_ref, tp = int(c[0, lab]), int(c[1, lab]), int(c[2, lab])
        fp, fn = n_pred - tp, n_ref - tp
        tn = total - tp - fp - fn
        if tp + fp + fn == 0:
            dice = iou = float("nan")
        else:
            dice, iou = 2 * tp / (2 * tp + fp + fn), tp / (tp + fp + fn)
        out[int(lab)] = {"Dice": dice, "IoU": iou, "FP": fp, "TP": tp, "FN": fn, "TN": tn, "n_pred": n_pred, "n_ref": n_ref}
    if surface:
        sm = surface_metrics(p, r, labels, (1.0, 1.0, 1.0) if spacing is None else spacing, nsd_tolerance_mm, device)
        for lab in labels:
            out[int(lab)].update(sm[int(lab)])
    return out


def compute_metrics_on_folder_simple(folder_ref, folder_pred, labels, output_file=None, device="cuda",
                                     suffixes=(".nii.gz", ".nii", ".nrrd", ".mha", ".mhd", ".npy"), surface_metrics=False,
                                     nsd_tolerance_mm=1.0):
    """Evaluates every prediction in folder_pred that has a reference of the same name in folder_ref; returns the summary
    dict (and writes it as JSON to output_file) in nnU-Net's layout: metric_per_case / mean / foreground_mean.
    surface_metrics: every label's dict, 'mean' and 'foreground_mean' also carry HD95, HD, ASSD and NSD(nsd_tolerance_mm), in
    the physical units of the REFERENCE file's header (`.npy` maps: unit spacing); 'mean' is the nanmean over cases, so inf
    (a label missing from one of a case's two maps) propagates into it."""
    folder_ref, folder_pred = Path(folder_ref), Path(folder_pred)
    files = sorted(f for f in folder_pred.iterdir() if f.name.endswith(tuple(suffixes)))
    per_case = []
    for f in files:
        ref = folder_ref / f.name
        if not ref.is_file():
            continue
        if surface_metrics:
            ref_map, ref_hdr = load_label_map_with_header(ref)
            m = case_metrics(load_label_map(f), ref_map, labels, device, spacing=array_spacing(ref_hdr), surface=True,
                             nsd_tolerance_mm=nsd_tolerance_mm)
        else:
            m = case_metrics(load_label_map(f), load_label_map(ref), labels, device)
        per_case.append({"metrics": m, "prediction_file": str(f), "reference_file": str(ref)})
    return summarize_cases(per_case, labels, output_file, surface_metrics)


def summarize_cases(per_case, labels, output_file=None, surface_metrics=False):
    """The summary dict of compute_metrics_on_folder_simple from its per-case entries
    [{"metrics": case_metrics(...), "prediction_file", "reference_file"}]; written as JSON to output_file when given.
    The region form: `labels` holds the keys of region_case_metrics (region_key: ints and tuples); every region is foreground."""
    keys = ["Dice", "IoU", "FP", "TP", "FN", "TN", "n_pred", "n_ref"] + (SURFACE_KEYS if surface_metrics else [])
    means = {}
    for lab in labels:
        means[_key(lab)] = {}
        for k in keys:
            vals = np.array([c["metrics"][_key(lab)][k] for c in per_case], dtype=np.float64)
            means[_key(lab)][k] = float(np.nanmean(vals)) if vals.size and not np.all(np.isnan(vals)) else float("nan")
    fg = [l for l in labels if l != 0]
    foreground_mean = {k: float(np.mean([means[_key(l)][k] for l in fg])) if fg else float("nan") for k in keys}
    summary = {"metric_per_case": per_case, "mean": means, "foreground_mean": foreground_mean}
    if output_file is not None:
        Path(output_file).parent.mkdir(parents=True, exist_ok=True)
        with open(output_file, "w") as fh:
            json.dump(_jsonable(summary), fh, indent=4, sort_keys=False)
    return summary


def _jsonable(o):
    if isinstance(o, dict):
        return {str(k): _jsonable(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_jsonable(v) for v in o]
    if isinstance(o, (np.integer,)):
        return int(o)
    if isinstance(o, (np.floating,)):
        return float(o)
    return o
