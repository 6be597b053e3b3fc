"""Connected-component post-processing of a predicted label map on the GPU (csrc/components.hip): label the components of
every organ in one pass, keep the largest one, drop small islands.

The reference has no such step: it hands the folder of predictions to the user's `ModifierFunctions.postprocess_results_fn`
(dg_tta/tta/tta.py:447-470), where nnU-Net users call `remove_all_but_largest_component_from_segmentation`.  The definitions
here are this project's and UNPINNED against any implementation:
  * groups: every entry of `labels_or_regions` is one group, an int (a label) or a tuple of ints (a region: its labels count as
    one object); "foreground" = all non-zero labels as one group; None = every non-zero label present, each on its own.
  * two voxels are connected iff they are neighbours under `connectivity` (6 faces, 18 + edges, 26 + corners) and belong to the
    same group; a component is named cc = 1 + the smallest linear index (d*H + h)*W + w of its voxels.
  * a voxel of a group keeps its label iff its component is the group's largest (ties: the smaller cc) and has at least
    `min_voxels` voxels; otherwise it becomes `background`.  Voxels of no group pass through.
Labels must lie in [0, 1024) to be looked at (the kernels' table size); volumes have fewer than 2^31 - 1 voxels.

Plan keys (all optional, none is written by prepare_tta): `postprocessing_keep_largest_component` (false | true | "foreground" |
a list of indices into / names from `optimized_labels`, a nested list being a region), `postprocessing_min_component_voxels`
(int, default 0), `postprocessing_connectivity` (6 | 18 | 26, default 26).  With one of the first two set, run_tta filters every
prediction before it is written.

Hole filling (fill_label_holes, the same file of kernels run on the complement of an organ) is the other half: a pocket of
background inside an organ becomes the organ.  Plan keys `postprocessing_fill_holes` (false | true | a list as above; "foreground"
names no label to fill with and is refused) and `postprocessing_fill_holes_connectivity` (6 | 18 | 26, default 6 = scipy's
binary_fill_holes); run_tta fills after it has filtered.  UNPINNED as well."""
import numpy as np
import torch

from .. import ops

MAX_LABELS = ops.CC_MAX_TABLE
CONNECTIVITIES = (6, 18, 26)


def _entries(labels_or_regions):
    """[(key, labels)] of a list of ints / tuples of ints; a label in two entries is an error."""
    if isinstance(labels_or_regions, (int, np.integer, tuple)):
        labels_or_regions = [labels_or_regions]
    out, seen = [], {}
    for e in labels_or_regions:
        labels = tuple(int(l) for l in e) if isinstance(e, (tuple, list)) else (int(e),)
        key = labels if isinstance(e, (tuple, list)) else labels[0]
        if not labels:
            raise ValueError("postprocessing: an empty region")
        for l in labels:
            if not 0 <= l < MAX_LABELS:
                raise ValueError(f"postprocessing: label {l} outside [0, {MAX_LABELS})")
            if l in seen:
                raise ValueError(f"postprocessing: label {l} is listed in {seen[l]!r} and in {key!r}; entries of one call must not "
                                 f"share a label - call twice, once per entry")
            seen[l] = key
        out.append((key, labels))
    return out


def _group_table(seg, spec):
    """(int32 table on seg's device, [group key by group id - 1]) of None | "foreground" | a list of entries."""
    if isinstance(spec, str):
        if spec != "foreground":
            raise ValueError(f"postprocessing: unknown group specification {spec!r}")
        table = torch.ones(MAX_LABELS, dtype=torch.int32)
        table[0] = 0
        return table.to(seg.device), ["foreground"]
    if spec is None:        # the labels present: those with a non-empty bounding box
        boxes = ops.label_bboxes(seg, seg, MAX_LABELS).cpu()
        entries = [(l, (l,)) for l in range(1, MAX_LABELS) if boxes[l, 0] <= boxes[l, 3]]
    else:
        entries = _entries(spec)
    # group ids 1 .. len(entries) index the kernels' per-group tables, which are as long as this one
    ntab = max(max([l for _, ls in entries for l in ls], default=0), len(entries)) + 1
    if ntab > MAX_LABELS:
        raise ValueError(f"postprocessing: {len(entries)} groups (at most {MAX_LABELS - 1})")
    table = torch.zeros(ntab, dtype=torch.int32)
    for k, (_, labels) in enumerate(entries):
        table[list(labels)] = k + 1
    return table.to(seg.device), [key for key, _ in entries]


def _to_device(label_map, device):
    """int64 [D,H,W] on the GPU, and the function that gives a result the input's container, dtype and device."""
    device = torch.device(device)
    is_np = isinstance(label_map, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(label_map)) if is_np else label_map
    if t.dim() != 3 or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"postprocessing: integer label map [D,H,W] expected, got {tuple(t.shape)} {t.dtype}")
    seg = t.to(device=device, dtype=torch.int64).contiguous()

    def back(x, dtype=None):
        x = x.to(device=t.device, dtype=t.dtype if dtype is None else dtype)
        return x.numpy() if is_np else x
    return seg, back


def _check_connectivity(connectivity):
    if isinstance(connectivity, bool) or connectivity not in CONNECTIVITIES:
        raise ValueError(f"postprocessing: connectivity {connectivity!r} (6, 18 or 26)")
    return int(connectivity)


def connected_components(label_map, groups=None, connectivity=26, device="cuda"):
    """(cc int32 [D,H,W], size int32 [D*H*W]) of an integer label map (numpy array or tensor; the results come in the same
    container): cc = 0 outside the groups, else 1 + the smallest linear index of the voxel's component; size[r] = voxels of the
    component with cc == r + 1.  `groups` as `labels_or_regions` of keep_largest_components."""
    connectivity = _check_connectivity(connectivity)
    seg, back = _to_device(label_map, device)
    table, _ = _group_table(seg, groups)
    cc = ops.cc_label(seg, table, connectivity)
    return back(cc, torch.int32), back(ops.cc_sizes(cc), torch.int32)


def keep_largest_components(label_map, labels_or_regions=None, connectivity=26, min_voxels=0, background=0, device="cuda",
                            keep_largest=True):
    """(filtered map, {group: removed voxels}).  Per group (module docstring) only the largest component keeps its labels, and only
    if it has at least `min_voxels` voxels; with keep_largest=False only the size threshold applies.  The map is a numpy array or a
    tensor [D,H,W] of an integer dtype; the result has its container, dtype and device.  The dictionary has one entry per group: the
    int, the tuple or "foreground"."""
    connectivity = _check_connectivity(connectivity)
    seg, back = _to_device(label_map, device)
    table, keys = _group_table(seg, labels_or_regions)
    if not keys:
        return back(seg), {}
    ws = torch.empty(ops.cc_ws_bytes(*seg.shape), dtype=torch.uint8, device=seg.device)
    cc = ops.cc_label(seg, table, connectivity, ws=ws)
    out, removed = ops.cc_filter(seg, table, cc, ops.cc_sizes(cc), keep_largest, min_voxels, background, ws=ws)
    removed = removed.cpu().tolist()
    return back(out), {key: removed[k + 1] for k, key in enumerate(keys)}


def remove_all_but_largest_component_from_segmentation(segmentation, labels_or_regions, background_label=0):
    """nnU-Net's post-processing call, by name and argument order, for hooks written against nnU-Net.  Restated from memory of
    nnU-Net's behaviour and UNPINNED: full connectivity (26); every entry (a label or a region tuple) is applied on its own to
    the ORIGINAL segmentation, so entries may share labels - they are then filtered in several passes."""
    if not isinstance(labels_or_regions, list):
        labels_or_regions = [labels_or_regions]
    passes = []             # entries that share no label go through the kernels together
    for e in labels_or_regions:
        labels = set(int(l) for l in e) if isinstance(e, (tuple, list)) else {int(e)}
        for p in passes:
            if not (p[1] & labels):
                p[0].append(e), p[1].update(labels)
                break
        else:
            passes.append(([e], labels))
    is_np = isinstance(segmentation, np.ndarray)
    ret = segmentation.copy() if is_np else segmentation.clone()
    for entries, _ in passes:
        kept, _ = keep_largest_components(segmentation, entries, connectivity=26, background=background_label)
        if len(passes) == 1:
            return kept
        ret[kept != segmentation] = background_label
    return ret


def fill_label_holes(label_map, labels_or_regions=None, connectivity=6, background=0, device="cuda"):
    """(filled map, {group: filled voxels}).  The complement of keep_largest_components: a pocket of `background` inside an organ
    becomes the organ.  This project's definition, UNPINNED against any implementation: the entries (an int, or a tuple of ints
    = a region; None = every non-zero label present, ascending) are processed in the listed order, each on the result of the one
    before.  For an entry with labels L, S = isin(map, L); a voxel outside S is enclosed iff its component of the complement of S
    under `connectivity` (6 = scipy.ndimage.binary_fill_holes, 18, 26) touches no face of the volume; every enclosed voxel whose
    value is `background` becomes the entry's FIRST label, enclosed voxels of another label (a lesion inside the organ) keep it.
    Labels outside [0, 1024) are never members of S.  Containers, dtypes and the dictionary's keys as in keep_largest_components.
    Each entry runs inside the bounding box of L, whose faces stand for the volume's: everything outside the box is complement
    and reaches the border, so the result is the whole volume's."""
    connectivity = _check_connectivity(connectivity)
    if isinstance(labels_or_regions, str):
        raise ValueError(f"postprocessing: {labels_or_regions!r} names no label to fill with; list labels or regions")
    seg, back = _to_device(label_map, device)
    boxes = ops.label_bboxes(seg, seg, MAX_LABELS).cpu().numpy()
    if labels_or_regions is None:
        entries = [(l, (l,)) for l in range(1, MAX_LABELS) if boxes[l, 0] <= boxes[l, 3]]
    else:
        entries = _entries(labels_or_regions)
    # the entries are applied in place: never to the caller's memory (an int64 tensor on the device comes through as it is)
    out = seg.clone() if isinstance(label_map, torch.Tensor) and seg.data_ptr() == label_map.data_ptr() else seg
    ws, counts = None, {}
    for key, labels in entries:
        present = [l for l in labels if boxes[l, 0] <= boxes[l, 3]]
        if not present:         # nothing of L in the map: filling changes no box, so the boxes taken before the loop hold
            counts[key] = 0
            continue
        lo, hi = boxes[present, :3].min(0), boxes[present, 3:].max(0)
        box = (*lo.tolist(), *(hi - lo + 1).tolist())
        table = torch.zeros(max(labels) + 1, dtype=torch.int32)
        table[list(labels)] = 1
        mask = ops.holes_member(out, table.to(out.device), box)
        nbytes = ops.holes_ws_bytes(*mask.shape)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=out.device)
        filled, _ = ops.fill_holes(mask, connectivity, ws=ws)
        counts[key] = ops.holes_apply(out, mask, filled, box, background, labels[0])
    return back(out), {key: int(v) for key, v in counts.items()}


# ---------------------------------------------------------------------------------------------- plan keys (host logic)
def _plan_groups(config, key_name, foreground):
    """The `labels_or_regions` that the plan key `key_name` asks for, in the index space of `optimized_labels` (the label values of
    a written prediction): None for false / absent, every foreground index for true, "foreground" where the key takes it, or the
    listed entries - an index or a name, a nested list of them being a region."""
    key = config.get(key_name, False)
    names = list(config["optimized_labels"])
    if key is None or key is False:
        return None
    if key is True:
        return list(range(1, len(names)))
    if key == "foreground" and foreground:
        return "foreground"
    if not isinstance(key, (list, tuple)):
        takes = "false, true, \"foreground\" or a list" if foreground else "false, true or a list"
        raise ValueError(f"{key_name}: {key!r} ({takes} expected)")

    def index(x):
        if isinstance(x, str):
            if x not in names:
                raise ValueError(f"{key_name}: label name {x!r} is not in optimized_labels {names}")
            return names.index(x)
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= x < len(names):
            raise ValueError(f"{key_name}: label index {x!r} is not in optimized_labels (0 to {len(names) - 1})")
        return int(x)
    groups = [tuple(index(x) for x in e) if isinstance(e, (list, tuple)) else index(e) for e in key]
    _entries(groups)        # duplicates are reported here, not at the first case
    return groups


def postprocessing_groups(config):
    """The `labels_or_regions` of keep_largest_components that the plan key `postprocessing_keep_largest_component` asks for."""
    return _plan_groups(config, "postprocessing_keep_largest_component", foreground=True)


def fill_holes_settings(config):
    """None when the plan asks for no hole filling, else the keyword arguments of fill_label_holes: `postprocessing_fill_holes`
    (false | true | a list as for the keep-largest key; "foreground" names no label to fill with and is refused) and
    `postprocessing_fill_holes_connectivity` (6 | 18 | 26, default 6)."""
    connectivity = _check_connectivity(config.get("postprocessing_fill_holes_connectivity", 6))
    groups = _plan_groups(config, "postprocessing_fill_holes", foreground=False)
    if groups is None:
        return None
    return dict(labels_or_regions=groups, connectivity=connectivity)


def postprocessing_settings(config):
    """None when the plan asks for no post-processing, else the keyword arguments of keep_largest_components."""
    connectivity = _check_connectivity(config.get("postprocessing_connectivity", 26))
    min_voxels = config.get("postprocessing_min_component_voxels", 0)
    if isinstance(min_voxels, bool) or not isinstance(min_voxels, (int, np.integer)) or min_voxels < 0:
        raise ValueError(f"postprocessing_min_component_voxels: {min_voxels!r} (a non-negative int expected)")
    groups = postprocessing_groups(config)
    if groups is None and min_voxels == 0:
        return None
    return dict(labels_or_regions=list(range(1, len(config["optimized_labels"]))) if groups is None else groups,
                connectivity=connectivity, min_voxels=int(min_voxels), keep_largest=groups is not None)
