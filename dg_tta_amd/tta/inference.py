"""Post-TTA ensemble sliding-window inference (SURVEY.md §8f "next" #1) — what the reference does at
dg_tta/tta/tta.py:379-416 through nnU-Net's predictor (dg_tta/tta/nnunet_utils.py:116-125, 208-230):
Gaussian-weighted 50 %-overlap sliding window, logits averaged over the ensemble's TTA'd parameter sets, argmax over
ALL pretrain classes, then map_label(argmaxed) to the target label ids.

Mirroring follows the checkpoint, as nnU-Net's predictor does (use_mirroring=True is its default): the DG trainers set
inference_allowed_mirroring_axes=None (nnUNetTrainer_GIN_MIND.py:34-35) and run exactly the passes they ran before; a stock
nnUNetTrainer checkpoint says (0, 1, 2), and `mirror_axes` then predicts every window under all 2^|A| flips - the window's
prediction is the mean over the subsets S of flip_S(net(flip_S(x))), subsets in the order (), (0), (1), (2), (0,1), (0,2), (1,2),
(0,1,2) (nnunetv2 2.2.1 _internal_maybe_mirror_and_predict, from memory: UNPINNED like the window logic).  Here every mirrored pass
is one more window of a batch (_mirror_work): ops.window_gather builds the flipped inputs in one launch and the mirrored accumulate
kernels add gauss[p] * out[flip_S(p)] at origin + p and gauss[p] into nsum, so acc / nsum is the mean over the mirrors and
everything downstream of the accumulators is untouched.  The Gaussian is NOT flipped: it is centred at i // 2 and at even tile
sizes its flip is a different array.  A fp16 logits accumulator is refused with mirroring (no headroom for eight passes).

The window logic is a restatement of nnunetv2==2.2.1 (`compute_gaussian`, `compute_steps_for_sliding_window`,
`predict_sliding_window_return_logits`) from its published behaviour: that package is not vendored with the reference, so
this stage is "parity unpinned" (checked against the CPU restatement in oracle/inference.py only).  Accumulators live
in HBM for the whole volume (105 classes x 512^3 = 56 GB in fp32 fits the 288 GB of an MI355X); they are fp32 by default
and fp16 - nnU-Net's storage type for `predicted_logits` - with DGTTA_WINDOW_ACC=fp16 or `acc_dtype=torch.float16` (sums
still formed in fp32, rounded once per window: half the read-modify-write traffic).  `export_segmentation` takes the logits back to the case's original geometry.

Round 5 - the FEATURE-space accumulator, what `predict_ensemble` / `run_inference` / `dgtta run_tta` use by default
(DGTTA_WINDOW_ACC=features): the segmentation head is linear and last, so sum_w g_w (W z_w + b) = W (sum_w g_w z_w) + b sum_w g_w;
the volume holds the 32 Gaussian-weighted feature channels the head reads (fp32: 16 GiB per member at 512^3 instead of 52.5 GiB of
logits, 2.8x less read-modify-write traffic per window) and the head runs once per voxel, fused with the argmax over the ensemble
(csrc/window_features.hip).  `predict_sliding_window_return_logits` / `predict_ensemble_logits` keep nnU-Net's logits-space form.
"""
import os

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check, ptr, stream_of
from ..mind import mind_groups
from .torch_utils import map_label


_GAUSS_CACHE = {}


def compute_gaussian(tile_size, sigma_scale=1.0 / 8, value_scaling_factor=10.0):
    """nnU-Net's importance map (cached per tile size: the scipy filter of a 128^3 tile costs ~0.15 s, more than the
    network passes of a small case)."""
    key = (tuple(int(t) for t in tile_size), float(sigma_scale), float(value_scaling_factor))
    if key not in _GAUSS_CACHE:
        _GAUSS_CACHE[key] = _compute_gaussian(key[0], sigma_scale, value_scaling_factor)
    return _GAUSS_CACHE[key].clone()


def _compute_gaussian(tile_size, sigma_scale, value_scaling_factor):
    from scipy.ndimage import gaussian_filter
    tmp = np.zeros(tile_size)
    tmp[tuple(i // 2 for i in tile_size)] = 1
    g = gaussian_filter(tmp, [i * sigma_scale for i in tile_size], 0, mode="constant", cval=0)
    g = torch.from_numpy(g).float()
    g = g / g.max() * value_scaling_factor
    g[g == 0] = g[g != 0].min()
    return g


def compute_steps_for_sliding_window(image_size, tile_size, tile_step_size=0.5):
    assert all(i >= j for i, j in zip(image_size, tile_size)), "image size must be as large or larger than patch_size"
    assert 0 < tile_step_size <= 1
    target = [i * tile_step_size for i in tile_size]
    num_steps = [int(np.ceil((i - k) / j)) + 1 for i, j, k in zip(image_size, target, tile_size)]
    steps = []
    for dim in range(len(tile_size)):
        max_step = image_size[dim] - tile_size[dim]
        actual = max_step / (num_steps[dim] - 1) if num_steps[dim] > 1 else 99999999999
        steps.append([int(np.round(actual * i)) for i in range(num_steps[dim])])
    return steps


def pad_to_patch(data, patch_size):
    """Centred zero padding up to the patch size (nnU-Net pads with constant 0); returns (padded, crop slices)."""
    pads, crop = [], []
    for have, want in zip(data.shape[1:], patch_size):
        extra = max(want - have, 0)
        lo = extra // 2
        pads.append((lo, extra - lo))
        crop.append(slice(lo, lo + have))
    if any(p != (0, 0) for p in pads):
        flat = [v for p in reversed(pads) for v in p]
        data = torch.nn.functional.pad(data, flat, mode="constant", value=0)
    return data, crop


# windows per network pass.  Measured at 512^3: 2 / 4 / 8 / 16 windows per pass = 3.26 / 3.14 / 3.07 / 3.03 ms per window in round 3;
# round 5 (feature-space accumulator): 0.541 s per member with 8, 0.537 with 12, 0.533 with 16 (~25 GB of activations in 16-bit storage)
WINDOW_BATCH = max(1, int(os.environ.get("DGTTA_WINDOW_BATCH", "16")))


def window_acc_mode():
    """DGTTA_WINDOW_ACC = features (default: feature-space accumulator where the network offers it, else fp32 logits) | fp32 | fp16
    (logits-space accumulator of that storage type)."""
    v = os.environ.get("DGTTA_WINDOW_ACC", "features").lower()
    if v not in ("features", "fp32", "fp16"):
        raise ValueError(f"DGTTA_WINDOW_ACC={v!r}: features, fp32 or fp16")
    return v


def window_acc_dtype():
    """Storage type of the LOGITS-space window accumulator: fp16 with DGTTA_WINDOW_ACC=fp16, else fp32."""
    return torch.float16 if window_acc_mode() == "fp16" else torch.float32


def _acc_code(acc):
    if acc.dtype not in (torch.float32, torch.float16):
        raise ValueError("the window accumulator is fp32 or fp16")
    return ops.F32 if acc.dtype == torch.float32 else ops.F16


def _inner(model):
    return getattr(model, "_orig_mod", model)


def _num_classes(model):
    return _inner(model).decoder.seg_layers[-1].out_channels


def _can_fuse_head_accumulate(model):
    """The head may write straight into the window accumulator when the network offers it and nothing stands between the
    head and the accumulation: every forward hook is the plan's untouched model-output modifier (identity)."""
    m = _inner(model)
    if not hasattr(m, "can_fuse_window_accumulate") or not m.can_fuse_window_accumulate():
        return False
    return _only_identity_output_hooks(m)


def _only_identity_output_hooks(m):
    from .config_log_utils import is_template_modifier
    for h in m._forward_hooks.values():
        cells = getattr(h, "__closure__", None) or ()
        fns = [c.cell_contents for c in cells if callable(c.cell_contents)]
        if len(fns) != 1 or not is_template_modifier(fns[0], "modfify_tta_model_output_fn"):
            return False
    return True


FEATURE_HEAD_MAX_CLASSES_MFMA = 128      # dgtta_feature_head_argmax: classes x 32 voxels per wave on the matrix cores
FEATURE_HEAD_MAX_CLASSES_VALU = 160      # its vector-ALU kernel with M > 1 members parks C * 256 * 4 B of partial sums in LDS


def _can_accumulate_features(model, members=1, regions=False):
    """Feature-space accumulation needs the network's offer (head = 1x1x1 conv on 32 channels, nothing selected), nothing
    between the head and the accumulation (every forward hook is the plan's untouched model-output modifier = identity), and a
    head the final head + argmax kernel takes (C <= 128, or one member, or C <= 160) - checked UP FRONT, so that a
    wider ensemble goes to the logits-space accumulator instead of failing after every member's sliding-window pass.
    regions: the label map will be the region one (WindowFeatures.regions): the head must then be one dgtta_feature_head_regions
    takes (R <= 32 outputs, an ensemble whose weight image fits the LDS; R = 1 included)."""
    m = _inner(model)
    if not (hasattr(m, "can_fuse_window_feature_accumulate") and m.can_fuse_window_feature_accumulate() and
            _only_identity_output_hooks(m)):
        return False
    ncls = _num_classes(m)
    if regions:
        return ops.feature_head_regions_supported(members, ncls)
    return ncls <= FEATURE_HEAD_MAX_CLASSES_MFMA or members == 1 or ncls <= FEATURE_HEAD_MAX_CLASSES_VALU


class WindowFeatures:
    """Feature-space window accumulator of an ensemble: facc [M,X,Y,Z,32] (fp32, sum over windows of gauss * head input of member m),
    nsum [X,Y,Z] (sum of the window Gaussians, shared), crop (slices back from the padding), w [M,C,32] / b [M,C] the members' head
    weights.  The ensemble's accumulated logits - what predict_ensemble_logits returns as `acc` - are
    sum_m (w[m] @ facc[m] + b[m] * nsum); they are never formed for the whole volume."""

    def __init__(self, facc, nsum, crop, w, b):
        self.facc, self.nsum, self.crop, self.w, self.b = facc, nsum, crop, w.contiguous(), b.contiguous()
        self.bsum = b.sum(0).contiguous()

    @property
    def shape(self):
        return (*self.facc.shape[1:4], self.w.shape[1])

    def argmax(self):
        """Label map [X,Y,Z] (int64, padded geometry): argmax over all classes of the ensemble logits, first maximum wins."""
        return ops.feature_head_argmax(self.facc, self.nsum, self.w, self.bsum)

    def regions(self, order):
        """Label map [X,Y,Z] (int64, padded geometry) of a REGION head: 0, then order[i] = regions_class_order[i] wherever the
        ensemble logit of output i is > 0, in order - the last positive region wins (ops.feature_head_regions; unpinned)."""
        return ops.feature_head_regions(self.facc, self.nsum, self.w, self.bsum, order)

    def softmax(self, classes, prob_dtype=torch.float32):
        """(label int64, confidence fp32, entropy fp32 [X,Y,Z], probs prob_dtype [K,X,Y,Z]) in the padded geometry: softmax over all
        classes of the ensemble-MEAN logits, probabilities of `classes` only (ops.feature_head_softmax; definitions unpinned).
        `label` holds the integers argmax() returns."""
        return ops.feature_head_softmax(self.facc, self.nsum, self.w, self.bsum, classes, prob_dtype=prob_dtype)

    def logits(self):
        """The accumulated ensemble logits [X,Y,Z,C] by torch (fp32) - for tests and small volumes only."""
        M, X, Y, Z, K = self.facc.shape
        out = (self.nsum[..., None] * self.bsum).float()
        for m in range(M):
            out = out + self.facc[m].reshape(-1, K).matmul(self.w[m].t()).reshape(X, Y, Z, -1)
        return out


def _mind_ahead_ok(model, dev):
    """The MIND descriptor of the NEXT window batch may be evaluated on a side stream while the network is in the current one
    (as tta.tta_epoch does for the next pass) when mind_hook is the last forward pre-hook and whatever stands in front of it
    leaves the input alone (gin_hook with the trainers' internal augmentation off, the plan's untouched input modifier).
    DGTTA_INFER_PREFETCH=0: in line."""
    from ..gin import gin_hook
    from ..mind import hook_owner, mind_hook
    from ..utils import get_internal_augmentation_enabled
    if torch.device(dev).type != "cuda" or os.environ.get("DGTTA_INFER_PREFETCH", "1") == "0":
        return False
    hooks = list(hook_owner(model)._forward_pre_hooks.values())
    if not hooks or hooks[-1] is not mind_hook or get_internal_augmentation_enabled():
        return False
    from .config_log_utils import is_template_modifier

    def leaves_input_alone(h):      # gin_hook (augmentation off, checked above) or the untouched template input modifier
        fn = getattr(h, "_dgtta_fn", None)
        return h is gin_hook or (fn is not None and is_template_modifier(fn, "modify_tta_input_fn"))
    return all(h is mind_hook or leaves_input_alone(h) for h in hooks) and sum(h is mind_hook for h in hooks) == 1


def _mirror_work(origins, mirror_axes):
    """The work list of a sliding-window pass: (origins, masks) with every window repeated once per mirror mask, in window order
    and, per window, in the order nnU-Net's predictor runs its mirrored passes (ops.mirror_masks).  Every mirrored pass is one
    more "window" of a batch: it adds gauss[p] * out[flip(p)] at origin + p and gauss[p] into nsum, so acc / nsum is the mean over
    the mirrors of the window-normalised logits and nothing downstream of the accumulators changes."""
    masks = ops.mirror_masks(mirror_axes)
    return [o for o in origins for _ in masks], [m for _ in origins for m in masks]


def _window_batches(model, data, origins, patch_size, dev, masks=None):
    """Yields (group, group_masks, work) per batch of WINDOW_BATCH windows.  masks: one mirror mask per origin (_mirror_work) -
    the batch is then built by ops.window_gather (one launch: slices and flips) instead of torch.stack.  Where _mind_ahead_ok,
    the window stack and its MIND descriptor (noise draw included: the draws keep their order, one batch after the other) are
    produced on a side stream one batch ahead and handed to the model's mind_hook (mind.push_features): same kernels, same draws,
    same result - the descriptor of a mirrored pass is that of the flipped window, as nnU-Net's hook order gives it."""
    from .._state import state_of
    from ..mind import MIND3D, hook_owner, push_features

    mirrored = masks is not None and any(masks)
    masks = [0] * len(origins) if masks is None else masks

    def stack(item):
        group, gmasks = item
        if mirrored:
            return ops.window_gather(data, group, gmasks, patch_size)
        return torch.stack([data[:, sx:sx + patch_size[0], sy:sy + patch_size[1], sz:sz + patch_size[2]]
                            for sx, sy, sz in group]).contiguous()

    groups = [(origins[g0:g0 + WINDOW_BATCH], masks[g0:g0 + WINDOW_BATCH]) for g0 in range(0, len(origins), WINDOW_BATCH)]
    if not groups:
        return
    if not _mind_ahead_ok(model, dev):
        for item in groups:
            yield item[0], item[1], stack(item)
        return
    main = torch.cuda.current_stream(dev)
    side = state_of(hook_owner(model)).stream("prep_stream", dev)
    adt = getattr(_inner(model), "act_dtype", torch.float32)
    side.wait_stream(main)          # once: the volume (uploaded on the main stream) is visible to the side stream

    def prepare(item):
        with torch.cuda.stream(side):
            work = stack(item)
            feat = MIND3D().forward(work, out_dtype=adt, groups=len(item[0]))
        for t in (work, feat):
            t.record_stream(main)
        return work, feat

    nxt = prepare(groups[0])
    try:
        for i, item in enumerate(groups):
            work, feat = nxt
            main.wait_stream(side)
            nxt = prepare(groups[i + 1]) if i + 1 < len(groups) else None      # runs beside this batch's network pass
            push_features(model, feat)
            yield item[0], item[1], work
    finally:
        state_of(hook_owner(model)).features.clear()      # (a descriptor no mind_hook call took must not meet a later input)


def _sliding_windows(model, data, patch_size, tile_step_size, mirror_axes, batch):
    """The sliding-window pass behind both accumulators: pads data [C,X,Y,Z] to the patch size, uploads it and sends every window,
    under every flip of mirror_axes (_mirror_work), through batch(work, group, gmasks, nsum, gauss) with the model in eval mode -
    work the stacked (flipped) windows of one network pass, group their origins, gmasks their mirror masks.  Returns (nsum, crop)."""
    dev = next(model.parameters()).device
    data, crop = pad_to_patch(data.float(), patch_size)
    data = data.to(dev)
    X, Y, Z = data.shape[1:]
    gauss = compute_gaussian(tuple(patch_size)).to(dev).contiguous()
    steps = compute_steps_for_sliding_window((X, Y, Z), patch_size, tile_step_size)
    nsum = torch.zeros((X, Y, Z), dtype=torch.float32, device=dev)
    was_training = model.training
    model.eval()
    # windows go through the network WINDOW_BATCH at a time: the 16^3-and-below layers are launch / occupancy bound at
    # batch 1 (same observation as in the TTA loop); per-sample InstanceNorm and per-window MIND statistics (below) make
    # the result independent of the grouping
    origins = [(sx, sy, sz) for sx in steps[0] for sy in steps[1] for sz in steps[2]]
    origins, masks = _mirror_work(origins, mirror_axes)
    for group, gmasks, work in _window_batches(model, data, origins, patch_size, dev, masks):
        # MIND's variance clamp uses the mean over the whole CALL's batch (mind.py:159-161) and nnU-Net predicts one
        # window per call: the batched pass keeps per-window statistics (groups = windows in the batch)
        with mind_groups(model, len(group)):
            batch(work, group, gmasks, nsum, gauss)
    model.train(was_training)
    return nsum, crop


def _mirrors_kw(gmasks):
    """The `mirrors` argument of a fuse_window_* context for one batch."""
    return {"mirrors": gmasks} if any(gmasks) else {}


@torch.no_grad()
def predict_sliding_window_return_logits(model, data, patch_size, acc=None, tile_step_size=0.5, acc_dtype=None, mirror_axes=None):
    """data [C,X,Y,Z] (CPU or GPU) -> accumulates gauss-weighted logits of `model` into acc [X,Y,Z,ncls] (GPU; fp32 or
    fp16: the dtype of a given `acc`, else `acc_dtype`, else window_acc_dtype()).
    Returns (acc, nsum, crop) ; logits = acc / nsum[..., None] cropped by `crop`.
    mirror_axes: None, or the subset of (0, 1, 2) nnU-Net's predictor mirrors along (module docstring): every window is then
    predicted under all 2^n flips, each un-flipped on its way into the accumulator; fp32 accumulator only."""
    mirror_axes = ops.check_mirror_axes(mirror_axes)
    if acc_dtype is None:
        acc_dtype = acc.dtype if acc is not None else window_acc_dtype()
    if acc_dtype not in (torch.float32, torch.float16):
        raise ValueError(f"the window accumulator is fp32 or fp16, not {acc_dtype}")
    if acc is not None and acc.dtype != acc_dtype:
        raise ValueError(f"acc is {acc.dtype} but acc_dtype = {acc_dtype}")
    if acc is not None and not (acc.is_cuda and acc.is_contiguous()):
        raise ValueError("acc must be a contiguous GPU tensor [X,Y,Z,classes]")
    if mirror_axes is not None and acc_dtype == torch.float16:
        raise ValueError(f"mirroring along {mirror_axes} with a fp16 window accumulator: {2 ** len(mirror_axes)} passes per window at "
                         "Gaussian weight 10 leave no headroom in half - use the fp32 logits accumulator (DGTTA_WINDOW_ACC=fp32) or "
                         "the feature-space accumulator (DGTTA_WINDOW_ACC=features)")
    lib = _lib.load()

    def batch(work, group, gmasks, nsum, gauss):
        nonlocal acc
        dev, vol = nsum.device, tuple(nsum.shape)
        if _can_fuse_head_accumulate(model):
            # the head evaluates straight into the accumulator (the windows' logits - 880 MB each at 128^3 x 105 - are not written)
            if acc is None:
                acc = torch.zeros((*vol, _num_classes(model)), dtype=acc_dtype, device=dev)
            with _inner(model).fuse_window_accumulate(acc, nsum, gauss, group, **_mirrors_kw(gmasks)):
                model(work)
            return
        out = model(work)
        if isinstance(out, tuple):
            out = out[0]
        out = out.float().contiguous(memory_format=torch.channels_last_3d)        # [n,C,P] stored voxel-major
        ncls = out.shape[1]
        if acc is None:
            acc = torch.zeros((*vol, ncls), dtype=acc_dtype, device=dev)
        for k, origin in enumerate(group):       # overlapping windows: accumulated one after the other
            args = (ptr(out[k]), ptr(gauss), ptr(acc), ptr(nsum), ncls, *patch_size, *vol, *origin, _acc_code(acc))
            if acc.dtype == torch.float32:       # a mirrored pass is un-flipped on its way into the accumulator (mask 0: no flip)
                check(lib.dgtta_window_accumulate_mirror_t(*args, gmasks[k], stream_of(dev)), "dgtta_window_accumulate_mirror_t")
            else:                                # (the _mirror entry takes fp32 accumulators only; fp16 is never mirrored: above)
                check(lib.dgtta_window_accumulate_t(*args, stream_of(dev)), "dgtta_window_accumulate_t")

    nsum, crop = _sliding_windows(model, data, patch_size, tile_step_size, mirror_axes, batch)
    return acc, nsum, crop


@torch.no_grad()
def accumulate_window_features(model, data, patch_size, facc=None, tile_step_size=0.5, mirror_axes=None):
    """The feature-space form of predict_sliding_window_return_logits for one member: data [C,X,Y,Z] -> adds gauss * (the head's
    input of every window, under every flip of mirror_axes) into facc [X,Y,Z,32] (fp32, GPU; allocated when None).  Returns
    (facc, nsum, crop)."""
    mirror_axes = ops.check_mirror_axes(mirror_axes)
    m = _inner(model)
    if not _can_accumulate_features(model):
        raise RuntimeError("accumulate_window_features: the network does not offer the feature-space accumulation here")
    X, Y, Z = (max(have, want) for have, want in zip(data.shape[1:], patch_size))      # the padded volume (pad_to_patch)
    if facc is None:
        facc = torch.zeros((X, Y, Z, 32), dtype=torch.float32, device=next(model.parameters()).device)
    if tuple(facc.shape) != (X, Y, Z, 32) or facc.dtype != torch.float32 or not (facc.is_cuda and facc.is_contiguous()):
        raise ValueError(f"facc must be a contiguous fp32 GPU tensor [{X},{Y},{Z},32]")

    def batch(work, group, gmasks, nsum, gauss):
        with m.fuse_window_feature_accumulate(facc, nsum, gauss, group, **_mirrors_kw(gmasks)):
            model(work)

    nsum, crop = _sliding_windows(model, data, patch_size, tile_step_size, mirror_axes, batch)
    return facc, nsum, crop


@torch.no_grad()
def predict_ensemble_features(data, model, parameter_sets, patch_size, mirror_axes=None):
    """Feature-space accumulators of the whole ensemble for one preprocessed case (see WindowFeatures); one [X,Y,Z,32] fp32
    volume per member, because the members' heads differ."""
    if hasattr(model, "set_selected_classes"):
        model.set_selected_classes(None)          # argmax runs over ALL pretrain classes, as in the reference
    dev = next(model.parameters()).device
    data = data.float().to(dev)      # one upload for all ensemble members
    padded, _ = pad_to_patch(data[:1], patch_size)
    facc = torch.zeros((len(parameter_sets), *padded.shape[1:], 32), dtype=torch.float32, device=dev)
    del padded
    ws, bs, nsum, crop = [], [], None, None
    for k, params in enumerate(parameter_sets):
        model.load_state_dict(params)
        head = _inner(model).decoder.seg_layers[-1]
        ws.append(head.weight.detach().reshape(head.out_channels, -1).float().clone())
        bs.append(head.bias.detach().float().clone())
        _, nsum, crop = accumulate_window_features(model, data, patch_size, facc[k], mirror_axes=mirror_axes)
    return WindowFeatures(facc, nsum, crop, torch.stack(ws), torch.stack(bs))


@torch.no_grad()
def predict_ensemble(data, model, parameter_sets, patch_size, mirror_axes=None, regions=False):
    """What run_inference / dgtta run_tta predict with: (acc, nsum, crop) for export_segmentation - acc a WindowFeatures when
    DGTTA_WINDOW_ACC=features (default) and the network offers it, else the logits-space accumulator of predict_ensemble_logits.
    mirror_axes: the checkpoint's inference_allowed_mirroring_axes (None for the DG trainers).  regions: the head is a region head
    (the feature-space form is then offered for the heads the region label-map kernel takes)."""
    if window_acc_mode() == "features" and _can_accumulate_features(model, len(parameter_sets), regions=regions):
        feats = predict_ensemble_features(data, model, parameter_sets, patch_size, mirror_axes)
        return feats, feats.nsum, feats.crop
    return predict_ensemble_logits(data, model, parameter_sets, patch_size, mirror_axes)


@torch.no_grad()
def predict_ensemble_logits(data, model, parameter_sets, patch_size, mirror_axes=None):
    """Window-accumulated logits of the whole ensemble for one preprocessed case: data [C,X,Y,Z] (image channel(s) only),
    parameter_sets: list of state dicts (the `*_tta_parameters.pt` contents).  Returns (acc [X,Y,Z,ncls] fp32 on the GPU =
    sum over members and windows of gauss * logits, nsum [X,Y,Z], crop): the ensemble-mean logits nnU-Net's predictor hands
    on are acc / nsum / len(parameter_sets) inside `crop`."""
    if hasattr(model, "set_selected_classes"):
        model.set_selected_classes(None)          # argmax runs over ALL pretrain classes, as in the reference
    acc, nsum, crop = None, None, None
    data = data.float().to(next(model.parameters()).device)      # one upload for all ensemble members
    for params in parameter_sets:
        model.load_state_dict(params)
        acc, nsum, crop = predict_sliding_window_return_logits(model, data, patch_size, acc, mirror_axes=mirror_axes)
    return acc, nsum, crop


@torch.no_grad()
def run_inference(data, model, parameter_sets, patch_size, label_mapping=None, optimized_labels=None, mirror_axes=None,
                  regions_class_order=None):
    """Ensemble prediction of one preprocessed case in the PREPROCESSED geometry.  Returns the label map [X,Y,Z] (int64,
    CPU), mapped to the target ids when label_mapping/optimized_labels are given (tta.py:407-411).
    regions_class_order: the model is a region model (dg_tta_amd/labels.py) - its R outputs are sigmoid logits of overlapping
    regions and the label map is the region one (0, then regions_class_order[i] wherever the ensemble-mean logit of output i is
    > 0, in order) instead of the argmax, for both accumulators, mirroring included.  No label mapping then."""
    from .torch_utils import get_map_idxs
    if regions_class_order is not None:
        if label_mapping is not None:
            raise ValueError("run_inference: a region label map holds regions_class_order's labels; there is no label mapping for it")
        regions_class_order = ops.check_regions_class_order(regions_class_order, _num_classes(model))
    acc, nsum, crop = predict_ensemble(data, model, parameter_sets, patch_size, mirror_axes, regions=regions_class_order is not None)
    seg = torch.as_tensor(export_segmentation(acc, nsum, crop, None, None, None, regions_class_order).astype(np.int64))
    if label_mapping is not None:
        seg = map_label(seg[None], get_map_idxs(label_mapping, optimized_labels, "pretrain_labels"), "argmaxed")[0]
    return seg


EXPORT_CLASS_GROUP = 8


def _resolved_configuration(plans, configuration):
    conf = plans["configurations"][configuration]
    while "inherits_from" in conf:
        parent = dict(plans["configurations"][conf["inherits_from"]])
        parent.update({k: v for k, v in conf.items() if k != "inherits_from"})
        conf = parent
    return conf


@torch.no_grad()
def export_segmentation(acc, nsum, crop, properties, plans, configuration, regions_class_order=None):
    """Label map (pretrain class ids, numpy) of accumulated ensemble logits.
    regions_class_order (a region head): the region label map replaces the argmax - the sign of the accumulated logit is the sign
    of the ensemble mean, so there is no division pass either.  With `properties` the logits are resampled as below and merged by
    dgtta_regions_merge_f64 (_RunningRegions) instead of the running argmax; the map then holds regions_class_order's labels.

    properties None: argmax in the preprocessed geometry (sum over members of acc_m / nsum has the argmax of sum_m acc_m,
    nsum > 0 being shared: no division pass).  Otherwise nnU-Net's
    convert_predicted_logits_to_segmentation_with_correct_shape [3P nnunetv2==2.2.1, reached from
    dg_tta/tta/nnunet_utils.py:208-230]: the normalised logits are resampled to
    properties['shape_after_cropping_and_before_resampling'] with the plans' probability resampler (linear; nearest along
    a strongly anisotropic axis), argmax'd (softmax is monotone), pasted into a zero volume of 'shape_before_cropping' at
    'bbox_used_for_cropping' and transposed back with the plans' transpose_backward.  The resampling runs on the GPU class
    group by class group with a running argmax, so the full-resolution 105-class volume never exists."""
    C = acc.shape[3]
    if regions_class_order is not None:
        regions_class_order = ops.check_regions_class_order(regions_class_order, C)
    label_map = _label_map_fn(acc, regions_class_order)
    cs, cur_shape = _crop_extents(acc, crop)
    if properties is None:
        return label_map()[tuple(crop)].cpu().numpy()
    tgt_shape = [int(v) for v in properties["shape_after_cropping_and_before_resampling"]]
    if tgt_shape == cur_shape:
        seg = label_map()[tuple(crop)].cpu().numpy()
    else:
        orders = _probability_resampling_orders(properties, plans, configuration)
        merge = _RunningArgmax(tgt_shape, nsum.device) if regions_class_order is None else \
            _RunningRegions(tgt_shape, nsum.device, regions_class_order, 1.0)      # (labels only: the scale is not read)
        for c0, cg, cur in _resampled_class_groups(acc, nsum, cs, tgt_shape, orders):
            merge.add(cur, c0, cg)
        seg = merge.labels()
    return _paste_label_map(seg, C, properties, plans, max_label=_max_label(C, regions_class_order))


def _label_map_fn(acc, regions_class_order=None):
    if regions_class_order is not None:
        return (lambda: acc.regions(regions_class_order)) if isinstance(acc, WindowFeatures) else \
            (lambda: ops.logits_regions(acc, regions_class_order))
    return (lambda: acc.argmax()) if isinstance(acc, WindowFeatures) else (lambda: ops.argmax_rows(acc))


def _crop_extents(acc, crop):
    """((x0, xs), (y0, ys), (z0, zs)) of the crop slices inside the padded accumulator, and [xs, ys, zs]."""
    cs = [(sl.start or 0, (sl.stop if sl.stop is not None else dim) - (sl.start or 0)) for sl, dim in zip(crop, acc.shape[:3])]
    return cs, [c[1] for c in cs]


def _probability_resampling_orders(properties, plans, configuration):
    """Interpolation order per axis of the plans' probability resampler: linear (or nearest), nearest slices along a strongly
    anisotropic axis."""
    from .preprocessing import separate_z
    conf = _resolved_configuration(plans, configuration)
    cur_spacing = list(conf["spacing"])
    if len(cur_spacing) < 3:
        cur_spacing = [properties["spacing"][0]] + cur_spacing
    kw = conf.get("resampling_fn_probabilities_kwargs", {"order": 1, "order_z": 0})
    order, order_z = int(kw.get("order", 1)), int(kw.get("order_z", 0))
    if order not in (0, 1) or order_z != 0:
        raise NotImplementedError("probability resampling is built for order 0 / 1 and order_z 0 (nnU-Net's defaults)")
    do_sep, axis = separate_z(cur_spacing, properties["spacing"])
    return [0 if (do_sep and ax == axis) else order for ax in range(3)]      # nearest slices along the low-resolution axis


def _resampled_class_groups(acc, nsum, cs, tgt_shape, orders):
    """The export loop export_segmentation and export_probabilities share: yields (c0, cg, vals) per group of EXPORT_CLASS_GROUP
    classes, vals [*tgt_shape, cg] float64 on the GPU = the SUM over members of the window-normalised logits of classes c0..,
    cropped back from the padding and resampled axis by axis to tgt_shape (no pass along an axis that already has its size)."""
    lib = _lib.load()
    feats = acc if isinstance(acc, WindowFeatures) else None
    dev = nsum.device
    X, Y, Z, C = acc.shape
    st = stream_of(dev)
    (x0, xs), (y0, ys), (z0, zs) = cs
    for c0 in range(0, C, EXPORT_CLASS_GROUP):
        cg = min(EXPORT_CLASS_GROUP, C - c0)
        cur = torch.empty((xs, ys, zs, cg), dtype=torch.float64, device=dev)
        if feats is not None:
            M = feats.facc.shape[0]
            check(lib.dgtta_feature_logits_chunk_f64(ptr(feats.facc), feats.facc.stride(0), ptr(nsum), ptr(feats.w), ptr(feats.bsum),
                                                     ptr(cur), M, 32, C, X, Y, Z, x0, y0, z0, xs, ys, zs, c0, cg, st),
                  "dgtta_feature_logits_chunk_f64")
        else:
            check(lib.dgtta_logits_chunk_f64_t(ptr(acc), ptr(nsum), ptr(cur), C, X, Y, Z, x0, y0, z0, xs, ys, zs, c0, cg,
                                               _acc_code(acc), st), "dgtta_logits_chunk_f64_t")
        for ax in range(3):          # channels-last: the class group rides in `inner` of every pass
            n, m = cur.shape[ax], tgt_shape[ax]
            if n == m:
                continue
            shp = list(cur.shape[:3])
            outer = int(np.prod(shp[:ax], dtype=np.int64))
            inner = int(np.prod(shp[ax + 1:], dtype=np.int64)) * cg
            dst = torch.empty((*shp[:ax], m, *shp[ax + 1:], cg), dtype=torch.float64, device=dev)
            check(lib.dgtta_resample_axis(ptr(cur), ptr(dst), None, 0, outer, n, m, inner, orders[ax], st), "dgtta_resample_axis")
            cur = dst
        yield c0, cg, cur


class _RunningArgmax:
    """dgtta_argmax_merge_f64 over the class groups: the label map of the resampled logits, first maximum wins."""

    def __init__(self, shape, dev):
        self.shape, self.dev = list(shape), dev
        self.vout = int(np.prod(shape, dtype=np.int64))
        self.best_val = torch.empty(self.vout, dtype=torch.float64, device=dev)
        self.best_idx = torch.empty(self.vout, dtype=torch.int32, device=dev)

    def add(self, vals, c0, cg):
        check(_lib.load().dgtta_argmax_merge_f64(ptr(vals), self.vout, cg, c0, ptr(self.best_val), ptr(self.best_idx), int(c0 == 0),
                                                 stream_of(self.dev)), "dgtta_argmax_merge_f64")

    def labels(self):
        return self.best_idx.reshape(self.shape).cpu().numpy()


class _RunningSoftmax:
    """dgtta_softmax_merge_f64 / dgtta_softmax_finalize_f64 over the class groups (online softmax: running maximum, sum exp and
    sum (l - max) exp per voxel, rescaled when the maximum moves).  The scaled logits of the K selected classes wait in a float64
    stash [K, V]: 8 K V bytes - 17 GB at 512^3 with K = 16, which the 288 GB of an MI355X carry."""

    def __init__(self, shape, dev, sel, scale, prob_dtype):
        import ctypes
        self.shape, self.dev, self.K, self.scale, self.prob_dtype = list(shape), dev, len(sel), float(scale), prob_dtype
        self.sel = (ctypes.c_int * len(sel))(*sel)
        self.vout = int(np.prod(shape, dtype=np.int64))
        self.state = torch.empty((3, self.vout), dtype=torch.float64, device=dev)
        self.stash = torch.empty((self.K, self.vout), dtype=torch.float64, device=dev)

    def add(self, vals, c0, cg):
        m, s, d = self.state[0], self.state[1], self.state[2]
        check(_lib.load().dgtta_softmax_merge_f64(ptr(vals), self.vout, cg, c0, self.scale, ptr(m), ptr(s), ptr(d), self.sel, self.K,
                                                  ptr(self.stash), int(c0 == 0), stream_of(self.dev)), "dgtta_softmax_merge_f64")

    def finalize(self):
        """(confidence fp32 [*shape], entropy fp32 [*shape], probs prob_dtype [K, *shape]) on the GPU."""
        conf = torch.empty(self.vout, dtype=torch.float32, device=self.dev)
        ent = torch.empty(self.vout, dtype=torch.float32, device=self.dev)
        probs = torch.empty((self.K, self.vout), dtype=self.prob_dtype, device=self.dev)
        m, s, d = self.state[0], self.state[1], self.state[2]
        check(_lib.load().dgtta_softmax_finalize_f64(ptr(m), ptr(s), ptr(d), ptr(self.stash), self.vout, self.K,
                                                     ops.prob_dtype_code(self.prob_dtype), ptr(conf), ptr(ent), ptr(probs),
                                                     stream_of(self.dev)), "dgtta_softmax_finalize_f64")
        return conf.reshape(self.shape), ent.reshape(self.shape), probs.reshape(self.K, *self.shape)


class _RunningRegions:
    """dgtta_regions_merge_f64 over the class groups: the region label map of the resampled logits (0, then order[i] wherever the
    summed logit of output i is > 0, in order: the last positive region wins) and, with prob_dtype, the sigmoid of the
    ensemble-mean logit scale * vals of every output in planes [R, V] - written group by group, no stash."""

    def __init__(self, shape, dev, order, scale, prob_dtype=None):
        import ctypes
        self.shape, self.dev, self.R, self.scale, self.prob_dtype = list(shape), dev, len(order), float(scale), prob_dtype
        self.order = (ctypes.c_int * len(order))(*[int(v) for v in order])
        self.vout = int(np.prod(shape, dtype=np.int64))
        self.label = torch.empty(self.vout, dtype=torch.int32, device=dev)
        self.probs = None if prob_dtype is None else torch.empty((self.R, self.vout), dtype=prob_dtype, device=dev)
        self.code = 0 if prob_dtype is None else ops.prob_dtype_code(prob_dtype)

    def add(self, vals, c0, cg):
        check(_lib.load().dgtta_regions_merge_f64(ptr(vals), self.vout, cg, c0, self.scale, self.order, self.R, ptr(self.label),
                                                  ptr(self.probs), self.code, int(c0 == 0), stream_of(self.dev)),
              "dgtta_regions_merge_f64")

    def labels(self):
        return self.label.reshape(self.shape).cpu().numpy()

    def probabilities(self):
        """probs prob_dtype [R, *shape] on the GPU."""
        if self.probs is None:
            raise ValueError("_RunningRegions was built without a probability type")
        return self.probs.reshape(self.R, *self.shape)


def _max_label(C, regions_class_order=None):
    """The largest value a label map can hold: the last class id, or the largest label of regions_class_order."""
    return C - 1 if regions_class_order is None else max(int(v) for v in regions_class_order)


def _paste_label_map(seg, C, properties, plans, max_label=None):
    """max_label: the largest value the map can hold (C - 1 when None: class ids); it picks the integer type."""
    max_label = C - 1 if max_label is None else int(max_label)
    full = np.zeros(tuple(int(v) for v in properties["shape_before_cropping"]),
                    dtype=np.uint8 if max_label < 255 else np.uint16 if max_label <= 65535 else np.uint32)
    sl = tuple(slice(int(a), int(b)) for a, b in properties["bbox_used_for_cropping"])
    full[sl] = seg
    return np.ascontiguousarray(full.transpose(plans["transpose_backward"]))


def can_fuse_head_softmax(acc):
    """True when dgtta_feature_head_softmax takes this accumulator (a WindowFeatures whose head it supports) - decided before any
    work is done, as _can_accumulate_features does; everything else goes through the class-group loop."""
    return isinstance(acc, WindowFeatures) and ops.feature_head_softmax_supported(acc.facc.shape[0], acc.shape[3])


@torch.no_grad()
def export_probabilities(acc, nsum, crop, properties, plans, configuration, members, classes, prob_dtype=np.float16):
    """Softmax end of accumulated ensemble logits, in the geometry export_segmentation returns (properties None: the preprocessed
    geometry; otherwise resampled, pasted into `shape_before_cropping` and transposed back).  Returns a dict of numpy arrays:

      segmentation   the label map export_segmentation returns for the same accumulators
      probabilities  [K, ...] `prob_dtype` (float16 or float32): p[classes[k]] - 1..32 distinct classes in any order.  The K maps sum
                     to at most 1; the rest is mass on classes that were not selected
      confidence     float32, p[label] of the voxel's own argmax
      entropy        float32, -sum_c p_c ln p_c in nats, in [0, ln C]

    p = softmax over ALL pretrain classes of the ensemble-MEAN logits acc / nsum / members (`members`: the number of parameter
    sets accumulated into acc).  Resampled exports resample the logits first and take the softmax afterwards, nnU-Net's order
    and the one the running argmax assumes.  Outside the crop box class 0 has probability 1 (confidence 1, entropy 0), consistent
    with the zero fill of the label map.  The definitions are nnU-Net's `save_probabilities` ones from memory: UNPINNED, like the
    window logic of this module.

    Routing: dgtta_feature_head_softmax (one fused pass on the matrix cores) when acc is a WindowFeatures it supports and the
    target shape is the preprocessed one; otherwise the class-group loop of export_segmentation with the online-softmax merge
    (logits-space accumulators, heads wider than 128 classes, every resampled export)."""
    C = acc.shape[3]
    sel = ops.check_selected_classes(classes, C)
    tdtype = {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32}.get(np.dtype(prob_dtype))
    if tdtype is None:
        raise ValueError(f"probabilities are stored as float16 or float32, not {prob_dtype}")
    members = int(members)
    if members < 1 or (isinstance(acc, WindowFeatures) and acc.facc.shape[0] != members):
        raise ValueError(f"members = {members} does not match the accumulator")
    cs, cur_shape = _crop_extents(acc, crop)
    tgt_shape = cur_shape if properties is None else [int(v) for v in properties["shape_after_cropping_and_before_resampling"]]
    resample = tgt_shape != cur_shape
    if not resample and can_fuse_head_softmax(acc):
        label, conf, ent, probs = acc.softmax(sel, prob_dtype=tdtype)
        seg = label[tuple(crop)].cpu().numpy()
        conf, ent, probs = conf[tuple(crop)], ent[tuple(crop)], probs[(slice(None), *crop)]
    else:
        orders = _probability_resampling_orders(properties, plans, configuration) if resample else [0, 0, 0]
        # without resampling the label is export_segmentation's own argmax of the fp32 accumulators (a float64 argmax of the
        # normalised values could break a rounding-level tie the other way)
        merge = _RunningArgmax(tgt_shape, nsum.device) if resample else None
        soft = _RunningSoftmax(tgt_shape, nsum.device, sel, 1.0 / members, tdtype)
        for c0, cg, cur in _resampled_class_groups(acc, nsum, cs, tgt_shape, orders):
            if merge is not None:
                merge.add(cur, c0, cg)
            soft.add(cur, c0, cg)
        seg = merge.labels() if resample else _label_map_fn(acc)()[tuple(crop)].cpu().numpy()
        conf, ent, probs = soft.finalize()
    conf, ent, probs = conf.cpu().numpy(), ent.cpu().numpy(), probs.cpu().numpy()
    if properties is None:
        return {"segmentation": seg, "probabilities": np.ascontiguousarray(probs), "confidence": np.ascontiguousarray(conf),
                "entropy": np.ascontiguousarray(ent)}
    full_shape = tuple(int(v) for v in properties["shape_before_cropping"])
    sl = tuple(slice(int(a), int(b)) for a, b in properties["bbox_used_for_cropping"])
    full_p = np.zeros((len(sel), *full_shape), dtype=probs.dtype)
    if 0 in sel:
        full_p[sel.index(0)] = 1      # outside the box: background with probability 1
    full_c, full_e = np.ones(full_shape, dtype=np.float32), np.zeros(full_shape, dtype=np.float32)
    full_p[(slice(None), *sl)], full_c[sl], full_e[sl] = probs, conf, ent
    tb = [int(a) for a in plans["transpose_backward"]]
    return {"segmentation": _paste_label_map(seg, C, properties, plans),
            "probabilities": np.ascontiguousarray(full_p.transpose([0] + [a + 1 for a in tb])),
            "confidence": np.ascontiguousarray(full_c.transpose(tb)), "entropy": np.ascontiguousarray(full_e.transpose(tb))}


@torch.no_grad()
def export_region_probabilities(acc, nsum, crop, properties, plans, configuration, members, regions_class_order,
                                prob_dtype=np.float16):
    """Sigmoid end of the accumulated ensemble logits of a REGION head, in the geometry export_segmentation returns (properties
    None: the preprocessed geometry; otherwise resampled, pasted into `shape_before_cropping` and transposed back).  Returns

      segmentation   the label map export_segmentation(..., regions_class_order=...) returns for the same accumulators
      probabilities  [R, ...] `prob_dtype` (float16 or float32): p_i = sigmoid(l_i), l_i the ensemble-MEAN window-normalised logit
                     acc / nsum / members of output i.  The regions overlap: the planes do not sum to 1

    Resampled exports resample the logits first and squash afterwards - nnU-Net 2.2.1's order from memory, UNPINNED, the one
    export_probabilities states.  Outside the crop box: label 0 and probability 0.  Always the class-group loop (orders [0, 0, 0]
    when nothing is resampled); the label of an unresampled export is _label_map_fn's own - dividing a non-zero fp32 sum by a
    positive weight in double cannot change its sign, so both routes agree."""
    C = acc.shape[3]
    order = ops.check_regions_class_order(regions_class_order, C)
    tdtype = {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32}.get(np.dtype(prob_dtype))
    if tdtype is None:
        raise ValueError(f"probabilities are stored as float16 or float32, not {prob_dtype}")
    members = int(members)
    if members < 1 or (isinstance(acc, WindowFeatures) and acc.facc.shape[0] != members):
        raise ValueError(f"members = {members} does not match the accumulator")
    cs, cur_shape = _crop_extents(acc, crop)
    tgt_shape = cur_shape if properties is None else [int(v) for v in properties["shape_after_cropping_and_before_resampling"]]
    resample = tgt_shape != cur_shape
    orders = _probability_resampling_orders(properties, plans, configuration) if resample else [0, 0, 0]
    merge = _RunningRegions(tgt_shape, nsum.device, order, 1.0 / members, tdtype)
    for c0, cg, cur in _resampled_class_groups(acc, nsum, cs, tgt_shape, orders):
        merge.add(cur, c0, cg)
    seg = merge.labels() if resample else _label_map_fn(acc, order)()[tuple(crop)].cpu().numpy()
    probs = merge.probabilities().cpu().numpy()
    if properties is None:
        return {"segmentation": seg, "probabilities": np.ascontiguousarray(probs)}
    full_shape = tuple(int(v) for v in properties["shape_before_cropping"])
    sl = tuple(slice(int(a), int(b)) for a, b in properties["bbox_used_for_cropping"])
    full_p = np.zeros((C, *full_shape), dtype=probs.dtype)
    full_p[(slice(None), *sl)] = probs
    tb = [int(a) for a in plans["transpose_backward"]]
    return {"segmentation": _paste_label_map(seg, C, properties, plans, max_label=_max_label(C, order)),
            "probabilities": np.ascontiguousarray(full_p.transpose([0] + [a + 1 for a in tb]))}
