"""nnU-Net's intensity augmentations for `dgtta pretrain --augmentation full`: what is drawn per batch item (host, float64)
and the chain of kernels (ops.intensity_stats / intensity_map / gauss_blur3, csrc/intensity_aug.hip) the draws are handed to.
Restated from memory of nnunetv2 2.2's training transforms / batchgenerators (UNPINNED, like pretraining/spatial.py and the
trainer around it).  The network takes one image channel, so batchgenerators' per-channel probabilities multiply into the
per-item ones below.

The order is transform-major - stage k is applied to every item of the batch, then stage k + 1 - and so are the draws: all
items of stage 1, then all items of stage 2, ...  Per item inside a stage, in this order, every draw from utils.numpy_rng()
(or the generator handed in; only its uniform() is called):

  1 Gaussian noise   u < 0.1                 s ~ U(0, 0.1); two 32-bit words floor(u 2^32), u ~ U(0, 1): the low and the high
                                             half of the 64-bit key of the item's noise field;   x + s n(v)
  2 Gaussian blur    u < 0.2, then u < 0.5   sigma ~ U(0.5, 1);   scipy.ndimage.gaussian_filter(x, sigma) (order 0, "reflect",
                                             truncate 4: radius int(4 sigma + 0.5) = 2, 3 or 4)
  3 brightness       u < 0.15                m ~ U(0.75, 1.25);   x m
  4 contrast         u < 0.15                u < 0.5 ? f ~ U(0.75, 1) : f ~ U(1, 1.25);   clip((x - mean) f + mean, min, max)
                                             with the item's mean / min / max before the stage
  5 low resolution   u < 0.25, then u < 0.5  zoom ~ U(0.5, 1);   resize to round(shape zoom) with order 0 and back with order 3
                                             (skimage.resize(mode="edge", anti_aliasing=False), clipped to the input range:
                                             discrete_downsampling._resize); the thin axis of spatial.thin_axis is left alone
  6 gamma, inverted  u < 0.1                 u < 0.5 ? g ~ U(0.7, 1) : g ~ U(1, 1.5);   x = -x, stage 7's formula, x = -x
  7 gamma            u < 0.3                 the same draws;   with mn, sd the mean and population std before the stage, lo the
                                             minimum and r the range: x = ((x - lo) / (r + 1e-7))^g r + lo, then with mn2, sd2
                                             of that result x = (x - mn2) / (sd2 + 1e-8) sd + mn

A draw that follows "then" or "?" is taken only when the one before it fired.  For the *_MultiRes trainers stage 5 is the
reference's SimulateDiscreteLowResolutionTransform (draw(discrete_lowres=)): no draw of stage 5 is taken here, the transform
runs at this position of the chain and keeps its own draws on numpy's global generator.

The noise n(v) is counter-based (Philox4x32-10 + Box-Muller, include/dgtta.h): a function of the item's key, its index in the
batch and the voxel, generated inside the kernel; there is no noise tensor and torch's generator is not used.

apply() issues no host synchronisation and no device-to-host copy: all parameters are drawn before the first launch and the
statistics of stages 4, 6 and 7 stay on the device.  Labels are never touched."""
from dataclasses import dataclass, field
from typing import Any, List, Optional

from ..utils import numpy_rng
from .spatial import thin_axis

STAGES = ("noise", "blur", "brightness", "contrast", "lowres", "gamma_inverted", "gamma")


@dataclass
class IntensityPlan:
    """The draws of one batch: per stage a list with, per item, its parameters or None (the stage did not fire).
    noise: (s, key); blur: sigma; brightness: m; contrast: f; lowres: zoom - or the discrete transform itself in place of the
    list; gamma_inverted, gamma: g.  thin: the axis stage 5 leaves alone, or None."""
    batch_size: int
    noise: List[Optional[tuple]] = field(default_factory=list)
    blur: List[Optional[float]] = field(default_factory=list)
    brightness: List[Optional[float]] = field(default_factory=list)
    contrast: List[Optional[float]] = field(default_factory=list)
    lowres: Any = field(default_factory=list)
    gamma_inverted: List[Optional[float]] = field(default_factory=list)
    gamma: List[Optional[float]] = field(default_factory=list)
    thin: Optional[int] = None

    def fired(self, stage):
        """Indices of the items whose `stage` fired (every item for the discrete low-resolution transform: it decides itself)."""
        v = getattr(self, stage)
        if not isinstance(v, list):
            return list(range(self.batch_size))
        return [i for i, p in enumerate(v) if p is not None]


def _word(rng):
    return min(int(rng.uniform() * 4294967296.0), 0xFFFFFFFF)


def simulate_low_resolution(volume, zoom, thin=None):
    """Stage 5 on one float32 CUDA volume [D, H, W]: down with order 0 to round(shape * zoom), back with order 3, each
    clipped to its input's range; axis `thin` keeps its extent.  Returns a new float32 tensor."""
    import numpy as np
    from .discrete_downsampling import _resize
    shape = [int(s) for s in volume.shape]
    target = [int(t) for t in np.round(np.asarray(shape, dtype=np.float64) * float(zoom))]
    target = [max(t, 1) for t in target]
    if thin is not None:
        target[thin] = shape[thin]
    vol = volume.double()
    return _resize(_resize(vol, target, 0), shape, 3).to(volume.dtype)


class IntensityAugmentation:
    """draw(batch_size, patch) -> IntensityPlan; apply(images, plan) -> the augmented batch (module docstring)."""

    def __init__(self, p_noise=0.1, noise_scale=(0.0, 0.1), p_blur=0.2, p_blur_channel=0.5, blur_sigma=(0.5, 1.0),
                 p_brightness=0.15, brightness=(0.75, 1.25), p_contrast=0.15, contrast=(0.75, 1.25), p_lowres=0.25,
                 p_lowres_channel=0.5, lowres_zoom=(0.5, 1.0), p_gamma_inverted=0.1, p_gamma=0.3, gamma=(0.7, 1.5)):
        if not 0.0 < blur_sigma[0] <= blur_sigma[1] <= 1.0:
            raise ValueError(f"blur sigma range {blur_sigma}: inside (0, 1] expected (ops.gauss_blur3 holds 9 taps)")
        if not 0.0 < lowres_zoom[0] <= lowres_zoom[1] <= 1.0:
            raise ValueError(f"zoom range {lowres_zoom}: inside (0, 1] expected")
        for name, (lo, hi) in (("contrast", contrast), ("gamma", gamma)):
            if not 0.0 < lo <= 1.0 <= hi:
                raise ValueError(f"{name} range {(lo, hi)}: 0 < low <= 1 <= high expected")
        if not 0.0 <= noise_scale[0] <= noise_scale[1]:
            raise ValueError(f"noise scale range {noise_scale}: 0 <= low <= high expected")
        self.p_noise, self.noise_scale = float(p_noise), tuple(noise_scale)
        self.p_blur, self.p_blur_channel, self.blur_sigma = float(p_blur), float(p_blur_channel), tuple(blur_sigma)
        self.p_brightness, self.brightness = float(p_brightness), tuple(brightness)
        self.p_contrast, self.contrast = float(p_contrast), tuple(contrast)
        self.p_lowres, self.p_lowres_channel, self.lowres_zoom = float(p_lowres), float(p_lowres_channel), tuple(lowres_zoom)
        self.p_gamma_inverted, self.p_gamma, self.gamma = float(p_gamma_inverted), float(p_gamma), tuple(gamma)

    # -------------------------------------------------------------------------------------------- draws
    @staticmethod
    def _two_sided(rng, rng_range):
        lo, hi = (rng_range[0], 1.0) if rng.uniform() < 0.5 else (1.0, rng_range[1])
        return float(rng.uniform(lo, hi))

    def draw(self, batch_size, patch, rng=None, discrete_lowres=None):
        rng = numpy_rng() if rng is None else rng
        n = int(batch_size)
        plan = IntensityPlan(batch_size=n, thin=thin_axis(patch))
        for _ in range(n):
            if rng.uniform() < self.p_noise:
                s = float(rng.uniform(*self.noise_scale))
                lo, hi = _word(rng), _word(rng)
                plan.noise.append((s, lo | (hi << 32)))
            else:
                plan.noise.append(None)
        for _ in range(n):
            fired = rng.uniform() < self.p_blur and rng.uniform() < self.p_blur_channel
            plan.blur.append(float(rng.uniform(*self.blur_sigma)) if fired else None)
        for _ in range(n):
            plan.brightness.append(float(rng.uniform(*self.brightness)) if rng.uniform() < self.p_brightness else None)
        for _ in range(n):
            plan.contrast.append(self._two_sided(rng, self.contrast) if rng.uniform() < self.p_contrast else None)
        if discrete_lowres is not None:
            plan.lowres = discrete_lowres
        else:
            for _ in range(n):
                fired = rng.uniform() < self.p_lowres and rng.uniform() < self.p_lowres_channel
                plan.lowres.append(float(rng.uniform(*self.lowres_zoom)) if fired else None)
        for _ in range(n):
            plan.gamma_inverted.append(self._two_sided(rng, self.gamma) if rng.uniform() < self.p_gamma_inverted else None)
        for _ in range(n):
            plan.gamma.append(self._two_sided(rng, self.gamma) if rng.uniform() < self.p_gamma else None)
        return plan

    # -------------------------------------------------------------------------------------------- the chain
    def apply(self, images, plan):
        """images [B, 1, D, H, W] float32 on the GPU -> a new tensor of that shape; stage by stage, 16 items per launch."""
        import torch
        from .. import ops
        if images.dim() != 5 or images.shape[1] != 1 or images.shape[0] != plan.batch_size:
            raise ValueError(f"IntensityAugmentation.apply: images {tuple(images.shape)} for a plan of {plan.batch_size} items; "
                             f"[B, 1, D, H, W] expected")
        x = images.clone(memory_format=torch.contiguous_format)

        def chunks(idx, n=ops._lib.INTENSITY_MAX_ITEMS):       # a stage that fired for no item launches nothing
            return [idx[k:k + n] for k in range(0, len(idx), n)]
        for idx in chunks(plan.fired("noise")):
            ops.intensity_map(x, idx, "linear", s=[plan.noise[i][0] for i in idx], keys=[plan.noise[i][1] for i in idx])
        scratch = None
        for idx in chunks(plan.fired("blur")):
            scratch = torch.empty_like(x) if scratch is None else scratch
            ops.gauss_blur3(x, idx, [plan.blur[i] for i in idx], scratch=scratch)
        for idx in chunks(plan.fired("brightness")):
            ops.intensity_map(x, idx, "linear", a=[plan.brightness[i] for i in idx])
        for idx in chunks(plan.fired("contrast")):
            ops.intensity_map(x, idx, "contrast", a=[plan.contrast[i] for i in idx], stats=ops.intensity_stats(x, idx))
        if isinstance(plan.lowres, list):
            for i in plan.fired("lowres"):
                x[i, 0].copy_(simulate_low_resolution(x[i, 0], plan.lowres[i], plan.thin))
        else:
            before = [x[i] for i in range(plan.batch_size)]
            data = list(before)
            plan.lowres(data=data)
            for i in range(plan.batch_size):
                if data[i] is not before[i]:
                    x[i].copy_(data[i])
        for stage, negate in (("gamma_inverted", True), ("gamma", False)):
            for idx in chunks(plan.fired(stage)):
                g = [getattr(plan, stage)[i] for i in idx]
                before = ops.intensity_stats(x, idx)
                ops.intensity_map(x, idx, "gamma", a=g, negate=negate, stats=before)
                ops.intensity_map(x, idx, "restore", negate=negate, stats=before, stats2=ops.intensity_stats(x, idx))
        return x
