"""Time of the intensity chain of `dgtta pretrain --augmentation full` (pretraining/intensity.py, csrc/intensity_aug.hip), one
GPU, on a 2 x 128^3 batch with EVERY stage forced on:
  * hip:    IntensityAugmentation.apply as the trainer calls it, its Python included (descriptor tables, ctypes calls, the
            allocations of the statistics and the scratch buffer) - stages 1-4, 6, 7, i.e. the kernels of csrc/intensity_aug.hip:
            20 launches, 108 B per voxel by the arithmetic (map 8 B x 7, stats 4 B x 5, blur 24 B);
  * torch:  the same stages written with torch operations on the same device (randn_like for the noise, three conv3d with
            symmetric padding for the blur, amin / amax / mean / std reductions, pow);
  * stage 5 (simulated low resolution: ops.resize_volume down with order 0 and back with order 3, csrc/resample.hip, in
            double) is the same code on both sides and is timed on its own;
  * the three kernels one by one with their bytes by the arithmetic.
Warmed up WARMUP times, then timed REPS times with the sides alternating, device events around each call with its host work;
medians and the spread (min .. max) are printed.  Not measured here: the chain inside a training step.

usage: python profiles/tools/intensitybench.py"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from dg_tta_amd import ops                                                                         # noqa: E402
from dg_tta_amd.pretraining.intensity import IntensityAugmentation, simulate_low_resolution      # noqa: E402

DEV = "cuda:0"
REPS, WARMUP = 30, 5
B, SIZE = 2, 128
ALL_ON = dict(p_noise=1.0, p_blur=1.0, p_blur_channel=1.0, p_brightness=1.0, p_contrast=1.0, p_lowres=1.0, p_lowres_channel=1.0,
              p_gamma_inverted=1.0, p_gamma=1.0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def line(name, t, extra=""):
    t = sorted(t)
    print(f"{name}: median {t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}){extra}", flush=True)
    return t[len(t) // 2]


def sym_pad(x, r, dim):
    """scipy's "reflect" (d c b a | a b c d | d c b a) along one axis."""
    n = x.shape[dim]
    return torch.cat([x.narrow(dim, 0, r).flip(dim), x, x.narrow(dim, n - r, r).flip(dim)], dim=dim)


def torch_chain(images, plan):
    x = images.clone()
    b = x.shape[0]
    col = lambda v: torch.tensor(v, dtype=torch.float32, device=x.device).view(b, 1, 1, 1, 1)      # noqa: E731
    x = x + col([p[0] for p in plan.noise]) * torch.randn_like(x)
    for i in range(b):
        radius, taps = ops.gauss_blur_taps(plan.blur[i])
        k = torch.from_numpy(taps).to(x.device)
        v = x[i:i + 1]
        for dim, shape in ((2, (1, 1, -1, 1, 1)), (3, (1, 1, 1, -1, 1)), (4, (1, 1, 1, 1, -1))):
            v = F.conv3d(sym_pad(v, radius, dim), k.view(shape))
        x[i:i + 1] = v
    x = x * col(plan.brightness)
    dims = (1, 2, 3, 4)
    mean, lo, hi = x.mean(dims, keepdim=True), x.amin(dims, keepdim=True), x.amax(dims, keepdim=True)
    x = torch.minimum(torch.maximum((x - mean) * col(plan.contrast) + mean, lo), hi)
    for g, negate in ((plan.gamma_inverted, True), (plan.gamma, False)):
        x = -x if negate else x
        mean, sd = x.mean(dims, keepdim=True), x.std(dims, keepdim=True, unbiased=False)
        lo = x.amin(dims, keepdim=True)
        r = x.amax(dims, keepdim=True) - lo
        x = torch.pow((x - lo) / (r + 1e-7), col(g)) * r + lo
        x = (x - x.mean(dims, keepdim=True)) / (x.std(dims, keepdim=True, unbiased=False) + 1e-8) * sd + mean
        x = -x if negate else x
    return x


def main():
    print(f"device {torch.cuda.get_device_name(0)}", flush=True)
    g = torch.Generator().manual_seed(3)
    images = (torch.randn(B, 1, SIZE, SIZE, SIZE, generator=g) * 1.5 + 0.3).to(DEV)
    aug = IntensityAugmentation(**ALL_ON)
    plan = aug.draw(B, (SIZE,) * 3, np.random.RandomState(7))
    zooms, plan.lowres = plan.lowres, [None] * B                      # stage 5 on its own (module docstring)
    idx, v = list(range(B)), SIZE ** 3
    stats = ops.intensity_stats(images, idx)
    work, scratch = images.clone(), torch.empty_like(images)
    sides = (
        ("hip", lambda: aug.apply(images, plan)),
        ("torch", lambda: torch_chain(images, plan)),
        ("lowres", lambda: [simulate_low_resolution(images[i, 0], zooms[i]) for i in range(B)]),
        ("stats", lambda: ops.intensity_stats(images, idx, out=stats)),
        ("map", lambda: ops.intensity_map(images, idx, "gamma", a=plan.gamma, stats=stats, out=work)),
        ("noise", lambda: ops.intensity_map(images, idx, "linear", s=[p[0] for p in plan.noise], keys=[p[1] for p in plan.noise], out=work)),
        ("blur", lambda: ops.gauss_blur3(images, idx, plan.blur, out=work, scratch=scratch)),
    )
    t = {name: [] for name, _ in sides}
    for rep in range(WARMUP + REPS):
        for name, fn in sides:
            ms = timed(fn)
            if rep >= WARMUP:
                t[name].append(ms)

    def rate(name, nbytes):
        m = sorted(t[name])[REPS // 2]
        return f"; {nbytes / 1e6:.1f} MB by the arithmetic -> {nbytes / (m * 1e-3) / 1e12:.2f} TB/s"
    print(f"batch {B} x {SIZE}^3, every stage on: sigma {[round(s, 3) for s in plan.blur]}, zoom {[round(z, 3) for z in zooms]}", flush=True)
    mh = line("hip chain (stages 1-4, 6, 7; 20 launches)", t["hip"], rate("hip", 108 * B * v))
    mt = line("torch chain (the same stages)", t["torch"])
    print(f"ratio torch / hip {mt / mh:.2f}", flush=True)
    line("stage 5, simulate_low_resolution per item (both sides)", t["lowres"])
    line("intensity_stats (2 launches)", t["stats"], rate("stats", 4 * B * v))
    line("intensity_map gamma (1 launch)", t["map"], rate("map", 8 * B * v))
    line("intensity_map noise (1 launch)", t["noise"], rate("noise", 8 * B * v))
    line("gauss_blur3 (3 launches)", t["blur"], rate("blur", 24 * B * v))


if __name__ == "__main__":
    main()
