"""Time of the spatial augmentation of `dgtta pretrain --augmentation spatial` (csrc/spatial_aug.hip), one GPU:
  * ops.bspline3_prefilter of a 256^3 case (once per case; 3 passes, each reads and writes the volume once: 6 x 4 B per voxel
    by the arithmetic);
  * ONE ops.sample_patches_aug launch for 2 x 128^3 patches out of that case (order 3: 64 coefficient taps + 8 label corners
    per voxel), through a rotation (17, -23, 9 degrees) scaled by 1.2 and 0.8;
  * the same 2 x 128^3 patches the way the trainer cuts them without the augmentation: per item get_batch(..., centers=), that is
    two ops.affine_sample launches (trilinear image, nearest labels) plus .long().
All three as the trainer calls them, their Python included (descriptor tables, ctypes calls, the theta upload of get_batch).
Warmed up, then timed alternately REPS times with device events; medians and the spread (min .. max) are printed.

usage: python profiles/tools/spatialbench.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from dg_tta_amd import ops                                                          # noqa: E402
from dg_tta_amd.pretraining.spatial import patch_start, rotation_matrix, sampling_map   # noqa: E402
from dg_tta_amd.tta.torch_utils import _resident, as_label_map_case, get_batch, release_resident, resident_spline   # noqa: E402

DEV = "cuda:0"
REPS, WARMUP = 30, 5
SIZE, PATCH = 256, [128, 128, 128]


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


def main():
    print(f"device {torch.cuda.get_device_name(0)}", flush=True)
    g = torch.Generator().manual_seed(3)
    case = as_label_map_case(torch.randn(SIZE, SIZE, SIZE, generator=g), torch.randint(0, 5, (SIZE, SIZE, SIZE), generator=g))
    dev = torch.device(DEV)
    img, _, lab = _resident(case, dev)
    coef = resident_spline(case, dev)
    centers = [(128, 128, 128), (100, 140, 120)]
    rot = rotation_matrix(*np.radians([17.0, -23.0, 9.0]))
    maps = [sampling_map(f * rot, patch_start(c, (SIZE,) * 3, PATCH), PATCH) for f, c in zip((1.2, 0.8), centers)]

    def prefilter():
        ops.bspline3_prefilter(img)

    def sample():
        ops.sample_patches_aug([coef, coef], [lab, lab], maps, PATCH, order=3)

    def crop():
        for c in centers:
            get_batch([case], [0], PATCH, None, DEV, centers=[c])

    t = {"prefilter": [], "sample": [], "crop": []}
    for rep in range(WARMUP + REPS):
        for name, fn in (("prefilter", prefilter), ("sample", sample), ("crop", crop)):
            ms = timed(fn)
            if rep >= WARMUP:
                t[name].append(ms)
    nbytes = 6 * 4 * SIZE ** 3
    mp = sorted(t["prefilter"])[REPS // 2]
    line(f"bspline3_prefilter {SIZE}^3", t["prefilter"], f"; {nbytes / 1e9:.3f} GB by the arithmetic -> {nbytes / (mp * 1e-3) / 1e12:.2f} TB/s")
    ms = line("sample_patches_aug 2 x 128^3, order 3, one launch", t["sample"])
    mc = line("get_batch(centers=) 2 x 128^3: 2 x (2 affine_sample + .long())", t["crop"])
    print(f"ratio sample / crop {ms / mc:.2f}", flush=True)
    release_resident()


if __name__ == "__main__":
    main()
