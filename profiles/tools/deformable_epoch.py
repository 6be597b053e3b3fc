"""Cost of spatial_aug_type="deformable": tta_epoch at 128^3 with 16 accumulation steps, fp32 and fp16 storage, once per
augmentation type, and every kernel of csrc/deform.hip beside the affine kernel of the same role on the same shape (time,
algorithmic bytes, achieved bandwidth).  Seeded He weights on the synthetic case: timing only.

    python profiles/tools/deformable_epoch.py [--size 128] [--accum 16] [--epochs 3] > profiles/deformable_epoch.txt"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
from dg_tta_amd import ops  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def row(name, ms, nbytes, beside=None):
    line = f"{name:34s} {ms:8.3f} ms {nbytes / 1e9:7.3f} GB {nbytes / ms / 1e6:8.1f} GB/s"
    if beside is not None:
        b_ms, b_bytes = beside
        line += f"   time x{ms / b_ms:5.2f}  bytes x{nbytes / b_bytes:5.2f} of the affine kernel"
    print(line, flush=True)


def kernels(size, n, c):
    """n = 2 branches x 4 steps x batch 1 samples per pass, c selected classes."""
    v = size ** 3
    low = [size // 5] * 3
    draw = torch.randn(n, 3, *low, device=DEV)
    field = ops.rf_field(draw, [size] * 3)
    disp, inv = ops.diffeo_fields(field, 0.5, 5)
    theta = (torch.eye(3, 4) + 0.05 * torch.randn(n, 3, 4)).to(DEV)
    img = torch.randn(n, 1, size, size, size, device=DEV)
    logits = torch.randn(n, size, size, size, c, device=DEV).permute(0, 4, 1, 2, 3).requires_grad_(True)
    print(f"# kernels at {size}^3, {n} samples per launch, {c} classes; best of 5; bytes = algorithmic (gathers counted once)")
    row("rf_field (3 box + stats + norm)", timed(lambda: ops.rf_field(draw, [size] * 3)), n * 3 * v * 4)
    row("diffeo_fields (5 iterations)", timed(lambda: ops.diffeo_fields(field, 0.5, 5)), n * v * (36 + 4 * 48))
    a = timed(lambda: ops.affine_warp(img, theta, padding_mode="border", tta_grid_algebra=True)), n * v * 8
    row("affine image warp (border)", *a)
    row("dense image warp (border)", timed(lambda: ops.dense_warp(img, disp, "border")), n * v * 20, a)
    a = timed(lambda: ops.affine_warp(logits, theta, padding_mode="zeros", tta_grid_algebra=True)), n * v * 8 * c
    row("affine logits warp (zeros)", *a)
    row("dense logits warp (zeros)", timed(lambda: ops.dense_warp(logits, inv, "zeros")), n * v * (8 * c + 12), a)
    g = torch.randn(n, size, size, size, c, device=DEV).permute(0, 4, 1, 2, 3)
    ya = ops.affine_warp(logits, theta, padding_mode="zeros", tta_grid_algebra=True)
    a = timed(lambda: torch.autograd.grad(ya, logits, g, retain_graph=True)), n * v * 8 * c
    row("affine logits warp backward", *a)
    yd = ops.dense_warp(logits, inv, "zeros")
    row("dense logits warp backward (atomics)", timed(lambda: torch.autograd.grad(yd, logits, g, retain_graph=True)),
        n * v * (8 * c + 12 + 4 * c), a)


def epochs(size, accum, n_epochs):
    print(f"# tta_epoch at {size}^3, {accum} accumulation steps, batch 1: seconds per epoch (first epoch = warm-up, not listed)")
    for dtype in ("fp32", "fp16"):
        res = {}
        for kind in ("affine", "deformable"):
            args = bench.parse_args(["--size", str(size), "--accum", str(accum), "--weights", "he", "--dtype", dtype])
            torch.manual_seed(0)
            torch.cuda.manual_seed(0)
            runner = bench.EpochRunner(args, torch.device(DEV), 0, dtype)
            runner.cfg["spatial_aug_type"] = kind
            times = []
            for e in range(n_epochs + 1):
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                runner.epoch()
                b.record()
                torch.cuda.synchronize()
                times.append(a.elapsed_time(b) / 1e3)
            res[kind] = min(times[1:])
            print(f"{dtype} {kind:10s} epochs {[round(t, 4) for t in times[1:]]} s, losses {[round(l, 4) for l in runner.losses]}",
                  flush=True)
            del runner
            torch.cuda.empty_cache()
        print(f"{dtype}: deformable - affine = {res['deformable'] - res['affine']:+.4f} s per epoch "
              f"(x{res['deformable'] / res['affine']:.3f})", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--accum", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=3)
    a = ap.parse_args()
    kernels(a.size, 8, 16)
    epochs(a.size, a.accum, a.epochs)
