"""Time of nnU-Net's optimiser step on the full 3d_fullres parameter set (HipPlainConvUNet(): 16.6 M parameters), same
tensors, same GPU:
  * ops.grad_sumsq + ops.sgd_step (csrc/sgd.hip): the norm pass and the fused clip + Nesterov update, called as
    optim.HipSGD.step calls them (the Python of the step included: pointer tables, ctypes calls);
  * torch.nn.utils.clip_grad_norm_(params, 12, foreach=True) + torch.optim.SGD(lr 1e-2, momentum 0.99, nesterov, weight decay
    3e-5, foreach=True).step().
Gradients ~ N(0, 1): the norm is far above 12, both sides clip.  Both sides are warmed up (momentum buffers exist), then
timed alternately, REPS times each, with device events around one step; the medians and the spread (min .. max) are printed,
and the bytes the HIP step needs by its arithmetic (3 reads + 2 writes + 1 read for the norm, 4 B each) over its median.

usage: python profiles/tools/sgdbench.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from dg_tta_amd import ops                                  # noqa: E402
from dg_tta_amd.unet import HipPlainConvUNet               # noqa: E402

DEV = "cuda:0"
REPS, WARMUP = 50, 5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    print(f"device {torch.cuda.get_device_name(0)}", flush=True)
    g = torch.Generator(device=DEV).manual_seed(3)
    shapes = [tuple(p.shape) for p in HipPlainConvUNet().parameters()]
    n = sum(torch.Size(s).numel() for s in shapes)
    grads = [torch.randn(s, device=DEV, generator=g) for s in shapes]
    p_hip = [torch.randn(s, device=DEV, generator=g) for s in shapes]
    b_hip = [torch.zeros_like(p) for p in p_hip]
    p_torch = [torch.nn.Parameter(p.clone()) for p in p_hip]
    for p, gr in zip(p_torch, grads):
        p.grad = gr.clone()
    tsgd = torch.optim.SGD(p_torch, lr=1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5, foreach=True)
    ws = torch.empty(ops.grad_sumsq_ws_bytes(n, len(grads)), dtype=torch.uint8, device=DEV)
    out = torch.empty((), dtype=torch.float32, device=DEV)

    def hip_step():
        ops.grad_sumsq(grads, out=out, ws=ws)
        ops.sgd_step(p_hip, grads, b_hip, 1e-2, 0.99, 3e-5, True, first_step=False, sumsq=out, max_norm=12.0)

    def torch_step():
        # clip_grad_norm_ scales the gradients in place, so from the second call on their norm is 12; torch multiplies by the
        # clamped coefficient either way: the work of a call is the same
        torch.nn.utils.clip_grad_norm_(p_torch, 12.0, foreach=True)
        tsgd.step()

    t_hip, t_torch = [], []
    for rep in range(WARMUP + REPS):
        a, b = timed(hip_step), timed(torch_step)
        if rep >= WARMUP:
            t_hip.append(a)
            t_torch.append(b)
    t_hip.sort()
    t_torch.sort()
    mh, mt = t_hip[len(t_hip) // 2], t_torch[len(t_torch) // 2]
    nbytes = 6 * 4 * n
    print(f"{len(shapes)} tensors, {n} parameters, {REPS} alternating repetitions", flush=True)
    print(f"grad_sumsq + sgd_step: median {mh:.3f} ms (min {t_hip[0]:.3f}, max {t_hip[-1]:.3f}); {nbytes / 1e9:.3f} GB by the "
          f"arithmetic -> {nbytes / (mh * 1e-3) / 1e12:.2f} TB/s over the whole step, host work included", flush=True)
    print(f"clip_grad_norm_ + torch.optim.SGD(foreach=True): median {mt:.3f} ms (min {t_torch[0]:.3f}, max {t_torch[-1]:.3f})",
          flush=True)
    print(f"ratio torch / hip {mt / mh:.2f}", flush=True)


if __name__ == "__main__":
    main()
