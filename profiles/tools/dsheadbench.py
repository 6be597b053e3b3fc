"""Micro-bench of the auxiliary (deep supervision) heads through the C ABI at the real plan's shapes: fp16, B = 2, 105 classes,
Cin 64 at 64^3, 128 at 32^3, 256 at 16^3, and of a pre-training step with deep supervision on against off.

  dsheadbench.py heads [iters] [reps]
      forward (dgtta_seghead_fwd) and backward with the accumulating data gradient (dgtta_seghead_bwd_acc) of this tree's library.
  DSHEAD_LIB=<libdgtta_hip.so of the parent commit> dsheadbench.py baseline [iters] [reps]
      the 'before' column: the SAME shapes through the library named by DSHEAD_LIB - dgtta_seghead_fwd, and dgtta_seghead_bwd
      into a temporary plus the add pass (dx += tmp) that an auxiliary head needed without the accumulate flag.  The library is
      opened on its own with only the four symbols used here (dg_tta_amd._lib.load() binds every symbol of the current header,
      which an older library does not have); on a library from before this kernel file these calls take the general VALU kernels.
  dsheadbench.py step [iters] [reps]
      one pre-training step (forward, loss, backward, AdamW) of the isotropic test cfg - features (32, 64, 128), 12 input
      channels, 11 classes, fp16 storage, B = 2 - on a 64^3 patch: dice_ce_loss on the plain net against deep_supervision_loss
      with weights (2/3, 1/3) on the net with deep_supervision on (the default weights of two outputs drop the second).

Medians of `reps` timed groups of `iters` calls after a warm-up of 3 calls."""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from dg_tta_amd import _lib                                   # noqa: E402
from dg_tta_amd._lib import SIGNATURES, ptr, stream_of        # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "heads"
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
DEV, dt, B, ncls = "cuda:0", 2, 2, 105


def timed(run):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ms)


def open_lib(baseline):
    if not baseline:
        return _lib.load()
    lib = ctypes.CDLL(os.environ["DSHEAD_LIB"])          # (torch is imported: the same HIP runtime instance)
    for name in ("dgtta_seghead_fwd", "dgtta_seghead_bwd_ws_bytes", "dgtta_seghead_bwd", "dgtta_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = SIGNATURES[name]
    return lib


def heads(baseline):
    lib = open_lib(baseline)

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed (code {rc}): {lib.dgtta_last_error().decode(errors='replace')}")

    for cin, n in ((64, 64), (128, 32), (256, 16)):
        V = n ** 3
        x = torch.randn(B * V, cin, device=DEV).half()
        w, bias = torch.randn(ncls, cin, device=DEV) * 0.05, torch.randn(ncls, device=DEV)
        out, dout = torch.empty(B * V, ncls, device=DEV), torch.randn(B * V, ncls, device=DEV)
        dx, tmp = torch.randn(B * V, cin, device=DEV).half(), torch.empty(B * V, cin, device=DEV).half()
        dw, db = torch.empty(ncls, cin, device=DEV), torch.empty(ncls, device=DEV)
        nb = lib.dgtta_seghead_bwd_ws_bytes(B, cin, ncls, V)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)

        def fwd():
            ok(lib.dgtta_seghead_fwd(ptr(x), cin, ptr(w), ptr(bias), None, ncls, ptr(out), 1, ncls, B, cin, V, dt, stream_of()), "fwd")
        if baseline:
            def bwd():
                ok(lib.dgtta_seghead_bwd(ptr(x), cin, ptr(dout), ncls, ptr(w), None, ncls, ptr(tmp), cin, ptr(dw), ptr(db), ptr(ws), nb,
                                         B, cin, V, 0, dt, stream_of()), "bwd")
                dx.add_(tmp)
        else:
            def bwd():
                ok(lib.dgtta_seghead_bwd_acc(ptr(x), cin, ptr(dout), ncls, ptr(w), None, ncls, ptr(dx), cin, ptr(dw), ptr(db), ptr(ws),
                                             nb, B, cin, V, 0, 1, dt, stream_of()), "bwd_acc")

        def bwd_dx_only():       # the data gradient alone (no weight / bias gradient): what the accumulate flag changes
            if baseline:
                ok(lib.dgtta_seghead_bwd(ptr(x), cin, ptr(dout), ncls, ptr(w), None, ncls, ptr(tmp), cin, None, None, ptr(ws), nb, B,
                                         cin, V, 0, dt, stream_of()), "bwd")
                dx.add_(tmp)
            else:
                ok(lib.dgtta_seghead_bwd_acc(ptr(x), cin, ptr(dout), ncls, ptr(w), None, ncls, ptr(dx), cin, None, None, ptr(ws), nb, B,
                                             cin, V, 0, 1, dt, stream_of()), "bwd_acc")
        print(f"{'baseline ' if baseline else ''}head fp16 B={B} Cin={cin} {n}^3 ncls={ncls}: fwd {timed(fwd):.3f} ms, "
              f"bwd {timed(bwd):.3f} ms (dx only {timed(bwd_dx_only):.3f} ms)", flush=True)


def step():
    from dg_tta_amd import ops
    from dg_tta_amd.optim import HipAdamW
    from dg_tta_amd.synthetic import he_init_
    from dg_tta_amd.unet import HipPlainConvUNet
    cfg = dict(features=(32, 64, 128), strides=(1, 2, 2), n_conv_enc=(2, 2, 2), n_conv_dec=(2, 2), in_channels=12, num_classes=11)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 12, 64, 64, 64, generator=g).to(DEV)
    labels = torch.randint(0, 11, (B, 64, 64, 64), generator=g).to(DEV)
    res = {}
    for ds in (False, True):
        net = he_init_(HipPlainConvUNet(cfg, act_dtype=torch.float16, deep_supervision=ds), seed=7).to(DEV).train()
        opt = HipAdamW(list(net.parameters()), lr=1e-4, weight_decay=0.0, grad_scale=getattr(net, "loss_scale", 1.0))

        def one():
            opt.resolve_overflow()
            if ds:
                loss, _ = ops.deep_supervision_loss(net(x), labels, weights=(2.0 / 3.0, 1.0 / 3.0))
            else:
                loss, _, _ = ops.dice_ce_loss(net(x), labels)
            torch.autograd.backward(loss, grad_tensors=torch.full((), float(opt.grad_scale), device=DEV))
            opt.step()
            opt.zero_grad(set_to_none=True)
        res[ds] = timed(one)
        print(f"pre-training step fp16 B={B} 64^3 iso test cfg, deep_supervision={ds}: {res[ds]:.3f} ms", flush=True)
    print(f"deep supervision adds {res[True] - res[False]:.3f} ms per step ({100 * (res[True] / res[False] - 1):.1f} %)", flush=True)


if mode == "step":
    step()
else:
    heads(mode == "baseline")
