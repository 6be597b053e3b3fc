"""Per-layer table of an ANISOTROPIC plan (what nnU-Net 2.2.1 writes for coarse-slice data): patch 40 x 160 x 160, features 32 64
128 256 320, pools [1,1,1] [1,2,2] [1,2,2] [2,2,2] [2,2,2], kernels [1,3,3] [1,3,3] [3,3,3] [3,3,3] [3,3,3], 8 samples per launch
as in the bench.  For every conv that runs on the anisotropic kernels (dgtta_conv3d_fwd / _dgrad / _wgrad) it times forward (with
fused statistics), data gradient and weight gradient, and the same layer EMULATED on the k3 entry points: 27-tap weights with the
missing taps zero, stride 1, on the full input extent (a strided layer's output would then be subsampled).  TFLOP/s count the
layer's useful work (2 * B * Vout * Cin * Cout * kd * 9) in both columns, so the ratio is the speed-up.  Then TTA epochs/s of the
plan (16 accumulation steps, GIN + affine + MIND, both branches) through the product's tta_epoch in fp16 and fp32 storage.
usage: aniso_layerbench.py [fp16|bf16] [batch]      (ALB_EPOCHS=0: no epoch timing)"""
import os, sys, time
from types import SimpleNamespace
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from dg_tta_amd import _lib
from dg_tta_amd._lib import check, ptr, stream_of
lib = _lib.load()
dts = sys.argv[1] if len(sys.argv) > 1 else "fp16"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 8
dt = {"bf16": 1, "fp16": 2}[dts]
tdt = {1: torch.bfloat16, 2: torch.float16}[dt]
DEV = "cuda:0"
PATCH = (40, 160, 160)
CFG = dict(features=(32, 64, 128, 256, 320), strides=((1, 1, 1), (1, 2, 2), (1, 2, 2), (2, 2, 2), (2, 2, 2)),
           kernel_sizes=((1, 3, 3), (1, 3, 3), (3, 3, 3), (3, 3, 3), (3, 3, 3)), n_conv_enc=(2, 2, 2, 2, 2), n_conv_dec=(2, 2, 2, 2),
           in_channels=12, num_classes=105)
# (name, cin, cout, input extent, kd, stride) of the convs the anisotropic kernels take (the 3x3x3 layers with isotropic strides run
# the k3 kernels: see layerbench.py)
LAYERS = [("enc0.0", 12, 32, (40, 160, 160), 1, (1, 1, 1)), ("enc0.1", 32, 32, (40, 160, 160), 1, (1, 1, 1)),
          ("enc1.0", 32, 64, (40, 160, 160), 1, (1, 2, 2)), ("enc1.1", 64, 64, (40, 80, 80), 1, (1, 1, 1)),
          ("enc2.0", 64, 128, (40, 80, 80), 3, (1, 2, 2)),
          ("dec2.0", 128, 64, (40, 80, 80), 1, (1, 1, 1)), ("dec2.1", 64, 64, (40, 80, 80), 1, (1, 1, 1)),
          ("dec3.0", 64, 32, (40, 160, 160), 1, (1, 1, 1)), ("dec3.1", 32, 32, (40, 160, 160), 1, (1, 1, 1))]


def timed(run, budget_ms=150.0):
    run(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); run(); e1.record(); torch.cuda.synchronize()
    n = max(3, min(400, int(budget_ms / max(e0.elapsed_time(e1), 1e-3))))
    for _ in range(n): run()            # warm clocks
    e0.record()
    for _ in range(n): run()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def pad(c):
    return (c + 15) // 16 * 16


def layer_table():
    st_ = stream_of()
    print(f"{dts}, batch {B}, patch {PATCH[0]}x{PATCH[1]}x{PATCH[2]}: useful TFLOP/s, new kernel / k3 emulation (speed-up)")
    print(f"{'layer':7s} {'shape':>30s} {'GFLOP':>7s} | {'fwd new':>8s} {'emul':>6s} {'x':>5s} | {'dgrad new':>9s} {'emul':>6s} {'x':>5s} | "
          f"{'wgrad new':>9s} {'emul':>6s} {'x':>5s}")
    worst = {}
    for name, cin, cout, (D, H, W), kd, s in LAYERS:
        cinp, coutp = pad(cin), pad(cout)
        Do, Ho, Wo = (D - 1) // s[0] + 1, (H - 1) // s[1] + 1, (W - 1) // s[2] + 1
        x = torch.randn(B, D, H, W, cinp, device=DEV).to(tdt)
        x[..., cin:] = 0
        w = torch.randn(cout, cin, kd, 3, 3, device=DEV) * 0.05
        w27 = torch.zeros(cout, cin, 3, 3, 3, device=DEV)          # the emulation's zero-padded 27-tap weights
        w27[:, :, 1 - kd // 2:2 + kd // 2] = w
        kp = torch.empty(lib.dgtta_conv3d_kpacked_bytes(kd, cinp, coutp, dt), dtype=torch.uint8, device=DEV)
        check(lib.dgtta_conv3d_kpack_weights(ptr(w), ptr(kp), kd, 3, 3, cin, cout, cinp, coutp, dt, st_), "kpack")
        ep = torch.empty(lib.dgtta_conv3d_packed_bytes(cinp, coutp, dt), dtype=torch.uint8, device=DEV)
        check(lib.dgtta_conv3d_pack_weights(ptr(w27), ptr(ep), cin, cout, cinp, coutp, dt, st_), "pack")
        y = torch.empty((B, Do, Ho, Wo, cout), dtype=tdt, device=DEV)
        yf = torch.empty((B, D, H, W, cout), dtype=tdt, device=DEV)            # emulation: full extent
        sn = torch.zeros(lib.dgtta_conv3d_stats_bytes(B, cout, Do, Ho, Wo), dtype=torch.uint8, device=DEV)
        sf = torch.zeros(lib.dgtta_conv3d_stats_bytes(B, cout, D, H, W), dtype=torch.uint8, device=DEV)
        dy = torch.randn(B, Do, Ho, Wo, cout, device=DEV).to(tdt)
        dyf = torch.randn(B, D, H, W, cout, device=DEV).to(tdt)
        dx = torch.empty((B, D, H, W, cinp), dtype=tdt, device=DEV)
        dw = torch.empty((cout, cin, kd, 3, 3), device=DEV)
        dw27 = torch.empty((cout, cin, 3, 3, 3), device=DEV)
        nbn = lib.dgtta_conv3d_kwgrad_ws_bytes(B, cin, cout, D, H, W, kd, *s)
        nbe = lib.dgtta_conv3d_wgrad_ws_bytes(B, cin, cout, D, H, W)
        ws = torch.empty(max(nbn, nbe, 256), dtype=torch.uint8, device=DEV)
        gf = B * 2 * 9 * kd * cin * cout * Do * Ho * Wo / 1e9
        t = {}
        t["fwd", 0] = timed(lambda: check(lib.dgtta_conv3d_fwd(ptr(x), cinp, ptr(kp), None, ptr(y), cout, ptr(sn), B, cin, cout, cinp, coutp,
                                                               D, H, W, kd, *s, dt, st_), "fwd"))
        t["fwd", 1] = timed(lambda: check(lib.dgtta_conv3d_k3_fwd(ptr(x), cinp, ptr(ep), None, ptr(yf), cout, ptr(sf), B, cin, cout, cinp,
                                                                  coutp, D, H, W, 1, dt, 0, st_), "k3 fwd"))
        if name != "enc0.0":      # (the first layer's input has no gradient)
            t["dgrad", 0] = timed(lambda: check(lib.dgtta_conv3d_dgrad(ptr(dy), cout, ptr(kp), ptr(dx), cinp, B, cin, cout, cinp, coutp,
                                                                       D, H, W, kd, *s, 0, dt, st_), "dgrad"))
            t["dgrad", 1] = timed(lambda: check(lib.dgtta_conv3d_k3_dgrad(ptr(dyf), cout, ptr(ep), ptr(dx), cinp, B, cin, cout, cinp, coutp,
                                                                          D, H, W, 1, 0, dt, 0, st_), "k3 dgrad"))
        t["wgrad", 0] = timed(lambda: check(lib.dgtta_conv3d_wgrad(ptr(x), cinp, ptr(dy), cout, ptr(dw), None, ptr(ws), ws.numel(), B, cin,
                                                                   cout, D, H, W, kd, *s, 0, dt, st_), "wgrad"))
        t["wgrad", 1] = timed(lambda: check(lib.dgtta_conv3d_k3_wgrad(ptr(x), cinp, ptr(dyf), cout, ptr(dw27), None, ptr(ws), ws.numel(), B,
                                                                      cin, cout, D, H, W, 1, 0, dt, 0, st_), "k3 wgrad"))
        cols = []
        for k in ("fwd", "dgrad", "wgrad"):
            if (k, 0) not in t:
                cols.append(f"{'-':>8s} {'-':>6s} {'-':>5s}")
                continue
            a, b = gf / t[k, 0], gf / t[k, 1]
            worst[k] = min(worst.get(k, 1e9), t[k, 1] / t[k, 0])
            cols.append(f"{a:8.0f} {b:6.0f} {t[k, 1] / t[k, 0]:5.2f}")
        print(f"{name:7s} {f'{cin}->{cout} k{kd}33 s{s} @{D}x{H}x{W}':>30s} {gf:7.1f} | " + " | ".join(cols), flush=True)
        del x, y, yf, dy, dyf, dx, dw, dw27, ws, sn, sf, kp, ep
        torch.cuda.empty_cache()
    print("smallest speed-up over the emulation: " + ", ".join(f"{k} {v:.2f}x" for k, v in worst.items()), flush=True)


def epochs_per_s(storage, epochs=3):
    from dg_tta_amd.gin import gin_hook
    from dg_tta_amd.mind import mind_hook
    from dg_tta_amd.optim import HipAdamW
    from dg_tta_amd.synthetic import he_init_, synthetic_case, synthetic_label_mapping
    from dg_tta_amd.tta.config_log_utils import ModifierFunctions, TEMPLATE_PLAN
    from dg_tta_amd.tta.model_utils import get_model_from_network
    from dg_tta_amd.tta.tta import _fuse_head_if_possible, tta_epoch
    from dg_tta_amd.tta.torch_utils import fix_all, release_all
    from dg_tta_amd.unet import HipPlainConvUNet
    from dg_tta_amd.utils import disable_internal_augmentation
    act = {"fp32": torch.float32, "fp16": torch.float16}[storage]
    net = he_init_(HipPlainConvUNet(CFG, act_dtype=act), seed=7)
    net.exact_zero_bias_grad = True
    net.accumulate_grads_in_place = True
    net.register_forward_pre_hook(gin_hook)
    net.register_forward_pre_hook(mind_hook)
    net = net.to(DEV)
    mapping, names = synthetic_label_mapping(15)
    cfg = dict(TEMPLATE_PLAN)
    cfg.update(do_intensity_aug_in="both", do_spatial_aug_in="both", patches_to_be_accumulated=16, optimized_labels=names,
               epochs=10 ** 6, ensemble_count=1, lr=1e-4)
    modmod = SimpleNamespace(ModifierFunctions=ModifierFunctions)
    data = [synthetic_case(size=192, k=15, seed=20240704)]
    model = get_model_from_network(net, modmod, None)
    fused = _fuse_head_if_possible(model, modmod, mapping, cfg["optimized_labels"])
    opt = HipAdamW(model.parameters(), lr=cfg["lr"], grad_scale=model.loss_scale)
    disable_internal_augmentation()
    model.apply(fix_all)
    model.apply(release_all)
    run = lambda: tta_epoch(model, opt, cfg, data, list(PATCH), mapping, modmod, DEV, fused, adapt=True)
    run(); torch.cuda.synchronize()           # warm-up epoch (packing, allocator)
    t0 = time.perf_counter()
    for _ in range(epochs):
        loss, dice = run()
    torch.cuda.synchronize()
    rate = epochs / (time.perf_counter() - t0)
    print(f"TTA epochs/s, {storage} storage, patch {PATCH[0]}x{PATCH[1]}x{PATCH[2]}, 16 steps: {rate:.3f} (last loss {loss:.4f})", flush=True)


if __name__ == "__main__":
    layer_table()
    if os.environ.get("ALB_EPOCHS", "1") != "0":
        for storage in ("fp16", "fp32"):
            epochs_per_s(storage)
