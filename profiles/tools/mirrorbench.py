"""What mirroring costs: python3 profiles/tools/mirrorbench.py [fp16|bf16] [size] [reps]

(a) predict_ensemble of one member of the full 3d_fullres net (one image channel, 16-bit storage) on a size^3 volume (default
    256: 27 windows of 128^3) with mirror_axes=(0, 1, 2) against EIGHT unmirrored calls of the same build, alternating, median of
    `reps` (default 5) after a warm-up of both;
(b) the pieces mirroring adds, alone, with device events (median of 20): ops.window_gather of 16 mirrored windows against
    torch.stack of 16 slices, one mirrored against one unmirrored feature accumulation of a 128^3 window;
(c) one ops.mirror_batch launch on a 2 x 1 x 128^3 training batch against torch.flip of image and labels.
Numbers: profiles/mirrorbench.txt."""
import pathlib
import statistics
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
import torch

from dg_tta_amd import _lib, ops
from dg_tta_amd.synthetic import he_init_
from dg_tta_amd.tta.inference import compute_gaussian, predict_ensemble
from dg_tta_amd.unet import PLANS_3D_FULLRES, HipPlainConvUNet

args = sys.argv[1:]
adt = torch.bfloat16 if "bf16" in args else torch.float16
nums = [int(a) for a in args if a.isdigit()]
n = nums[0] if nums else 256
reps = nums[1] if len(nums) > 1 else 5
dev = torch.device("cuda:0")
patch = [128] * 3


def host_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def event_time(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


# ---- (a) a mirrored member against eight unmirrored ones
net = he_init_(HipPlainConvUNet(dict(PLANS_3D_FULLRES, in_channels=1), act_dtype=adt), seed=7).to(dev)
params = [net.state_dict()]
vol = torch.randn(1, n, n, n, generator=torch.Generator().manual_seed(3)).to(dev)
mirrored = lambda: predict_ensemble(vol, net, params, patch, mirror_axes=(0, 1, 2))
plain8 = lambda: [predict_ensemble(vol, net, params, patch) for _ in range(8)]
mirrored(), plain8()                                          # warm-up of every shape both sides use
tm, tp = [], []
for _ in range(reps):                                         # alternating: both sides see the same machine
    tm.append(host_time(mirrored))
    tp.append(host_time(plain8))
windows = (2 * (n - 128) // 128 + 1) ** 3 if n > 128 else 1
print(f"{adt}, {n}^3, {windows} windows, {reps} reps")
print(f"(a) mirrored member   median {statistics.median(tm):.4f} s  (min {min(tm):.4f}, max {max(tm):.4f})")
print(f"    8 x unmirrored    median {statistics.median(tp):.4f} s  (min {min(tp):.4f}, max {max(tp):.4f})")
print(f"    ratio mirrored / (8 x unmirrored) = {statistics.median(tm) / statistics.median(tp):.3f}")
del vol

# ---- (b) the pieces
sub = torch.randn(1, 256, 256, 256, device=dev)
origins = [(64 * (i % 3), 64 * ((i // 3) % 3), 64 * (i % 2)) for i in range(16)]
masks = [i % 8 for i in range(16)]
g = ops.window_gather(sub, origins, masks, patch)
t_g = event_time(lambda: ops.window_gather(sub, origins, masks, patch))
t_s = event_time(lambda: torch.stack([sub[:, x:x + 128, y:y + 128, z:z + 128] for x, y, z in origins]).contiguous())
print(f"(b) window_gather, 16 mirrored windows   median {t_g[0]:.3f} ms (min {t_g[1]:.3f}, max {t_g[2]:.3f}); "
      f"torch.stack of 16 slices {t_s[0]:.3f} ms (min {t_s[1]:.3f}, max {t_s[2]:.3f})")
lib = _lib.load()
gauss = compute_gaussian(tuple(patch)).to(dev)
z = torch.randn(128, 128, 128, 32, device=dev).to(adt)
facc, nsum = torch.zeros(256, 256, 256, 32, device=dev), torch.zeros(256, 256, 256, device=dev)
code = ops.dtype_code(adt)
st = _lib.stream_of(dev)
for mask in (0, 1, 4, 7):
    t = event_time(lambda: _lib.check(lib.dgtta_feature_window_accumulate_mirror(z.data_ptr(), gauss.data_ptr(), facc.data_ptr(), nsum.data_ptr(),
                                                                                  32, 128, 128, 128, 256, 256, 256, 64, 64, 64, code, mask, st), "acc"))
    print(f"    feature accumulate of one 128^3 window, mask {mask}: median {t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})")
del sub, g, z, facc, nsum

# ---- (c) the training batch
img = torch.randn(2, 1, 128, 128, 128, device=dev)
lab = torch.randint(0, 105, (2, 128, 128, 128), device=dev)
t_m = event_time(lambda: ops.mirror_batch(img, lab, [5, 7]))
t_f = event_time(lambda: (torch.stack([img[0].flip(1, 3), img[1].flip(1, 2, 3)]), torch.stack([lab[0].flip(0, 2), lab[1].flip(0, 1, 2)])))
print(f"(c) mirror_batch 2 x 128^3 (masks 5, 7)   median {t_m[0]:.3f} ms (min {t_m[1]:.3f}, max {t_m[2]:.3f}); "
      f"torch.flip + stack {t_f[0]:.3f} ms (min {t_f[1]:.3f}, max {t_f[2]:.3f})")
