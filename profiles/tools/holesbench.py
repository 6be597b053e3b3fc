"""Times of the hole filling (csrc/components.hip) as the non-zero crop of the preprocessing uses it, on 256^3 and 512^3:
  * the kernels alone: ops.nonzero_mask (one channel) and ops.fill_holes at connectivity 6 with the box, device events, warmed up,
    median;
  * the whole GPU crop, preprocessing.crop_to_nonzero_gpu: upload of the volume, the kernels, download of the box and of the mask
    inside it, the host slicing - wall clock, synchronised, median of three;
  * the host crop on the same machine: scipy.ndimage.binary_fill_holes and the np.where box, one run each.
Inputs: a body-like volume (an ellipsoid of non-zero voxels of which one in ten is zero, in a zero volume) and the volume without
a zero voxel.

usage: python profiles/tools/holesbench.py [--no-host] [sizes ...]      (default: 256 512; --no-host leaves scipy out)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from dg_tta_amd import ops                                  # noqa: E402
from dg_tta_amd.tta import preprocessing                    # noqa: E402

DEV = "cuda:0"
REPS, WARMUP = 9, 2


def body(s):
    ax = (torch.arange(s, dtype=torch.float32, device=DEV) + 0.5) / s - 0.5
    inside = (ax[:, None, None] / 0.45) ** 2 + (ax[None, :, None] / 0.40) ** 2 + (ax[None, None, :] / 0.35) ** 2 <= 1.0
    g = torch.Generator(device=DEV).manual_seed(7)
    return (inside & (torch.rand(s, s, s, device=DEV, generator=g) >= 0.1)).float()[None]


def full(s):
    return torch.ones(1, s, s, s, dtype=torch.float32, device=DEV)


def median_ms(fn):
    times = []
    for rep in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if rep >= WARMUP:
            times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def crop_seconds(data):
    times = []
    for _ in range(4):              # the first one warms the allocator up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        preprocessing.crop_to_nonzero_gpu(data, None, DEV)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return sorted(times[1:])[1]


def host_seconds(data):
    try:
        from scipy.ndimage import binary_fill_holes
    except ImportError:
        return None
    raw = data[0] != 0
    t0 = time.perf_counter()
    mask = binary_fill_holes(raw)
    t1 = time.perf_counter()
    idx = np.where(mask)
    bbox = [[int(np.min(i)), int(np.max(i)) + 1] for i in idx]
    return t1 - t0, time.perf_counter() - t1, bbox


def main():
    host_wanted = "--no-host" not in sys.argv[1:]
    sizes = [int(v) for v in sys.argv[1:] if v != "--no-host"] or [256, 512]
    print(f"device {torch.cuda.get_device_name(0)}", flush=True)
    for s in sizes:
        for name, make in (("body", body), ("all non-zero", full)):
            vol = make(s)
            raw = torch.empty(s, s, s, dtype=torch.uint8, device=DEV)
            out = torch.empty(s ** 3, dtype=torch.uint8, device=DEV)
            ws = torch.empty(ops.holes_ws_bytes(s, s, s), dtype=torch.uint8, device=DEV)
            t_mask = median_ms(lambda: ops.nonzero_mask(vol))
            raw = ops.nonzero_mask(vol)
            t_fill = median_ms(lambda: ops.fill_holes(raw, 6, out=out, ws=ws, return_box=True))
            _, n_filled, box = ops.fill_holes(raw, 6, out=out, ws=ws, return_box=True)
            n_filled, box = int(n_filled), box.cpu().tolist()
            data = vol.cpu().numpy()
            del vol, raw, out, ws
            t_crop = crop_seconds(data)
            print(f"{s}^3 {name}: nonzero_mask {t_mask:.3f} ms, fill_holes {t_fill:.3f} ms, {n_filled} voxels filled, box {box}; "
                  f"crop_to_nonzero_gpu with upload and mask download {1e3 * t_crop:.1f} ms", flush=True)
            host = host_seconds(data) if host_wanted else None
            if host is not None:
                assert host[2] == [[box[k], box[3 + k] + 1] for k in range(3)], (host[2], box)
                print(f"{s}^3 {name}: host binary_fill_holes {host[0]:.2f} s, np.where box {host[1]:.2f} s", flush=True)


if __name__ == "__main__":
    main()
