"""Times of the connected-component post-processing (csrc/components.hip): cc_label, cc_sizes and cc_filter at connectivity 26 on
256^3 and 512^3, device events, warmed up, median.  Inputs: the ellipsoid anatomy of dg_tta_amd/synthetic.py (atlas_layout, 15
structures painted in order, plus 200 stray voxels per structure for the filter to remove) and uniform noise at p = 0.31, the
adversarial case near the percolation threshold.  Where scipy is importable, scipy.ndimage.label over the same labels (one call per
label, as a post-processing hook on the host does it) stands beside it.

usage: python profiles/tools/ccbench.py [--no-host] [sizes ...]      (default: 256 512; --no-host leaves scipy out)"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from dg_tta_amd import ops                       # noqa: E402
from dg_tta_amd.synthetic import atlas_layout    # noqa: E402

DEV = "cuda:0"
K, REPS, WARMUP = 15, 9, 2


def ellipsoids(s):
    centres, radii, _ = atlas_layout(K)
    ax = (torch.arange(s, dtype=torch.float32, device=DEV) + 0.5) / s
    lab = torch.zeros(s, s, s, dtype=torch.int64, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    for i in range(K):
        c, r = centres[i].tolist(), radii[i].tolist()
        lab[(((ax[:, None, None] - c[0]) / r[0]) ** 2 + ((ax[None, :, None] - c[1]) / r[1]) ** 2 +
             ((ax[None, None, :] - c[2]) / r[2]) ** 2) <= 1.0] = i + 1
        lab.view(-1)[torch.randint(0, s ** 3, (200,), device=DEV, generator=g)] = i + 1
    return lab


def noise(s):
    g = torch.Generator(device=DEV).manual_seed(31)
    return (torch.rand(s, s, s, device=DEV, generator=g) < 0.31).long()


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


def scipy_seconds(lab, nlab):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    a = lab.cpu().numpy()
    t0 = time.perf_counter()
    st = ndimage.generate_binary_structure(3, 3)
    for l in range(1, nlab + 1):
        ndimage.label(a == l, structure=st)
    return time.perf_counter() - t0


def main():
    host_wanted = "--no-host" not in sys.argv[1:]
    sizes = [int(v) for v in sys.argv[1:] if v != "--no-host"] or [256, 512]
    print(f"device {torch.cuda.get_device_name(0)}", flush=True)
    for s in sizes:
        for name, lab, nlab in (("ellipsoids", ellipsoids(s), K), ("noise0.31", noise(s), 1)):
            table = torch.arange(nlab + 1, dtype=torch.int32, device=DEV)
            n = s ** 3
            cc = torch.empty(n, dtype=torch.int32, device=DEV)
            size = torch.empty(n, dtype=torch.int32, device=DEV)
            out = torch.empty(n, dtype=torch.int64, device=DEV)
            ws = torch.empty(ops.cc_ws_bytes(s, s, s), dtype=torch.uint8, device=DEV)
            t_label = median_ms(lambda: ops.cc_label(lab, table, 26, out=cc, ws=ws))
            ccv = cc.view(s, s, s)
            t_sizes = median_ms(lambda: ops.cc_sizes(ccv, out=size))
            t_filter = median_ms(lambda: ops.cc_filter(lab, table, ccv, size, out=out, ws=ws))
            _, removed = ops.cc_filter(lab, table, ccv, size, out=out, ws=ws)
            ncomp = int(torch.count_nonzero(size))
            host = scipy_seconds(lab, nlab) if host_wanted else None
            print(f"{s}^3 {name}: cc_label {t_label:.3f} ms, cc_sizes {t_sizes:.3f} ms, cc_filter {t_filter:.3f} ms, "
                  f"{ncomp} components, {int(removed.sum())} voxels removed"
                  + (f", scipy.ndimage.label x {nlab}: {host:.2f} s" if host is not None else ", no scipy time"), flush=True)
            del lab, cc, size, out, ws


if __name__ == "__main__":
    main()
