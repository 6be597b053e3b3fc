"""Stage times of the REGION export in the original geometry: R = 3 outputs, two members, a 192^3 crop of logits exported to 256^3.

Every stage of inference._resampled_class_groups + _RunningRegions is timed on its own with device events, after warm-up, as the
median of 20: the chunk kernel (dgtta_logits_chunk_f64_t, fp32 accumulator), the three linear axis passes (dgtta_resample_axis)
and the merge (dgtta_regions_merge_f64) without probability planes, with fp16 planes and with fp32 planes.  Beside each time stand
the bytes the stage has to move - computed here from the shapes, reads + writes, nothing counted twice - and bytes / time.  The
numbers are measurements of one run; no ratio to anything is claimed.  Reads nothing outside the repository.

    python profiles/tools/regionexportbench.py [crop] [target] > profiles/regionexportbench.txt"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from dg_tta_amd import _lib, ops      # noqa: E402
from dg_tta_amd._lib import check, ptr, stream_of      # noqa: E402

DEV = "cuda:0"
R, M, ORDER = 3, 2, [1, 3, 2]
WARMUP, REPS = 5, 20


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(times), min(times), max(times)


def report(name, nbytes, fn):
    med, lo, hi = timed(fn)
    print(f"{name:<34s} {nbytes / 1e6:10.1f} MB  median {med * 1e3:8.3f} ms  (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  "
          f"{nbytes / med / 1e9:8.1f} GB/s", flush=True)
    return med


def main():
    if not torch.cuda.is_available():
        raise SystemExit("regionexportbench: no GPU - nothing is measured without one")
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 192
    m = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    lib = _lib.load()
    st = stream_of(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    acc = torch.randn(n, n, n, R, device=DEV, generator=g) * (2.0 * M)
    nsum = torch.rand(n, n, n, device=DEV, generator=g) + 0.5
    print(f"region export: R = {R}, {M} members, crop {n}^3 -> {m}^3, fp32 logits accumulator, {torch.cuda.get_device_name(0)}")
    print(f"median of {REPS} after {WARMUP} warm-up calls, device events; bytes = reads + writes the stage needs, from the shapes")

    cur = torch.empty((n, n, n, R), dtype=torch.float64, device=DEV)
    total = 0.0
    total += report("chunk (fp32 acc / nsum -> f64)", n ** 3 * (4 * R + 4 + 8 * R),
                    lambda: check(lib.dgtta_logits_chunk_f64_t(ptr(acc), ptr(nsum), ptr(cur), R, n, n, n, 0, 0, 0, n, n, n, 0, R, ops.F32, st),
                                  "dgtta_logits_chunk_f64_t"))
    shp = [n, n, n]
    for ax in range(3):
        outer = 1
        for s in shp[:ax]:
            outer *= s
        inner = R
        for s in shp[ax + 1:]:
            inner *= s
        dst = torch.empty((*shp[:ax], m, *shp[ax + 1:], R), dtype=torch.float64, device=DEV)
        src = cur
        total += report(f"axis pass {ax} ({shp[ax]} -> {m}, linear)", 8 * outer * inner * (shp[ax] + m),
                        lambda: check(lib.dgtta_resample_axis(ptr(src), ptr(dst), None, 0, outer, n, m, inner, 1, st), "dgtta_resample_axis"))
        cur, shp[ax] = dst, m
    V = m ** 3
    order = (ctypes.c_int * R)(*ORDER)
    label = torch.empty(V, dtype=torch.int32, device=DEV)
    med_label = report("merge, labels only", V * (8 * R + 4),
                       lambda: check(lib.dgtta_regions_merge_f64(ptr(cur), V, R, 0, 1.0 / M, order, R, ptr(label), None, 0, 1, st),
                                     "dgtta_regions_merge_f64"))
    for tdt, size in ((torch.float16, 2), (torch.float32, 4)):
        planes = torch.empty((R, V), dtype=tdt, device=DEV)
        report(f"merge, labels + {str(tdt).split('.')[1]} planes", V * (8 * R + 4 + size * R),
               lambda: check(lib.dgtta_regions_merge_f64(ptr(cur), V, R, 0, 1.0 / M, order, R, ptr(label), ptr(planes),
                                                         ops.prob_dtype_code(tdt), 1, st), "dgtta_regions_merge_f64"))
    print(f"sum of the medians, chunk + three passes + label merge: {(total + med_label) * 1e3:.3f} ms; labels present "
          f"{sorted(torch.unique(label[::97]).tolist())}")


if __name__ == "__main__":
    main()
