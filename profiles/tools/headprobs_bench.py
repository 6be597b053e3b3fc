"""Fused head + softmax (dgtta_feature_head_softmax) against the head + argmax kernel on the same buffers, timed on a quarter of a
512^3 volume at 105 classes and scaled to the volume: python3 profiles/tools/headprobs_bench.py
Per configuration: 3 warm-up calls, then the median of 9 event-timed calls of each kernel, alternating."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from dg_tta_amd import ops
V = 512 * 512 * 512 // 4
C = 105


def timed(fn, n=9):
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


for M in (1, 3):
    facc = torch.randn(M, 1, 1, V, 32, device="cuda")
    nsum = torch.rand(1, 1, V, device="cuda") + 0.5
    w = torch.randn(M, C, 32, device="cuda")
    b = torch.randn(C, device="cuda")
    arg = lambda: ops.feature_head_argmax(facc, nsum, w, b)
    t_arg = None
    for K, pt in ((1, torch.float16), (16, torch.float16), (16, torch.float32)):
        sel = list(range(0, C, C // K))[:K]
        soft = lambda: ops.feature_head_softmax(facc, nsum, w, b, sel, prob_dtype=pt)
        for _ in range(3):
            arg(), soft()
        torch.cuda.synchronize()
        t_arg, t_soft = timed(arg) * 4, timed(soft) * 4
        extra = 8 + K * (2 if pt == torch.float16 else 4)
        print(f"members {M} K {K} {str(pt).split('.')[-1]}: argmax {t_arg:.2f} ms, softmax {t_soft:.2f} ms per 512^3 volume, ratio "
              f"{t_soft / t_arg:.3f} (+{extra} B per voxel over the argmax's 8 + {128 * M + 4} read)")
    del facc, nsum
