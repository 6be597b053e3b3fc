"""What the region kernels cost: python3 profiles/tools/regionlossbench.py [reps] [out file]

At 2 x 128^3 voxels, R = 3 nested regions (whole = [1, 2, 3], core = [2, 3], centre = 3), device events, median of `reps`
(default 20) after a warm-up of both sides, the two sides alternating:
(a) ops.region_loss forward + backward (csrc/region_loss.hip: label map + membership table, no target tensor) against the same
    step written with torch operations - the region target [B, R, D, H, W] built from the label map, then
    binary_cross_entropy_with_logits + the Dice formula + autograd;
(b) the region label map of a logits-space accumulator [128^3, 3] (ops.logits_regions, csrc/region_map.hip) against the torch
    loop seg[acc[..., i] > 0] = order[i], and of feature-space accumulators of one member (ops.feature_head_regions,
    csrc/window_features.hip) against matmul + the same loop;
(c) ops.region_counts against the torch masks.
The results of both sides are compared before anything is timed.  Fails without a GPU.  Numbers: profiles/regionlossbench.txt."""
import pathlib
import statistics
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
import torch

from dg_tta_amd import ops
from dg_tta_amd.labels import membership_table

args = sys.argv[1:]
reps = int(args[0]) if args and args[0].isdigit() else 20
out_file = next((a for a in args if not a.isdigit()), None)
if not torch.cuda.is_available():
    raise SystemExit("regionlossbench: no GPU - nothing is measured on a CPU")
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def event_pair(fa, fb, reps=reps, warm=3):
    """Median / min / max milliseconds of fa and fb, alternating."""
    for _ in range(warm):
        fa(), fb()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
    return tuple((statistics.median(t), min(t), max(t)) for t in (ta, tb))


def fmt(t):
    return f"median {t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


B, R, N = 2, 3, 128
regions, order = ((1, 2, 3), (2, 3), (3,)), [1, 2, 3]
table = ops.region_table(membership_table(regions), dev)
g = torch.Generator(device=dev).manual_seed(5)
logits = (torch.randn(B, R, N, N, N, device=dev, generator=g) * 3).contiguous(memory_format=torch.channels_last_3d)
labels = torch.randint(0, 4, (B, N, N, N), device=dev, generator=g)
say(f"{torch.cuda.get_device_name(0)}; {B} x {N}^3 voxels, R = {R}, {reps} reps, device events")


# ---- (a) loss forward + backward
def hip_step():
    x = logits.detach().requires_grad_(True)
    loss, _, _ = ops.region_loss(x, labels, table)
    loss.backward()
    return loss.detach(), x.grad


def torch_step(smooth=1e-5):
    x = logits.detach().requires_grad_(True)
    target = torch.stack([torch.isin(labels, torch.tensor(r, device=dev)) for r in regions], dim=1).float()
    bce = torch.nn.functional.binary_cross_entropy_with_logits(x, target)
    s = torch.sigmoid(x)
    inter, ps, ts = (s * target).sum((2, 3, 4)), s.sum((2, 3, 4)), target.sum((2, 3, 4))
    loss = bce - ((2 * inter + smooth) / torch.clip(ps + ts + smooth, 1e-8)).mean()
    loss.backward()
    return loss.detach(), x.grad


(lh, gh), (lt, gt) = hip_step(), torch_step()
say(f"(a) loss: HIP {float(lh):.7f}, torch {float(lt):.7f}; largest gradient difference {float((gh - gt).abs().max()):.3e} "
    f"(largest gradient {float(gt.abs().max()):.3e})")
assert abs(float(lh) - float(lt)) < 1e-4 and float((gh - gt).abs().max()) < 1e-3 * float(gt.abs().max())
th, tt = event_pair(hip_step, torch_step)
say(f"    ops.region_loss fwd + bwd          {fmt(th)}")
say(f"    torch target + BCE + Dice + autograd {fmt(tt)}")
del gh, gt

# ---- (b) label maps
acc = (torch.randn(N, N, N, R, device=dev, generator=g) * 3).contiguous()


def torch_map(a):
    seg = torch.zeros(a.shape[:-1], dtype=torch.int64, device=dev)
    for i, lab in enumerate(order):
        seg[a[..., i] > 0] = lab
    return seg


assert torch.equal(ops.logits_regions(acc, order), torch_map(acc))
th, tt = event_pair(lambda: ops.logits_regions(acc, order), lambda: torch_map(acc))
say(f"(b) ops.logits_regions, {N}^3 x {R}       {fmt(th)}")
say(f"    torch loop over the order          {fmt(tt)}")
facc = torch.randn(1, N, N, N, 32, device=dev, generator=g)
nsum = torch.rand(N, N, N, device=dev, generator=g) + 0.5
w, bsum = torch.randn(1, R, 32, device=dev, generator=g), torch.randn(R, device=dev, generator=g)


def torch_feature_map():
    return torch_map(facc[0].reshape(-1, 32).matmul(w[0].t()).reshape(N, N, N, R) + nsum[..., None] * bsum)


a, b = ops.feature_head_regions(facc, nsum, w, bsum, order), torch_feature_map()
say(f"    feature space: the two maps differ in {float((a != b).float().mean()):.2e} of the voxels (sums re-associated)")
assert float((a != b).float().mean()) < 1e-4
th, tt = event_pair(lambda: ops.feature_head_regions(facc, nsum, w, bsum, order), torch_feature_map)
say(f"    ops.feature_head_regions, 1 member {fmt(th)}")
say(f"    torch matmul + loop                {fmt(tt)}")
del facc, nsum, acc


# ---- (c) counts
def torch_counts():
    target = torch.stack([torch.isin(labels, torch.tensor(r, device=dev)) for r in regions], dim=1)
    pred = logits > 0
    return torch.stack([(pred & target).sum((0, 2, 3, 4)), (pred & ~target).sum((0, 2, 3, 4)), (~pred & target).sum((0, 2, 3, 4))])


assert torch.equal(ops.region_counts(logits, labels, table), torch_counts())
th, tt = event_pair(lambda: ops.region_counts(logits, labels, table), torch_counts)
say(f"(c) ops.region_counts                  {fmt(th)}")
say(f"    torch masks                        {fmt(tt)}")
if out_file:
    pathlib.Path(out_file).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out_file).write_text("\n".join(lines) + "\n")
