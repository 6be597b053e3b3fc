"""MIND3D (oracle/mind.py) restated stage by stage, in float64 by default (test infrastructure; licensed by
tests/test_mind_ref.py).

The taps are an argument: the float32 values the kernel receives, cast to the working type.  `rw` is the float32 value the
C ABI receives.  The same functions run in float32 (dtype=torch.float32), one rounding per operation in the order written
here, which is what the exactness licences of the dyadic cases compare with the float64 evaluation bit for bit.

  stages()        ssd, m = ssd - min [B][V][12], var, the global mean, out [B,12,D,H,W], the two clamp masks, and `dssd`,
                  the per-element forward error ceiling of a float32 evaluation of ssd (module docstring of
                  tests/test_gpu_mind_exact.py, section 2d)
  finish()        out from a given m [B][V][12] and a given global mean: the finish pass alone
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from oracle.mind import SHIFT1, SHIFT2

U = 2.0 ** -24


def edges(img, delta):
    """oracle.mind.edge_selection: e_c = p[v + delta s1_c] - p[v + delta s2_c] on the replicate-padded image.
    img [B,1,D,H,W] -> [B,12,D,H,W]."""
    b, _, d, h, w = img.shape
    p = F.pad(img, [delta] * 6, mode="replicate")

    def pick(pos):
        z, y, x = (q * delta for q in pos)
        return p[:, 0, z:z + d, y:y + h, x:x + w]

    return torch.stack([pick(a) - pick(c) for a, c in zip(SHIFT1, SHIFT2)], dim=1)


def filter_axis(vol, taps, axis):
    """Replicate-padded correlation along spatial axis 0/1/2 of [B,C,D,H,W]: sum_t taps[t] vol[i + t - R], t ascending."""
    n = len(taps)
    pad = [0] * 6
    pad[4 - 2 * axis] = pad[5 - 2 * axis] = n // 2
    x = F.pad(vol, pad, mode="replicate")
    size = vol.shape[axis + 2]
    acc = taps[0] * x.narrow(axis + 2, 0, size)
    for t in range(1, n):
        acc = acc + taps[t] * x.narrow(axis + 2, t, size)
    return acc


def smooth(vol, taps):
    for axis in (0, 1, 2):                      # D, H, W: the kernel's order
        vol = filter_axis(vol, taps, axis)
    return vol


def to_voxel_major(t):
    """[B,12,D,H,W] -> [B][V][12]."""
    b, c = t.shape[:2]
    return t.reshape(b, c, -1).permute(0, 2, 1).contiguous()


def finish(m, gm, dtype=torch.float64):
    """mind.py:158-164 from m [B,V,12] and the global mean: var = mean_c m, clamped to [1e-3, 1e3] gm, out = exp(-m / var).
    -> (out [B,V,12], var before the clamp, var after it, low mask, high mask)."""
    m = m.to(dtype)
    gm = torch.as_tensor(gm, dtype=dtype)
    var = m.sum(dim=-1) / 12
    lo, hi = gm * 0.001, gm * 1000
    varc = torch.minimum(torch.maximum(var, lo), hi)
    return torch.exp(-(m / varc[..., None])), var, varc, var < lo, var > hi


def stages(img, noise, taps, rw, delta, dtype=torch.float64):
    """img [B,1,D,H,W], noise [B,12,D,H,W], taps: sequence of float32 values, rw: float32 value."""
    img, noise = img.to(dtype), noise.to(dtype)
    tp = [torch.tensor(float(t), dtype=dtype) for t in taps]
    rwt = torch.tensor(float(rw), dtype=dtype)
    e = edges(img, delta)
    rn = rwt * noise
    ev = e + rn
    q = ev * ev
    ssd = smooth(q, tp)
    mind = ssd - ssd.min(dim=1, keepdim=True)[0]
    m = to_voxel_major(mind)
    var = m.sum(dim=-1) / 12
    gm = var.mean()
    out, _, varc, low, high = finish(m, gm, dtype)
    b, _, d, h, w = img.shape
    # float32 forward error ceiling of ssd: ev carries u (|e| + |rw n| + |ev|) (difference, product, sum; the sum can
    # cancel, so the error is NOT relative to ev), q = ev^2 carries 2 |ev| dev + dev^2 + u q, and each of the three filter
    # passes rounds every term at most ntaps + 1 times (one product, ntaps - 1 additions, margin 1) with non-negative weights
    dev = U * (e.abs() + rn.abs() + ev.abs())
    dq = 2 * ev.abs() * dev + dev * dev + U * q
    kf = 3 * (len(taps) + 1)
    dssd = (smooth(dq, tp) + kf * U * ssd) * (1 + kf * U)
    return SimpleNamespace(ssd=ssd, m=m, var=var, varc=varc, gm=gm, low=low, high=high,
                           out=out.permute(0, 2, 1).reshape(b, 12, d, h, w).contiguous(), out_vm=out, dssd=to_voxel_major(dssd))


# ------------------------------------------------------------------------------------------------ error bounds
# Global mean, mind_ssd_kernel + mind_reduce_kernel: every voxel's var = (sum of 12 m) / 12 is rounded 12 times, a thread adds
# 4 of them (4), the wave butterfly adds 6 times, the block adds 8 wave sums (8); the partials continue in double and the mean
# is cast to float (1): 31 roundings of non-negative terms, so the relative error is below 32 u.
REL_GM = 32 * U
TINY = 2.0 ** -126       # a float32 result below the normal range may be flushed


def finish_bound(out, q, u_t=0.0, sub_t=0.0):
    """|mind_finish_kernel's out - finish() in float64 on the same m and global mean|, elementwise; out = exp(-q), q = m / var.
    var: 11 additions and a division (12 u); a clamp bound gm * 0.001f or gm * 1000.0f carries the constant's rounding and the
    product's (2 u; 1000 is exact), and the clamp passes on the larger of the two: 12 u.  q = m / var: one more, 13 u (14 u
    with the second-order terms).  exp(-q) moves by out (e^{14 u q} - 1); expf is within 1 ulp = 2 u out.  Storing in a
    16-bit type T adds u_T |stored value| and half the subnormal spacing SUB_T."""
    b32 = out * torch.expm1((14 * U * q).clamp(max=700.0)) + 2 * U * out + TINY      # (the clamp: out is 0 long before)
    return b32 + u_t * (out + b32) + sub_t


def out_bound(ref, ntaps, u_t=0.0, sub_t=0.0):
    """|a float32 evaluation of the whole descriptor - ref.out_vm|, elementwise [B,V,12], for any order of the sums with at
    most the roundings counted in stages() and above.  m_c = ssd_c - min: dm_c = dssd_c + max_c' dssd_c' + u m_c (the minimum
    of perturbed values moves by at most the largest perturbation).  var = mean_c m_c: mean_c dm_c + 12 u var.  The global
    mean: mean of dvar + REL_GM gm.  The clamp is 1-Lipschitz in var and in its bounds; a bound's error (1e-3 or 1e3 times
    the mean's, + 2 u) enters only where var is within a factor 2 of that bound.  out = exp(-m / var) then moves by
    out (e^{dq} - 1), dq = dm / var + q dvar / var, plus the finish pass's own arithmetic (finish_bound)."""
    dssd = ref.dssd
    dm = dssd + dssd.max(dim=-1, keepdim=True)[0] + U * ref.m
    dvar = dm.mean(dim=-1) + 12 * U * ref.var
    dgm = dvar.mean() + REL_GM * ref.gm
    lo, hi = 0.001 * ref.gm, 1000 * ref.gm
    dlo, dhi = 0.001 * dgm + 2 * U * lo, 1000 * dgm + 2 * U * hi
    dvarc = torch.where(ref.var < 2 * lo, torch.clamp(dvar, min=float(dlo)),
                        torch.where(ref.var > hi / 2, torch.clamp(dvar, min=float(dhi)), dvar))
    varc = ref.varc[..., None]
    q = ref.m / varc
    dq = dm / varc + q * dvarc[..., None] / varc
    return ref.out_vm * torch.expm1(dq.clamp(max=700.0)) + finish_bound(ref.out_vm, q + dq, u_t, sub_t)


def gm_bound(ref):
    """|a float32 evaluation's global mean - ref.gm| (see out_bound)."""
    dssd = ref.dssd
    dm = dssd + dssd.max(dim=-1, keepdim=True)[0] + U * ref.m
    return float((dm.mean(dim=-1) + 12 * U * ref.var).mean() + REL_GM * ref.gm)


# ------------------------------------------------------------------------------------------------ the clamp case
def clamp_inputs():
    """(img [1,1,40,40,64], noise): 1 in one half of W and 0 in the other, one voxel at 50, a block of texture of amplitude
    0.01.  With rw = 0 the flat halves have var = 0 (low clamp) and the neighbourhood of the spike has var far above 1e3 x the
    mean (high clamp); with rw = 0.05 the noise lifts the flat halves off the low clamp."""
    g = torch.Generator().manual_seed(4064)
    img = torch.zeros(1, 1, 40, 40, 64)
    img[..., 32:] = 1.0
    img[0, 0, 20, 20, 10] = 50.0
    img[0, 0, 4:12, 4:12, 40:56] += 0.01 * torch.randn(8, 8, 16, generator=g)
    return img, torch.randn(1, 12, 40, 40, 64, generator=g)


# ------------------------------------------------------------------------------------------------ the exact cases of pass A
DYADIC_TAPS = {3: [0.25, 0.5, 0.25],
               5: [1 / 16, 4 / 16, 6 / 16, 4 / 16, 1 / 16],
               7: [1 / 64, 6 / 64, 15 / 64, 20 / 64, 15 / 64, 6 / 64, 1 / 64]}
EXACT_KERNELS = [(delta, ntaps) for delta in (1, 2) for ntaps in (3, 5, 7)]
# (B, D, H, W): extents below the halo R + delta; one exact tile of 8 x 8 x 32; ragged; 27 tiles per sample, 81 in all (no
# multiple of 8: tiles in launch order); 8 and 16 tiles (the launch order is permuted)
EXACT_SHAPES = [(1, 1, 1, 1), (1, 1, 2, 3), (2, 2, 1, 40), (1, 3, 9, 33), (1, 8, 8, 32), (1, 9, 10, 37), (3, 19, 21, 70),
                (1, 16, 16, 64), (2, 16, 16, 40)]


def exact_inputs(delta, ntaps, shape):
    """Integer image in [0, 8) ([0, 4) for 7 taps), integer noise in [-2, 2], rw = 1, dyadic taps: q <= 81 (25) is an integer
    of 7 (5) bits and the three filter passes add 6 (12, 18) fraction bits, so every intermediate of a float32 evaluation
    has at most 23 significant bits and is exact, in any order of the sums."""
    b, d, h, w = shape
    g = torch.Generator().manual_seed(7919 * delta + 131 * ntaps + 17 * b + 5 * d + 3 * h + w)
    img = torch.randint(0, 4 if ntaps == 7 else 8, (b, 1, d, h, w), generator=g).float()
    noise = torch.randint(-2, 3, (b, 12, d, h, w), generator=g).float()
    return img, noise, DYADIC_TAPS[ntaps], 1.0
