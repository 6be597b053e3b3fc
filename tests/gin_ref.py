"""GIN chain (oracle/gin.py) restated in float64 by default, with its stages and the worst-case forward error ceiling of a
float32 evaluation (test infrastructure; licensed by tests/test_gin_ref.py).

chain() returns mixed, the two Frobenius norms, out, and `ceil_mixed` / `ceil_out`: elementwise bounds on
|float32 result - float64 result| that hold for ANY order of the sums (u = 2^-24), propagated layer by layer:

  layer      E_l = |W_l| * E_{l-1} + (n_l + 2) u (|W_l| * |a_{l-1}| + |shift_l|)      n_l = c_in k^3 products per output
             (* = the layer's zero-padded correlation with the absolute kernel; n_l - 1 additions of rounded products, the
             shift addition and one spare), then + u |a_l| for the LeakyReLU product (the function is 1-Lipschitz and
             continuous, so a sign decided differently costs nothing more)
  blend      E_mixed = alpha E_4 + 3 u (|alpha a_4| + |(1 - alpha) x|)       (1 - alpha, two products, one sum)
  norms      a sum of squares taken with K roundings per term has relative error K u, its root K u / 2 + u:
             REL_NORM = 12 u covers the kernels' K = 20 (below); the input error adds ||E_mixed||_2 to ||mixed||
  scale      out = (mixed * (1 / (|mixed| + 1e-5))) * |x|: 4 roundings, REL_SCALE = 4 u

K for gin_chain_kernel + gin_norm_kernel: a thread squares (1) and adds 4 values (4), the wave butterfly adds 6 times, the
block adds 8 wave sums, the double sum of the per-tile partials and its cast to float (1): 20; sqrtf is correctly rounded.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS32 = float(np.float32(1e-5))          # the kernel's 1e-5f
SLOPE32 = float(np.float32(0.01))
REL_NORM = 12 * U
REL_SCALE = 4 * U


def _conv(x, ker, k, nb):
    sp = x.shape[2:]
    c_out = ker.shape[0] // nb
    y = F.conv3d(x.reshape(1, -1, *sp), ker, padding=k // 2, groups=nb)
    return y.reshape(nb, c_out, *sp)


def chain(x_in, alpha, ks, kers, shifts, dtype=torch.float64, ceiling=True):
    """x_in [B,1,D,H,W], alpha [B], kers[l] [c_out B, c_in, k,k,k], shifts[l] [c_out B,1,1,1]: float32 values."""
    nb = x_in.shape[0]
    x_in, alpha = x_in.to(dtype), alpha.to(dtype)
    kers, shifts = [k.to(dtype) for k in kers], [s.to(dtype) for s in shifts]
    slope = torch.tensor(SLOPE32, dtype=dtype)
    a, err = x_in, torch.zeros_like(x_in)
    for li, (k, ker, sh) in enumerate(zip(ks, kers, shifts)):
        shv = sh.reshape(nb, -1, 1, 1, 1)
        y = _conv(a, ker, k, nb) + shv
        if ceiling:
            n = ker.shape[1] * k ** 3
            err = _conv(err, ker.abs(), k, nb) + (n + 2) * U * (_conv(a.abs(), ker.abs(), k, nb) + shv.abs())
        if li < len(ks) - 1:
            y = torch.where(y > 0, y, y * slope)
            if ceiling:
                err = err + U * y.abs()
        a = y
    al = alpha.view(nb, 1, 1, 1, 1)
    om = 1.0 - al
    mixed = al * a + om * x_in
    n_in = x_in.reshape(nb, -1).norm(dim=1)
    n_mix = mixed.reshape(nb, -1).norm(dim=1)
    eps = torch.tensor(EPS32, dtype=dtype)
    scale = (1.0 / (n_mix + eps)).view(nb, 1, 1, 1, 1)
    out = (mixed * scale) * n_in.view(nb, 1, 1, 1, 1)
    res = SimpleNamespace(y=a, mixed=mixed, n_in=n_in, n_mix=n_mix, out=out)
    if ceiling:
        e_mixed = al * err + 3 * U * ((al * a).abs() + (om * x_in).abs())
        d_mix = (REL_NORM * n_mix + e_mixed.reshape(nb, -1).norm(dim=1)).view(nb, 1, 1, 1, 1)
        s = scale * n_in.view(nb, 1, 1, 1, 1)
        res.ceil_mixed = e_mixed
        res.ceil_out = s * e_mixed + out.abs() * (d_mix * scale + REL_NORM + REL_SCALE)
    return res


def recover_mixed(out, n_in, n_mix):
    """mixed from out with the float64 norms: out (|mixed| + 1e-5) / |x|."""
    nb = out.shape[0]
    return out.double() * ((n_mix + EPS32) / n_in).view(nb, 1, 1, 1, 1)


# relative error of the kernel's `out` against mixed * scale with exact mixed: both norms and the four roundings of the scale
REL_RECOVER = 2 * REL_NORM + REL_SCALE


# ------------------------------------------------------------------------------------------------ the exact cases
ALL_KS = [(a, b, c, d) for a in (1, 3) for b in (1, 3) for c in (1, 3) for d in (1, 3)]
EXACT_SHAPES = [(1, 1, 1, 1), (2, 1, 2, 3), (1, 3, 1, 33), (1, 8, 8, 32), (2, 9, 11, 37)]
EXACT_ALPHAS = (1.0, 0.5, 0.0)


def exact_inputs(ks, shape, seed=0):
    """Integer x in [1, 4), 0/1 kernels (k = 3: each tap set with probability 0.1; k = 1: 0.7; at least one tap per output
    row), shifts in {1, 2} (non-zero: a voxel outside the volume that is not forced to 0 carries the shift), alpha cycling
    through 1, 0.5, 0.  Everything is a non-negative integer, so the LeakyReLU is the identity, and the blend adds two
    multiples of 1/2: exact in float32 while |value| < 2^23."""
    from oracle.gin import layer_channels
    b, d, h, w = shape
    g = torch.Generator().manual_seed(1009 * sum(k * 3 ** i for i, k in enumerate(ks)) + 31 * b + 7 * d + 3 * h + w + 100003 * seed)
    x = torch.randint(1, 4, (b, 1, d, h, w), generator=g).float()
    kers, shifts = [], []
    for k, (cin, cout) in zip(ks, layer_channels(1)):
        ker = (torch.rand(cout * b, cin, k, k, k, generator=g) < (0.1 if k == 3 else 0.7)).float()
        flat = ker.view(cout * b, -1)
        pick = torch.randint(0, flat.shape[1], (cout * b,), generator=g)
        flat[torch.arange(cout * b), pick] = 1.0
        kers.append(ker)
        shifts.append(torch.randint(1, 3, (cout * b, 1, 1, 1), generator=g).float())
    first = seed + (1 if d == 1 else 0)          # (1, 0.5) for two samples; (0.5, 0) at the D = 1 shape, where alpha = 0 is covered
    alpha = torch.tensor([EXACT_ALPHAS[(i + first) % 3] for i in range(b)])
    return x, alpha, list(ks), kers, shifts


def real_inputs(ks, shape, seed=0):
    """randn x, kernels and shifts (both LeakyReLU branches), alpha in (0, 1) for the first sample, then 0 and 1."""
    from oracle.gin import layer_channels
    b, d, h, w = shape
    g = torch.Generator().manual_seed(77 + 1009 * sum(k * 3 ** i for i, k in enumerate(ks)) + 7 * d + 3 * h + w + 100003 * seed)
    x = torch.randn(b, 1, d, h, w, generator=g)
    kers = [torch.randn(cout * b, cin, k, k, k, generator=g) for k, (cin, cout) in zip(ks, layer_channels(1))]
    shifts = [torch.randn(cout * b, 1, 1, 1, generator=g) for _, cout in layer_channels(1)]
    alpha = torch.rand(b, generator=g)
    for i in range(1, b):
        alpha[i] = float((i + seed) % 2)
    return x, alpha, list(ks), kers, shifts
