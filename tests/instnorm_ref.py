"""InstanceNorm + LeakyReLU of dg_tta_amd/csrc/instnorm.hip restated in float64 (test infrastructure): torch on the CPU,
no autograd, the formulas written out.  Everything works on rows [B, V, C] (V voxels of a sample, channels last); the
per-(sample, channel) quantities are [B, C].

    mean = E_v y            rstd = 1 / sqrt(E_v (y - mean)^2 + eps)                       (biased variance)
    xhat = (y - mean) rstd  a = xhat gamma + beta      z = a if a > 0 else slope a
    da = gz if a > 0 else slope gz      S0 = sum_v da      S1 = sum_v da xhat
    dy = gamma rstd ((da - S0 / V) - xhat S1 / V)      dgamma = sum_b S1      dbeta = sum_b S0

partials() lays per-tile sums out as the conv epilogues and the data-gradient kernel do (dgtta_conv3d_stats_bytes,
in_bwd_finalize_kernel given mean_rstd): a 256-byte header whose first int64 is the number of tiles per sample, then
[B][nblk][C][2] doubles - (sum y, sum y^2) for the forward, (sum da, sum da y) for the backward.
"""
import torch

HEADER_DOUBLES = 32          # 256 bytes


def stats(y64, eps):
    """[B,V,C] float64 -> (mean, rstd), each [B,C]."""
    mean = y64.mean(dim=1)
    var = ((y64 - mean[:, None, :]) ** 2).mean(dim=1)
    return mean, 1.0 / torch.sqrt(var + eps)


def pre_activation(y64, mean, rstd, gamma, beta):
    """(xhat, a), each [B,V,C]."""
    xhat = (y64 - mean[:, None, :]) * rstd[:, None, :]
    return xhat, xhat * gamma + beta


def forward(y64, mean, rstd, gamma, beta, slope):
    _, a = pre_activation(y64, mean, rstd, gamma, beta)
    return torch.where(a > 0, a, slope * a)


def backward(gz64, y64, mean, rstd, gamma, beta, slope):
    """-> (dy [B,V,C], dgamma [C], dbeta [C], S0 [B,C], S1 [B,C])."""
    V = y64.shape[1]
    xhat, a = pre_activation(y64, mean, rstd, gamma, beta)
    da = torch.where(a > 0, gz64, slope * gz64)
    S0 = da.sum(dim=1)
    S1 = (da * xhat).sum(dim=1)
    dy = (gamma * rstd)[:, None, :] * ((da - S0[:, None, :] / V) - xhat * S1[:, None, :] / V)
    return dy, S1.sum(dim=0), S0.sum(dim=0), S0, S1


def partials(values0, values1, cuts):
    """Per-tile float64 sums of two [B,V,C] fields for the partition of the V rows into tiles [cuts[i], cuts[i+1])
    (cuts[0] = 0, cuts[-1] = V, non-decreasing: a repeated cut is an empty tile).  Returns the buffer as a float64 tensor
    of 32 + B*nblk*C*2 elements whose first 8 bytes hold nblk as an int64."""
    B, V, C = values0.shape
    cuts = [int(c) for c in cuts]
    nblk = len(cuts) - 1
    assert nblk >= 1 and cuts[0] == 0 and cuts[-1] == V and all(a <= b for a, b in zip(cuts, cuts[1:]))
    tile = torch.zeros(V, dtype=torch.int64)
    for i in range(nblk):
        tile[cuts[i]:cuts[i + 1]] = i
    body = torch.zeros(B, nblk, C, 2, dtype=torch.float64)
    body[..., 0].index_add_(1, tile, values0.double())
    body[..., 1].index_add_(1, tile, values1.double())
    buf = torch.zeros(HEADER_DOUBLES + body.numel(), dtype=torch.float64)
    buf[:HEADER_DOUBLES].view(torch.int64)[0] = nblk
    buf[HEADER_DOUBLES:] = body.reshape(-1)
    return buf


def unpack_partials(buf, B, C):
    """The inverse view: (nblk, [B,nblk,C,2])."""
    nblk = int(buf[:HEADER_DOUBLES].view(torch.int64)[0])
    return nblk, buf[HEADER_DOUBLES:].reshape(B, nblk, C, 2)


def ragged_cuts(V, nblk, seed):
    """A partition of V rows into nblk ragged tiles, some of them empty (nblk > 1), reproducible from the seed."""
    if nblk == 1:
        return [0, V]
    g = torch.Generator().manual_seed(seed)
    inner = torch.randint(0, V + 1, (nblk - 1,), generator=g)
    if nblk > 2:
        inner[1] = inner[0]              # at least one empty tile whatever the draw
    return [0] + sorted(int(c) for c in inner) + [V]
