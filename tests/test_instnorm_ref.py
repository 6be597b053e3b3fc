"""Host test of tests/instnorm_ref.py, the float64 restatement the GPU tests of instnorm.hip are measured against: its
forward and backward against torch.autograd of F.leaky_relu(F.instance_norm(...)) in float64, and its per-tile partial
sums against the whole-sample sums.  This is the licence for using the restatement as the reference on the GPU."""
import pytest
import torch
import torch.nn.functional as F

import instnorm_ref as iref

EPS, SLOPE = 1e-5, 0.01
REL = 1e-12


def _close(got, ref, what):
    err = float((got - ref).abs().max())
    lim = REL * float(ref.abs().max())
    assert err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e}"


@pytest.mark.parametrize("shape", [(2, 5, 37), (1, 8, 64)])
def test_forward_and_backward_match_autograd_in_float64(shape):
    B, C, V = shape
    g = torch.Generator().manual_seed(B * 1000 + C * 10 + V)
    x = (torch.randn(B, C, V, generator=g, dtype=torch.float64) * 1.7 + 0.4).requires_grad_()
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_()
    beta = (torch.randn(C, generator=g, dtype=torch.float64) * 0.3).requires_grad_()
    gz = torch.randn(B, C, V, generator=g, dtype=torch.float64)
    z = F.leaky_relu(F.instance_norm(x, weight=gamma, bias=beta, eps=EPS), SLOPE)
    z.backward(gz)

    rows = lambda t: t.detach().permute(0, 2, 1).contiguous()          # [B,C,V] -> [B,V,C]
    y64, gz64 = rows(x), rows(gz)
    mean, rstd = iref.stats(y64, EPS)
    _close(mean, x.detach().mean(dim=2), "mean")
    _close(rstd, 1.0 / torch.sqrt(x.detach().var(dim=2, unbiased=False) + EPS), "rstd")
    _close(iref.forward(y64, mean, rstd, gamma.detach(), beta.detach(), SLOPE), rows(z), "z")
    dy, dgamma, dbeta, S0, S1 = iref.backward(gz64, y64, mean, rstd, gamma.detach(), beta.detach(), SLOPE)
    _close(dy, rows(x.grad), "dy")
    _close(dgamma, gamma.grad, "dgamma")
    _close(dbeta, beta.grad, "dbeta")
    _close(S0.sum(dim=0), dbeta, "S0")
    _close(S1.sum(dim=0), dgamma, "S1")


@pytest.mark.parametrize("nblk", [1, 2, 7, 64, 100])
def test_partials_of_any_partition_reproduce_the_whole_sample_sums(nblk):
    B, V, C = 2, 61, 5
    g = torch.Generator().manual_seed(nblk)
    v0 = torch.randn(B, V, C, generator=g, dtype=torch.float64) + 3.0
    v1 = v0 * v0
    cuts = iref.ragged_cuts(V, nblk, seed=nblk)
    buf = iref.partials(v0, v1, cuts)
    assert buf.dtype == torch.float64 and buf.numel() == iref.HEADER_DOUBLES + B * nblk * C * 2
    assert buf.numel() * 8 == 256 + B * nblk * C * 2 * 8                # a 256-byte header, then [B][nblk][C][2] doubles
    n, body = iref.unpack_partials(buf, B, C)
    assert n == nblk and int(buf[:1].view(torch.int64)[0]) == nblk      # the header's first int64
    assert not buf[1:iref.HEADER_DOUBLES].any()
    if nblk > 2:
        assert any(a == b for a, b in zip(cuts, cuts[1:])), "the partition has no empty tile"
    _close(body[..., 0].sum(dim=1), v0.sum(dim=1), "sum of values0")
    _close(body[..., 1].sum(dim=1), v1.sum(dim=1), "sum of values1")
    for i in (0, nblk // 2, nblk - 1):                                  # single tiles, laid out [b][blk][c][pair]
        lo, hi = cuts[i], cuts[i + 1]
        ref = v0[:, lo:hi].sum(dim=1)
        assert float((body[:, i, :, 0] - ref).abs().max()) <= REL * float(v0.abs().sum(dim=1).max())
