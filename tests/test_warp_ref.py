"""Host test of tests/warp_ref.py, the float64 restatement the GPU tests of warp.hip are measured against: its warp against
F.affine_grid + F.grid_sample in float64 (zeros / border padding, linear / nearest, resize, B = 2, non-cubic sizes), its
explicit-scatter adjoint and the head gradients against torch.autograd of the composed float64 expression.  This is the
licence for using the restatement as the reference on the GPU."""
import pytest
import torch
import torch.nn.functional as F

import warp_ref as wref

REL = 1e-12


def _close(got, ref, what):
    err = float((got - ref).abs().max())
    lim = REL * max(float(ref.abs().max()), 1.0)
    assert err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e}"


def _theta(B, strength, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.eye(3, 4, dtype=torch.float64)[None] + strength * torch.randn(B, 3, 4, generator=g, dtype=torch.float64)


def _torch_warp(x_cl, theta, dst_size, pad, interp):
    """x_cl [B, D, H, W, C] -> [B, Dd, Hd, Wd, C] through torch's own grid and sampler."""
    x = x_cl.permute(0, 4, 1, 2, 3)
    grid = F.affine_grid(theta, [x.shape[0], x.shape[1], *dst_size], align_corners=False)
    y = F.grid_sample(x, grid, mode="bilinear" if interp == "linear" else "nearest", padding_mode=pad, align_corners=False)
    return y.permute(0, 2, 3, 4, 1)


CASES = [  # (B, C, src_size, dst_size, strength)
    (2, 3, (7, 9, 21), (7, 9, 21), 0.1),
    (2, 5, (8, 8, 18), (8, 8, 18), 0.3),          # strong: a good part of the samples leaves the volume
    (1, 2, (5, 6, 18), (7, 4, 11), 0.1),          # resize
    (2, 4, (1, 6, 9), (1, 6, 9), 0.05),           # a size-1 axis
    (1, 1, (3, 1, 5), (4, 2, 3), 0.2),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}-C{}-{}-{}-{}".format(c[0], c[1], "x".join(map(str, c[2])), "x".join(map(str, c[3])), c[4]))
@pytest.mark.parametrize("pad", ["zeros", "border"])
def test_warp_and_adjoint_match_grid_sample_in_float64(case, pad):
    B, C, src, dst, strength = case
    g = torch.Generator().manual_seed(B * 100 + C)
    x = torch.randn(B, *src, C, generator=g, dtype=torch.float64).requires_grad_()
    theta = _theta(B, strength, 11 * B + C)
    gout = torch.randn(B, *dst, C, generator=g, dtype=torch.float64)
    y = _torch_warp(x, theta, dst, pad, "linear")
    y.backward(gout)
    _close(wref.warp(x.detach(), theta, dst, pad, "linear"), y.detach(), "warp")
    _close(wref.warp_adjoint(gout, theta, src, pad), x.grad, "warp_adjoint")
    # sub: the volume continued by a constant instead of zeros = warp(x - sub) + sub
    _close(wref.warp(x.detach(), theta, dst, pad, "linear", sub=0.7), _torch_warp(x.detach() - 0.7, theta, dst, pad, "linear") + 0.7, "sub")
    # |.|-adjoint: weights are non-negative
    _close(wref.warp_abs_adjoint(gout, theta, src, pad), wref.warp_adjoint(gout.abs(), theta, src, pad), "abs adjoint")
    assert bool((wref.warp_abs_adjoint(gout, theta, src, pad) >= wref.warp_adjoint(gout, theta, src, pad).abs() - 1e-12).all())


@pytest.mark.parametrize("case", CASES[:4], ids=lambda c: "B{}-C{}-{}".format(c[0], c[1], "x".join(map(str, c[2]))))
@pytest.mark.parametrize("pad", ["zeros", "border"])
def test_nearest_matches_grid_sample(case, pad):
    B, C, src, dst, strength = case
    g = torch.Generator().manual_seed(B * 100 + C + 1)
    x = torch.randn(B, *src, C, generator=g, dtype=torch.float64)
    theta = _theta(B, strength, 13 * B + C)
    got, ref = wref.warp(x, theta, dst, pad, "nearest"), _torch_warp(x, theta, dst, pad, "nearest")
    assert torch.equal(got, ref)


def test_sample_positions_are_the_unnormalised_affine_grid():
    theta = _theta(2, 0.2, 5)
    src, dst = (5, 6, 18), (7, 4, 11)
    grid = F.affine_grid(theta, [2, 1, *dst], align_corners=False)
    pos = wref.sample_positions(theta, dst, src)
    for a, n in zip(range(3), (src[2], src[1], src[0])):
        _close(pos[a], ((grid[..., a] + 1.0) * n - 1.0) / 2.0, f"axis {a}")
    assert float(wref.base_coords(1)[0]) == 0.0
    ident = torch.eye(3, 4, dtype=torch.float64)[None]
    ix, iy, iz = wref.sample_positions(ident, (3, 4, 5), (3, 4, 5))
    _close(ix[0, 1, 2], torch.arange(5, dtype=torch.float64), "identity ix")
    _close(iz[0, :, 0, 0], torch.arange(3, dtype=torch.float64), "identity iz")


def test_candidate_sums_count_the_corner_samples():
    """With tol = 0 and a map whose positions are not lattice points: count = number of samples with the voxel as a corner,
    so the counts sum to 8 per sample inside the volume, and sum |g| >= the weighted |.|-adjoint."""
    theta = _theta(1, 0.02, 3)
    theta[:, :, 3] = 0.0
    size = (6, 7, 9)
    gout = torch.randn(1, *size, 2, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    cnt, sums = wref.candidate_sums(gout, theta, size)
    pos = wref.sample_positions(theta, size, size)
    per_sample = sum(wref._flat_index(cx, cy, cz, size)[1].long() for cx, cy, cz, _ in wref._corners(pos))
    assert int(cnt.sum()) == int(per_sample.sum())
    assert bool((sums >= wref.warp_abs_adjoint(gout, theta, size) - 1e-12).all())
    cnt2, sums2 = wref.candidate_sums(gout, theta, size, tol=0.3)
    assert bool((cnt2 >= cnt).all()) and bool((sums2 >= sums).all()) and float(cnt2.sum()) > float(cnt.sum())


@pytest.mark.parametrize("sel", [None, [7, 2, 9, 0]])
def test_head_gradients_match_autograd_of_the_composed_expression(sel):
    B, size, Cin, K = 2, (4, 5, 9), 6, 11
    g = torch.Generator().manual_seed(17)
    z = torch.randn(B, *size, Cin, generator=g, dtype=torch.float64).requires_grad_()
    w = torch.randn(K, Cin, generator=g, dtype=torch.float64).requires_grad_()
    bias = torch.randn(K, generator=g, dtype=torch.float64).requires_grad_()
    theta = _theta(B, 0.15, 23)
    idx = None if sel is None else torch.tensor(sel)
    nsel = K if sel is None else len(sel)
    gout = torch.randn(B, *size, nsel, generator=g, dtype=torch.float64)
    logits = z @ (w if idx is None else w[idx]).t() + (bias if idx is None else bias[idx])
    y = _torch_warp(logits, theta, size, "zeros", "linear")
    y.backward(gout)
    _close(wref.head_then_warp(z.detach(), w.detach(), bias.detach(), idx, theta), y.detach(), "head_then_warp")
    gl, gz, dw, db = wref.head_then_warp_grads(z.detach(), w.detach(), idx, theta, gout)
    _close(gz, z.grad, "gz")
    _close(dw, w.grad if idx is None else w.grad[idx], "dw_sel")
    _close(db, bias.grad if idx is None else bias.grad[idx], "db_sel")
    if idx is not None:                                  # rows that were not selected get no gradient
        rest = [k for k in range(K) if k not in sel]
        assert not bool(w.grad[rest].any()) and not bool(bias.grad[rest].any())
