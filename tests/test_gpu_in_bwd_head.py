"""GPU: the backward of the block in front of the segmentation head with its gz never stored.

  dgtta_seghead_warp_bwd_g16_d16   head_warp_bwd_kernel<T, true, false>: the fused head + warp backward that stops at d16, the
                                   gathered logit gradient in the storage type, in a caller-owned buffer.  No W^T, no gz.
  dgtta_instnorm_lrelu_bwd_head    in_bwd_head_kernel<T, 0 / 1>: both passes of the InstanceNorm + LeakyReLU backward rebuild
                                   gz[c] = sum_k W[sel[k]][c] float(d16[k]) on the fp32 matrix cores and use it unrounded.

The bounds are those of tests/test_gpu_warp.py (gathered gradient: e16 of its module docstring) and of
tests/test_gpu_instnorm.py (backward, fp32 partial sums), whose helpers and constants are imported, not restated.  One term is
added to the latter: gz is no input here but a 16-term fp32 dot product of exact products, so every gz carries
    e_g = (16 + 1) u sum_k |w d|          (the form of _within in tests/test_gpu_conv_exact.py: n + 1 roundings of n terms)
which enters da (|lrelu'| <= 1), hence dy through |gamma rstd| (e_g + dc1 + |xhat| dc2) with dc1 += E[e_g], dc2 += E[e_g |xhat|],
and dbeta / dgamma through V dc1 / V dc2.

LeakyReLU kink: as in test_gpu_instnorm.py the decision a > 0 must not matter where float64 |a| is within 1e-4 of 0 relative to
its terms; gz cannot be set to 0 element by element here, so the whole d16 ROW of such a voxel is zeroed (under 2 % of the rows).

Measured on an MI355X (largest error / bound; no bound widened): d16 0.72-0.97 on the interpolating maps (the storage rounding
itself reaches half an ulp) and 0.005 on the identity; dy 0.95-0.99 (its 16-bit rounding again), dgamma / dbeta under 0.01
(worst-case sums of rounding errors that do not line up)."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import instnorm_ref as iref
import test_gpu_instnorm as tin
import test_gpu_warp as tw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, NS = 32, 16
U, U_T, SUB_T, TDT = tin.U, tin.U_T, tin.SUB_T, tin.TDT
SLOPE = tin.SLOPE
OK, UNSUPPORTED = 0, -2


def _lib():
    from dg_tta_amd import _lib as L
    return L.load()


# ------------------------------------------------------------------------------------------------ head + warp backward, d16 mode
def k_head_bwd_d16(p):
    """dgtta_seghead_warp_bwd_g16_d16 on problem p (tests/test_gpu_warp.py::_head_bwd_problem) -> (d16 as stored, dw, db)."""
    from dg_tta_amd._lib import check, ptr, stream_of
    lib = _lib()
    B, D, H, W, _ = p.z_t.shape
    n, dt = B * D * H * W, p.dt
    zr = tw.Rows(n, C, C, math.nan, p.z_t, dtype=TDT[dt])
    gr = tw.Rows(n, NS, NS, math.nan, p.gout, dtype=TDT[dt])
    d16 = tw.Rows(n, NS, NS, tw.SENTINEL, dtype=TDT[dt])
    dw, db = tw.Rows(NS, C, C, tw.SENTINEL), tw.Rows(1, NS, NS, tw.SENTINEL)
    th, h_theta = p.theta.to(DEV), p.theta.clone().contiguous()
    nws = lib.dgtta_seghead_warp_bwd_ws_bytes(B, C, NS, D, H, W)
    assert nws > 0
    ws = torch.full((nws + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    check(lib.dgtta_seghead_warp_bwd_g16_d16(zr.ptr, gr.ptr, ptr(th), h_theta.data_ptr(), NS, d16.ptr, dw.ptr, db.ptr, ptr(ws), nws,
                                             B, C, D, H, W, 1, 0, dt, stream_of()), "seghead_warp_bwd_g16_d16")
    torch.cuda.synchronize()
    assert bool((ws[nws:] == 0xFF).all()), "seghead_warp_bwd_g16_d16 wrote past its workspace"
    for r, what in ((d16, "d16"), (dw, "dw"), (db, "db")):
        r.assert_padding_untouched(f"seghead_warp_bwd_g16_d16 {what}")
    assert torch.equal(zr.get().view(torch.int16), p.z_t.reshape(-1, C).view(torch.int16)), "the backward modified z"
    return d16.get().view(B, D, H, W, NS), dw.get(), db.get().view(-1)


@pytest.mark.parametrize("dt", [2, 1], ids=["fp16", "bf16"])
@pytest.mark.parametrize("names", [("tta008", "strong"), ("rot_z", "shift_half"), ("identity", "outside")], ids="+".join)
def test_head_warp_backward_without_gz(names, dt):
    """B = 2, 8 x 12 x 20: ragged against the 16 x 4 x 4 tile in W, B V = 3840 a multiple of 128.  dw_sel and db_sel are those of
    dgtta_seghead_warp_bwd_g16 bit for bit (the same d16 rows feed the same weight-gradient kernels, the same block sums the bias);
    d16_out is the float64 gather rounded to the storage type, within the bound test_gpu_warp.py has for the 16-bit copy of the
    gathered gradient: e16 = E_acc + u_T (|acc| + E_acc) + SUB_T."""
    B, size = 2, (8, 12, 20)
    p = tw._head_bwd_problem(B, size, names, (dt, True, NS, True, 0, True, True))
    assert _lib().dgtta_seghead_warp_supported(p.theta.data_ptr(), B, C, NS, *size, dt) == 1
    rc, gz, dw_ref, db_ref = tw.k_head_bwd(p.z_t, p.gout, p.theta, p.w, p.sel, p.nsel, dt, p.o)
    assert rc == OK
    d16, dw, db = k_head_bwd_d16(p)
    assert torch.equal(dw.view(torch.int32), dw_ref.view(torch.int32)), "dw_sel differs from dgtta_seghead_warp_bwd_g16"
    assert torch.equal(db.view(torch.int32), db_ref.view(torch.int32)), "db_sel differs from dgtta_seghead_warp_bwd_g16"
    adj = tw._adjoint(p.gout.double(), p.theta, size, "zeros", 1)
    e16 = adj.bound + U_T[dt] * (adj.ref.abs() + adj.bound) + SUB_T[dt]
    tw._within(f"d16 {'+'.join(names)} dt{dt}", d16.double(), adj.ref, e16)
    for b, name in enumerate(names):
        if name == "outside":
            assert not bool(d16[b].float().any())
        else:
            assert float(d16[b].float().abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------ InstanceNorm backward from d16
@functools.lru_cache(maxsize=None)
def _problem(B, V, dt):
    """y, statistics and affine parameters of tests/test_gpu_instnorm.py::_inputs(B, 32, V, dt); d16 rows, head rows and the
    float64 reference of the backward with gz64 = d W from the same 16-bit d.  Computed once per case, nothing modifies it."""
    inp = tin._inputs(B, C, V, dt)
    g = torch.Generator().manual_seed(7001 * B + 13 * V + dt)
    w = torch.randn(105, C, generator=g) * 0.3
    sel = torch.tensor(tw.SEL16, dtype=torch.int32)
    d32 = torch.randn(B, V, NS, generator=g)
    m32, r32 = inp.mr32[..., 0].double(), inp.mr32[..., 1].double()
    xhat, a = iref.pre_activation(inp.y64, m32, r32, inp.g64, inp.b64)
    near = (a.abs() < 1e-4 * ((xhat * inp.g64).abs() + inp.b64.abs() + 1.0)).any(dim=-1)
    assert float(near.float().mean()) < 0.02, f"kink guard touches {float(near.float().mean()):.2%} of the rows"
    d32[near] = 0.0
    d_t = d32.to(TDT[dt])
    d64, w64 = d_t.double(), w[sel.long()].double()
    gz64 = d64 @ w64
    e_g = (NS + 1) * U * (d64.abs() @ w64.abs())
    dy, dgamma, dbeta, S0, S1 = iref.backward(gz64, inp.y64, m32, r32, inp.g64, inp.b64, SLOPE)
    da = torch.where(a > 0, gz64, SLOPE * gz64)
    c1, c2 = S0 / V, S1 / V
    dc1 = 2.0 ** -17 * da.abs().mean(dim=1) + e_g.mean(dim=1)
    dc2 = 2.0 ** -17 * (da * xhat).abs().mean(dim=1) + (e_g * xhat.abs()).mean(dim=1)
    gr = (inp.g64 * r32).abs()[:, None, :]
    b_dy = U_T[dt] * dy.abs() + SUB_T[dt] + gr * (
        8 * U * (da.abs() + c1.abs()[:, None, :] + (xhat * c2[:, None, :]).abs()) + e_g + dc1[:, None, :] + xhat.abs() * dc2[:, None, :])
    bounds = SimpleNamespace(dy=b_dy, dbeta=V * dc1.sum(dim=0) + U * dbeta.abs(), dgamma=V * dc2.sum(dim=0) + U * dgamma.abs())
    ref = SimpleNamespace(dy=dy, dgamma=dgamma, dbeta=dbeta)
    return SimpleNamespace(inp=inp, w=w, sel=sel, d_t=d_t, ref=ref, bounds=bounds)


def k_in_bwd_head(pr, ld_extra=0, accumulate=0, bufs=None, with_sel=True):
    """dgtta_instnorm_lrelu_bwd_head -> ((dy [B,V,C] as stored, dgamma, dbeta) on the CPU, buffers for a second run)."""
    from dg_tta_amd._lib import check, ptr, stream_of
    inp = pr.inp
    ld, col0 = tin._layout(C, ld_extra)
    if bufs is None:
        bufs = SimpleNamespace(y=tin.Rows(inp, ld, col0, math.nan, inp.y_t), dy=tin.Rows(inp, ld, col0, tin.SENTINEL),
                               d=pr.d_t.to(DEV).contiguous(), gamma=inp.gamma.to(DEV), beta=inp.beta.to(DEV), mr=inp.mr32.to(DEV),
                               w=(pr.w if with_sel else pr.w[pr.sel.long()].contiguous()).to(DEV), sel=pr.sel.to(DEV) if with_sel else None,
                               dgamma=torch.full((C,), math.nan, device=DEV), dbeta=torch.full((C,), math.nan, device=DEV))
    ws, nws = tin._ws(inp.B, C, inp.V)
    check(_lib().dgtta_instnorm_lrelu_bwd_head(ptr(bufs.d), ptr(bufs.w), ptr(bufs.sel), NS, bufs.y.ptr, ld, ptr(bufs.gamma), ptr(bufs.beta),
                                               ptr(bufs.mr), bufs.dy.ptr, ld, ptr(bufs.dgamma), ptr(bufs.dbeta), ptr(ws), nws, inp.B, C, inp.V,
                                               SLOPE, accumulate, inp.dt, stream_of()), "instnorm_lrelu_bwd_head")
    torch.cuda.synchronize()
    bufs.dy.assert_padding_untouched("dy")
    assert torch.equal(bufs.y.get().view(torch.uint8), inp.y_t.view(torch.uint8)), "the backward modified y"
    assert torch.equal(bufs.d.cpu().view(torch.int16), pr.d_t.view(torch.int16)), "the backward modified d16"
    return (bufs.dy.get(), bufs.dgamma.cpu(), bufs.dbeta.cpu()), bufs


IN_CASES = [  # (B, V, dt, ld_extra, sel given)
    (2, 3840, 2, 0, True),        # the shape of the head + warp test: whole units of 16 rows
    (2, 3851, 1, 0, False),       # V no multiple of the 16 rows a wave takes: a ragged last unit
    (1, 13, 2, 0, True),          # less than one unit
    (3, 2049, 1, 32, True),       # the second half of rows of 64 elements
    # the sums pass: 128 workgroups per sample take 64 rows at a time (B >= 32: the 128-block floor) - a second round for some
    # waves (two units in flight), none for the others, a ragged last unit
    (32, 128 * 64 + 16 * 5 + 3, 2, 0, True),
]


@pytest.mark.parametrize("case", IN_CASES, ids=lambda c: "B{}-V{}-dt{}-ld+{}-sel{:d}".format(*c))
def test_instnorm_backward_from_d16_vs_float64(case):
    B, V, dt, ld_extra, with_sel = case
    # a lane of the sums pass adds at most 64 fp32 terms before the sums continue in double, as the bound's 2^-17 assumes
    assert tin._cdiv(V, tin.reduce_blocks(V, B) * 64) <= 64
    pr = _problem(B, V, dt)
    tag = "head " + "-".join(map(str, case))
    out0, bufs = k_in_bwd_head(pr, ld_extra, with_sel=with_sel)
    tin._check_backward(tag, pr.ref, out0, pr.bounds)
    assert float(out0[0].float().abs().max()) > 0
    # accumulate = 1 on the same buffers: twice the sums (the factor of test_gpu_instnorm.py), dy unchanged
    out1, _ = k_in_bwd_head(pr, ld_extra, accumulate=1, bufs=bufs, with_sel=with_sel)
    tin._check_backward(f"{tag} accumulate", pr.ref, out1, pr.bounds, factor=2.0)
    assert torch.equal(out1[0].view(torch.uint8), out0[0].view(torch.uint8)), "dy changed with accumulate = 1"


def test_instnorm_backward_from_d16_argument_checks():
    """Shapes the kernel is not built for are refused before anything is launched."""
    from dg_tta_amd._lib import ptr, stream_of
    lib = _lib()
    t = torch.zeros(4096, device=DEV)
    dy, dg, db = torch.zeros(4096, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    ws, nws = tin._ws(1, C, 16)

    def call(nsel=NS, c=C, dt=2, d=t, w=t):
        return lib.dgtta_instnorm_lrelu_bwd_head(ptr(d), ptr(w), None, nsel, ptr(t), c, ptr(t), ptr(t), ptr(t), ptr(dy), c, ptr(dg), ptr(db),
                                                 ptr(ws), nws, 1, c, 16, SLOPE, 0, dt, stream_of())
    assert call() == OK
    assert call(nsel=8) == UNSUPPORTED and call(c=16) == UNSUPPORTED and call(dt=0) == UNSUPPORTED
    assert call(d=None) == tin.BADARG and call(w=None) == tin.BADARG
    torch.cuda.synchronize()
