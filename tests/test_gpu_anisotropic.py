"""Anisotropic layers on the GPU: the dgtta_conv3d_* / dgtta_convT3d_s_* kernels through the C ABI against torch CPU float64, and
a whole anisotropic PlainConvUNet (forward, every parameter gradient, one TTA step) against the CPU oracle."""
import copy

import pytest
import torch
import torch.nn.functional as F

from test_anisotropic_plans import aniso_oracle

pytestmark = pytest.mark.gpu

TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
STRIDES = [(1, 1, 1), (1, 2, 2), (2, 2, 2), (1, 2, 1)]


def _pad(c, m):
    return (c + m - 1) // m * m


def _lib():
    from dg_tta_amd import _lib
    return _lib.load()


def _check(rc, what):
    from dg_tta_amd._lib import check
    check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max()) / (float(b.abs().max()) + 1e-30)


@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("kd", [1, 3])
def test_conv_kernels_vs_torch(kd, stride, dt):
    _conv_case(kd, stride, dt, *((12, 32), (24, 40))[(kd + sum(stride)) % 2], 2, 6, 20, 28)


# output rows of >= 32 voxels: the 32-wide tile (TD x TH x TW = 4 x 4 x 32), with the W-parity staging where SW = 2 and the deepest
# halo (kd = 3) - the tile the level-1 / level-2 layers of a realistic anisotropic plan run on
@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("kd,stride", [(1, (1, 2, 2)), (3, (1, 2, 2)), (3, (1, 1, 1)), (1, (1, 1, 2))])
def test_conv_kernels_wide_tile_vs_torch(kd, stride, dt):
    _conv_case(kd, stride, dt, 24, 40, 1, 6, 10, 72)


def _conv_case(kd, stride, dt, cin, cout, B, D, H, W):
    lib = _lib()
    CP = 8 if dt == 0 else 16
    cinp, coutp = _pad(cin, CP), _pad(cout, CP)
    g = torch.Generator().manual_seed(100 * kd + 10 * sum(stride) + dt)
    q = lambda t: t.to(TDT[dt]).double()         # the values as stored
    x = q(torch.randn(B, cin, D, H, W, generator=g))
    w = torch.randn(cout, cin, kd, 3, 3, generator=g) / (cin * kd * 9) ** 0.5
    b = torch.randn(cout, generator=g)
    wq = q(w) if dt else w.double()
    xr, wr, br = x.clone().requires_grad_(), wq.clone().requires_grad_(), b.double().clone().requires_grad_()
    y_ref = F.conv3d(xr, wr, br, stride=stride, padding=(kd // 2, 1, 1))
    gy = q(torch.randn(y_ref.shape, generator=g))
    y_ref.backward(gy)
    Do, Ho, Wo = y_ref.shape[2:]
    st = _stream()
    # forward: x is a channel slice (row length ldx > Cin, offset xoff) of a wider buffer
    ldx, xoff = cinp + CP, CP
    xb = torch.zeros((B, D, H, W, ldx), dtype=TDT[dt], device="cuda")
    xb[..., xoff:xoff + cin] = x.permute(0, 2, 3, 4, 1).to(TDT[dt]).cuda()
    xp = xb.data_ptr() + xoff * xb.element_size()
    nb = lib.dgtta_conv3d_kpacked_bytes(kd, cinp, coutp, dt)
    wpack = torch.empty(nb, dtype=torch.uint8, device="cuda")
    wd, bd = w.cuda().contiguous(), b.cuda()
    _check(lib.dgtta_conv3d_kpack_weights(wd.data_ptr(), wpack.data_ptr(), kd, 3, 3, cin, cout, cinp, coutp, dt, st), "kpack")
    y = torch.empty((B, Do, Ho, Wo, cout), dtype=TDT[dt], device="cuda")
    _check(lib.dgtta_conv3d_fwd(xp, ldx, wpack.data_ptr(), bd.data_ptr(), y.data_ptr(), cout, None, B, cin, cout, cinp, coutp,
                                D, H, W, kd, *stride, dt, st), "conv3d_fwd")
    torch.cuda.synchronize()
    yr = y_ref.detach().permute(0, 2, 3, 4, 1)
    tol = {0: 2e-5, 1: 1.0 / 128, 2: 1.0 / 1024}[dt]          # test_gpu_conv_mfma.py's limits for the k3 kernels
    assert float((y.double().cpu() - yr).abs().max()) < tol * float(yr.abs().max()) + 1e-3 * (dt > 0) + 1e-4
    # data gradient into the channel slice: overwrite (the rest of the rows untouched), then accumulate onto it
    dy = gy.permute(0, 2, 3, 4, 1).contiguous().to(TDT[dt]).cuda()
    dxb = torch.randn((B, D, H, W, ldx), generator=g).to(TDT[dt]).cuda()
    dxp = dxb.data_ptr() + xoff * dxb.element_size()
    before = dxb.clone()
    ref = xr.grad.permute(0, 2, 3, 4, 1)
    for acc in (0, 1):
        _check(lib.dgtta_conv3d_dgrad(dy.data_ptr(), cout, wpack.data_ptr(), dxp, ldx, B, cin, cout, cinp, coutp, D, H, W, kd,
                                      *stride, acc, dt, st), "conv3d_dgrad")
        torch.cuda.synchronize()
        got = dxb[..., xoff:xoff + cin].double().cpu()
        want = ref * (1 + acc)
        assert float((got - want).abs().max()) < tol * float(want.abs().max()) + 1e-3 * (dt > 0) + 1e-4, f"dgrad accumulate={acc}"
        assert torch.equal(dxb[..., :xoff], before[..., :xoff]) and torch.equal(dxb[..., xoff + cin:], before[..., xoff + cin:])
    # weight / bias gradient, then accumulated once more
    nbw = lib.dgtta_conv3d_kwgrad_ws_bytes(B, cin, cout, D, H, W, kd, *stride)
    ws = torch.empty(nbw, dtype=torch.uint8, device="cuda")
    dw = torch.zeros((cout, cin, kd, 3, 3), device="cuda")
    db = torch.zeros(cout, device="cuda")
    wtol = 3e-5 if dt == 0 else 2e-2
    for k, acc in ((1, 0), (2, 1)):
        _check(lib.dgtta_conv3d_wgrad(xp, ldx, dy.data_ptr(), cout, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbw, B, cin, cout,
                                      D, H, W, kd, *stride, acc, dt, st), "conv3d_wgrad")
        torch.cuda.synchronize()
        assert _rel(dw, k * wr.grad) < wtol, f"wgrad accumulate={acc}: {_rel(dw, k * wr.grad):.3e}"
        assert torch.allclose(db.double().cpu(), k * br.grad, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("stride", [(1, 2, 2), (2, 2, 2), (1, 2, 1), (2, 1, 1)])
def test_transposed_conv_kernels_vs_torch(stride, dt):
    lib = _lib()
    cin, cout = 40, 24
    B, D, H, W = 2, 3, 10, 7
    g = torch.Generator().manual_seed(7 + sum(stride) + dt)
    q = lambda t: t.to(TDT[dt]).double()
    x = q(torch.randn(B, cin, D, H, W, generator=g))
    w = torch.randn(cin, cout, *stride, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g)
    wq = q(w) if dt else w.double()
    xr, wr, br = x.clone().requires_grad_(), wq.clone().requires_grad_(), b.double().clone().requires_grad_()
    y_ref = F.conv_transpose3d(xr, wr, br, stride=stride)
    gy = q(torch.randn(y_ref.shape, generator=g))
    y_ref.backward(gy)
    Do, Ho, Wo = y_ref.shape[2:]
    st = _stream()
    xd = x.permute(0, 2, 3, 4, 1).contiguous().to(TDT[dt]).cuda()
    wd, bd = w.cuda().contiguous(), b.cuda()
    # forward into the first half of a concat buffer (row length 2 C)
    out = torch.zeros((B, Do, Ho, Wo, 2 * cout), dtype=TDT[dt], device="cuda")
    nb = lib.dgtta_convT3d_s_fwd_ws_bytes(cin, cout, *stride, dt)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    _check(lib.dgtta_convT3d_s_fwd(xd.data_ptr(), cin, wd.data_ptr(), bd.data_ptr(), out.data_ptr(), 2 * cout, ws.data_ptr(), nb, B,
                                   cin, cout, D, H, W, *stride, dt, st), "convT3d_s_fwd")
    torch.cuda.synchronize()
    yr = y_ref.detach().permute(0, 2, 3, 4, 1)
    tol = {0: 2e-5, 1: 1.0 / 128, 2: 1.0 / 1024}[dt]
    assert float((out[..., :cout].double().cpu() - yr).abs().max()) < tol * float(yr.abs().max()) + 1e-3 * (dt > 0) + 1e-4
    assert not out[..., cout:].any()
    # backward from the first half of a concat gradient
    gc = torch.zeros((B, Do, Ho, Wo, 2 * cout), dtype=TDT[dt], device="cuda")
    gc[..., :cout] = gy.permute(0, 2, 3, 4, 1).to(TDT[dt]).cuda()
    nb = lib.dgtta_convT3d_s_bwd_ws_bytes(B, cin, cout, D, H, W, *stride)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dx = torch.empty((B, D, H, W, cin), dtype=TDT[dt], device="cuda")
    dw = torch.zeros_like(wd)
    db = torch.zeros_like(bd)
    wtol = 3e-5 if dt == 0 else 2e-2
    for k, acc in ((1, 0), (2, 1)):
        _check(lib.dgtta_convT3d_s_bwd(xd.data_ptr(), cin, gc.data_ptr(), 2 * cout, wd.data_ptr(), dx.data_ptr(), cin, dw.data_ptr(),
                                       db.data_ptr(), ws.data_ptr(), nb, B, cin, cout, D, H, W, *stride, acc, dt, st), "convT3d_s_bwd")
        torch.cuda.synchronize()
        ref = xr.grad.permute(0, 2, 3, 4, 1)
        assert float((dx.double().cpu() - ref).abs().max()) < tol * float(ref.abs().max()) + 1e-3 * (dt > 0) + 1e-4
        assert _rel(dw, k * wr.grad) < wtol
        assert torch.allclose(db.double().cpu(), k * br.grad, rtol=1e-5, atol=1e-4)


def test_unsupported_geometry_is_rejected():
    lib = _lib()
    t = torch.zeros(1 << 16, device="cuda")
    rc = lib.dgtta_conv3d_fwd(t.data_ptr(), 16, t.data_ptr(), None, t.data_ptr(), 16, None, 1, 16, 16, 16, 16, 4, 8, 8, 5, 1, 1, 1, 0,
                              _stream())
    assert rc == -2 and b"not supported" in lib.dgtta_last_error()
    rc = lib.dgtta_convT3d_s_fwd(t.data_ptr(), 16, t.data_ptr(), None, t.data_ptr(), 16, t.data_ptr(), 1 << 18, 1, 16, 16, 2, 2, 2,
                                 3, 2, 2, 0, _stream())
    assert rc == -2


# one weight-image pack serves both blobs: the kd = 3 blob of dgtta_conv3d_kpack_weights is the image region [imgF | imgB] of the
# 3x3x3 blob, which follows its [wf | wb] of 2 * 27 * CinP * CoutP elements
@pytest.mark.parametrize("dt", [0, 1, 2])
def test_kpack_kd3_is_the_image_region_of_pack_weights(dt):
    lib = _lib()
    cin, cout = 5, 12
    CP = 8 if dt == 0 else 16
    cinp, coutp = _pad(cin, CP), _pad(cout, CP)
    w = torch.randn(cout, cin, 3, 3, 3, generator=torch.Generator().manual_seed(11 + dt)).cuda().contiguous()
    st = _stream()
    nk, n3 = lib.dgtta_conv3d_kpacked_bytes(3, cinp, coutp, dt), lib.dgtta_conv3d_packed_bytes(cinp, coutp, dt)
    off = 2 * 27 * cinp * coutp * TDT[dt].itemsize
    assert nk > 0 and n3 == off + nk
    kblob = torch.full((nk,), 0xA5, dtype=torch.uint8, device="cuda")
    blob = torch.full((n3,), 0x5A, dtype=torch.uint8, device="cuda")
    _check(lib.dgtta_conv3d_kpack_weights(w.data_ptr(), kblob.data_ptr(), 3, 3, 3, cin, cout, cinp, coutp, dt, st), "kpack")
    _check(lib.dgtta_conv3d_pack_weights(w.data_ptr(), blob.data_ptr(), cin, cout, cinp, coutp, dt, st), "pack")
    torch.cuda.synchronize()
    assert torch.equal(kblob, blob[off:off + nk])
    assert kblob.view(TDT[dt]).count_nonzero() == w.to(TDT[dt]).count_nonzero() * 2      # every weight once per image, padding zero


POOLS =[[1, 1, 1], [1, 2, 2], [1, 2, 2], [2, 2, 2]]
POOLS_121 = [[1, 1, 1], [1, 2, 1], [1, 2, 2], [2, 2, 2]]
KERNELS = [[1, 3, 3], [1, 3, 3], [3, 3, 3], [3, 3, 3]]


def _cfg(pools):
    return dict(features=(8, 16, 24, 32), strides=tuple(tuple(p) for p in pools), kernel_sizes=tuple(tuple(k) for k in KERNELS),
                n_conv_enc=(2, 2, 2, 2), n_conv_dec=(2, 2, 2), in_channels=12, num_classes=5)


def _nets(cfg, adt, seed=3):
    from oracle import unet as ounet
    from dg_tta_amd.unet import HipPlainConvUNet
    om = ounet.perturb_affine(ounet.init_he(aniso_oracle(cfg), seed), seed + 1)
    hm = HipPlainConvUNet(cfg, act_dtype=adt)
    hm.load_state_dict(om.state_dict())
    return om, hm.cuda()


@pytest.mark.parametrize("pools,dtype", [(POOLS, "fp32"), (POOLS, "bf16"), (POOLS, "fp16"), (POOLS_121, "fp32"), (POOLS_121, "fp16")])
def test_network_forward_and_gradients_vs_oracle(pools, dtype):
    adt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    om, hm = _nets(_cfg(pools), adt)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 12, 8, 32, 48, generator=g)
    gout = torch.randn(2, 5, 8, 32, 48, generator=g)
    om32 = copy.deepcopy(om)        # fp32 reference: its distance from float64 is the conditioning of each gradient
    om32(x).backward(gout)
    om64 = om.double()
    y_ref = om64(x.double())
    y_ref.backward(gout.double())
    y = hm(x.cuda())
    y.backward(gout.cuda())
    torch.cuda.synchronize()
    y_ref = y_ref.detach()
    rng = float(y_ref.max() - y_ref.min())
    err = float((y.detach().double().cpu() - y_ref).abs().max())
    assert err < {"fp32": 2e-4, "bf16": 3e-2, "fp16": 4e-3}[dtype] * rng, f"{dtype}: logits err {err:.3e} (range {rng:.2f})"
    ref_grads, ref32 = dict(om64.named_parameters()), dict(om32.named_parameters())
    checked = 0
    for n, p in hm.named_parameters():
        gr = ref_grads[n].grad
        # a conv bias in front of InstanceNorm has an identically zero gradient: both sides hold rounding noise only
        if n.endswith("conv.bias") and "seg_layers" not in n and "transpconvs" not in n:
            continue
        if gr is None:          # the deep-supervision heads the forward does not evaluate
            assert p.grad is None, n
            continue
        got = p.grad.double().cpu()
        cos = float(F.cosine_similarity(got.flatten(), gr.flatten(), dim=0))
        if dtype == "fp32":
            # a pre-activation within ~1e-7 of the LeakyReLU kink takes the other slope in fp32 than in float64 (seen: one voxel
            # of the level-0 decoder block moves its channel's beta gradient by 0.7 %); the layers below inherit that, so the
            # limit is the fp32 reference's own error or 2e-2, whichever is larger, plus a cosine that a wrong kernel misses
            cond = _rel(ref32[n].grad, gr)
            assert _rel(got, gr) < max(15.0 * cond, 2e-2), f"fp32 grad {n}: {_rel(got, gr):.3e} (fp32 reference {cond:.3e})"
            assert cos > 0.9995, f"fp32 grad {n}: cosine {cos:.6f}"
        else:
            assert cos > (0.85 if dtype == "bf16" else 0.98), f"{dtype} grad {n}: cosine {cos:.4f}"
        checked += 1
    assert checked > 40


def test_tta_step_vs_oracle():
    """One TTA accumulation step (GIN -> affine warp -> MIND -> net -> inverse warp -> masked soft Dice -> backward) of a small
    anisotropic net, product path against oracle.tta.tta_step (as __graft_entry__.smoke does for an isotropic one)."""
    from dg_tta_amd import ops
    from dg_tta_amd.mind import MIND3D
    from oracle import gin as ogin, tta as otta
    om, hm = _nets(_cfg(POOLS), torch.float32, seed=7)
    sel = torch.tensor([0, 2, 3])
    hm.set_selected_classes(sel)
    D, H, W = 8, 32, 48
    torch.manual_seed(0)
    imgs = torch.randn(1, 1, D, H, W)

    def draws(seed):
        torch.manual_seed(seed)
        return dict(gin_draw=ogin.draw_gin_params(1), affine_draw=torch.randn(1, 3, 4), mind_noise=torch.randn(1, 12, D, H, W))

    da, db = draws(1), draws(2)
    ref_loss = otta.tta_step(om, imgs, sel, da, db, accum=1, backward=True)

    def branch(d):
        alpha, ks, kers, shifts = d["gin_draw"]
        x = ops.gin_chain(imgs.cuda(), alpha.cuda(), ks, [k.cuda() for k in kers], [s.cuda() for s in shifts])
        r, rinv = otta.rand_affine_from_draw(d["affine_draw"])
        x = ops.affine_warp(x, r.cuda(), padding_mode="border", tta_grid_algebra=True)
        y = hm(MIND3D()(x, d["mind_noise"].cuda()))
        return ops.affine_warp(y, rinv.cuda(), padding_mode="zeros", tta_grid_algebra=True)

    loss, _ = ops.consistency_loss(branch(da), branch(db), 1)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(ref_loss)) < 2e-4, f"loss {float(loss):.6f} vs oracle {float(ref_loss):.6f}"
    g_ref = om.decoder.seg_layers[-1].weight.grad
    gerr = float((hm.decoder.seg_layers[-1].weight.grad.cpu() - g_ref).abs().max()) / float(g_ref.abs().max())
    assert gerr < 1e-3, f"head weight grad rel err {gerr:.3e}"


REAL_CFG = dict(features=(32, 64, 128, 256, 320), strides=((1, 1, 1), (1, 2, 2), (1, 2, 2), (2, 2, 2), (2, 2, 2)),
                kernel_sizes=((1, 3, 3), (1, 3, 3), (3, 3, 3), (3, 3, 3), (3, 3, 3)), n_conv_enc=(2, 2, 2, 2, 2), n_conv_dec=(2, 2, 2, 2),
                in_channels=12, num_classes=105)
REAL_PATCH = (40, 160, 160)
_REAL = {}


def _real_oracle():
    """One TTA step of the realistic anisotropic plan on the CPU oracle (<= 16 threads), computed once for both storage types:
    (oracle model, images, selected classes, draws, loss, both branch outputs, per-class soft Dice)."""
    if not _REAL:
        from oracle import gin as ogin, tta as otta, unet as ounet
        torch.set_num_threads(min(16, torch.get_num_threads()))
        om = ounet.perturb_affine(ounet.init_he(aniso_oracle(REAL_CFG), 5), 6)
        sel = torch.tensor([0, 2, 3, 5, 8])
        torch.manual_seed(0)
        imgs = torch.randn(1, 1, *REAL_PATCH)

        def draws(seed):
            torch.manual_seed(seed)
            return dict(gin_draw=ogin.draw_gin_params(1), affine_draw=torch.randn(1, 3, 4), mind_noise=torch.randn(1, 12, *REAL_PATCH))

        da, db = draws(1), draws(2)
        with torch.no_grad():
            ta, tb = otta.calc_branch(om, imgs, sel, **da), otta.calc_branch(om, imgs, sel, **db)
            mask = (ta.sum(1, keepdim=True) > 0.0).float() * (tb.sum(1, keepdim=True) > 0.0).float()
            dice = otta.soft_dice_loss(ta.softmax(1) * mask, tb.softmax(1) * mask)
            loss = otta.consistency_loss(ta, tb)
        _REAL.update(om=om, imgs=imgs, sel=sel, da=da, db=db, loss=float(loss), ta=ta, tb=tb, dice=dice)
    return _REAL


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_tta_step_realistic_plan_vs_oracle(dtype):
    """One TTA step at the realistic anisotropic plan (patch 40 x 160 x 160, features 32..320, [1,3,3] kernels and (1,2,2) pools at
    the two high-resolution levels) against the CPU oracle, at DESIGN.md section 2's tolerances: fp32 loss within 1e-5 and identical
    labels where the oracle's top-2 margin exceeds 1e-3; fp16 loss and Dice within 1e-3."""
    from dg_tta_amd import ops
    from dg_tta_amd.mind import MIND3D
    from dg_tta_amd.unet import HipPlainConvUNet
    from oracle import tta as otta
    r = _real_oracle()
    adt = {"fp32": torch.float32, "fp16": torch.float16}[dtype]
    hm = HipPlainConvUNet(REAL_CFG, act_dtype=adt)
    hm.load_state_dict(r["om"].state_dict())
    hm = hm.cuda()
    hm.set_selected_classes(r["sel"])
    imgs = r["imgs"].cuda()

    def branch(d):
        alpha, ks, kers, shifts = d["gin_draw"]
        x = ops.gin_chain(imgs, alpha.cuda(), ks, [k.cuda() for k in kers], [s.cuda() for s in shifts])
        rr, rinv = otta.rand_affine_from_draw(d["affine_draw"])
        x = ops.affine_warp(x, rr.cuda(), padding_mode="border", tta_grid_algebra=True)
        y = hm(MIND3D()(x, d["mind_noise"].cuda()))
        return ops.affine_warp(y, rinv.cuda(), padding_mode="zeros", tta_grid_algebra=True)

    ta, tb = branch(r["da"]), branch(r["db"])
    loss, dice = ops.consistency_loss(ta, tb, 1)
    (loss * hm.loss_scale).backward()
    torch.cuda.synchronize()
    err = abs(float(loss) - r["loss"])
    g = hm.decoder.seg_layers[-1].weight.grad
    assert g is not None and bool(torch.isfinite(g).all())
    if dtype == "fp32":
        assert err < 1e-5, f"fp32 loss {float(loss):.7f} vs oracle {r['loss']:.7f}"
        for got, ref in ((ta, r["ta"]), (tb, r["tb"])):
            top2 = ref.topk(2, dim=1).values
            safe = (top2[:, 0] - top2[:, 1]) > 1e-3
            assert torch.equal(got.detach().cpu().argmax(1)[safe], ref.argmax(1)[safe])
    else:
        assert err < 1e-3, f"fp16 loss {float(loss):.6f} vs oracle {r['loss']:.6f}"
        derr = float((dice.detach().cpu() - r["dice"]).abs().max())
        assert derr < 1e-3, f"fp16 Dice err {derr:.2e}"


def test_prepare_and_run_tta_cli_anisotropic_plans(tmp_path, monkeypatch):
    """`dgtta prepare_tta` + `run_tta` with a model folder whose plans are anisotropic ([1,3,3] kernels, (1,2,2) pools) and a seeded
    checkpoint of that shape: the predictions come back in each case's original geometry."""
    import json
    from pathlib import Path
    import numpy as np
    from dg_tta_amd.run import DGTTAProgram
    from dg_tta_amd.synthetic import he_init_, synthetic_case
    from dg_tta_amd.tta.nifti_io import read_nifti, write_nifti
    from dg_tta_amd.tta.nnunet_utils import unet_cfg_from_plans
    from dg_tta_amd.unet import HipPlainConvUNet
    raw = tmp_path / "raw" / "Dataset804_Target"
    (raw / "imagesTs").mkdir(parents=True)
    (raw / "labelsTs").mkdir()
    case = synthetic_case(size=64, k=3, seed=5)
    img = (case[0] * 300.0).numpy()
    lab = torch.cat([(case[1:].sum(0, keepdim=True) < 1).float(), case[1:]]).argmax(0).numpy().astype(np.int16)
    write_nifti(raw / "imagesTs" / "ct01_0000.nii.gz", img.astype(np.float32), spacing=(1.5, 1.5, 1.5))
    write_nifti(raw / "labelsTs" / "ct01.nii.gz", lab, spacing=(1.5, 1.5, 1.5))
    img2 = np.zeros((40, 76, 74), np.float32)          # thick slices (2.5 x 1.1 x 1.1 mm), zero border cropped by preprocessing
    lab2 = np.zeros((40, 76, 74), np.int16)
    img2[3:37, 6:70, 5:69] = img[:34] + 700.0
    lab2[3:37, 6:70, 5:69] = lab[:34]
    write_nifti(raw / "imagesTs" / "ct02_0000.nii.gz", img2, spacing=(1.1, 1.1, 2.5))
    write_nifti(raw / "labelsTs" / "ct02.nii.gz", lab2, spacing=(1.1, 1.1, 2.5))
    json.dump({"labels": {"background": 0, "liver": 1, "spleen": 2, "my_organ": 3}}, open(raw / "dataset.json", "w"))
    root = tmp_path / "dgroot"
    root.mkdir()
    for k, v in {"nnUNet_raw": str(tmp_path / "raw"), "nnUNet_results": str(tmp_path / "res"),
                 "nnUNet_preprocessed": str(tmp_path / "pre"), "DG_TTA_ROOT": str(root)}.items():
        monkeypatch.setenv(k, v)
    DGTTAProgram(["dgtta", "prepare_tta", "TS104_GIN_MIND", "804"])
    plan_dir = root / "plans" / "Pretrained_TS104_GIN_MIND_at_Dataset804_Target" / "nnUNetTrainer_GIN_MIND__3d_fullres" / "fold_0"
    plan = json.load(open(plan_dir / "tta_plan.json"))
    weights = Path(plan["pretrained_weights_filepath"])
    # the model folder's plans rewritten to an anisotropic 3d_fullres configuration, checkpoint of that shape
    mplans = json.load(open(weights.parents[1] / "plans.json"))
    conf = mplans["configurations"]["3d_fullres"]
    conf.update(patch_size=[32, 64, 64], pool_op_kernel_sizes=[[1, 1, 1], [1, 2, 2], [1, 2, 2], [2, 2, 2], [2, 2, 2]],
                conv_kernel_sizes=[[1, 3, 3], [1, 3, 3], [3, 3, 3], [3, 3, 3], [3, 3, 3]],
                n_conv_per_stage_encoder=[2] * 5, n_conv_per_stage_decoder=[2] * 4)
    json.dump(mplans, open(weights.parents[1] / "plans.json", "w"))
    dsj = json.load(open(weights.parents[1] / "dataset.json"))
    cfg, patch = unet_cfg_from_plans(mplans, dsj, "3d_fullres", 12)
    assert patch == [32, 64, 64] and cfg["kernel_sizes"][0] == (1, 3, 3)
    net = he_init_(HipPlainConvUNet(cfg), seed=7)
    torch.save({"network_weights": net.state_dict(), "trainer_name": "nnUNetTrainer_GIN_MIND"}, weights)
    plan.update(epochs=1, start_tta_at_epoch=0, patches_to_be_accumulated=2, ensemble_count=1)
    json.dump(plan, open(plan_dir / "tta_plan.json", "w"), indent=4)
    DGTTAProgram(["dgtta", "run_tta", "TS104_GIN_MIND", "804", "--device", "cuda:0"])
    runs = sorted((root / "results" / "Pretrained_TS104_GIN_MIND_at_Dataset804_Target" /
                   "nnUNetTrainer_GIN_MIND__3d_fullres" / "fold_0").iterdir())
    assert len(runs) == 1
    out = runs[0] / "tta_outputTs"
    state = torch.load(out / "ct01__ensemble_idx_0_tta_parameters.pt", map_location="cpu")[0]
    assert {k: tuple(v.shape) for k, v in state.items()} == {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert sum(int(not torch.equal(state[k], v)) for k, v in net.state_dict().items()) > 30      # adapted
    seg, hdr = read_nifti(out / "ct01.nii.gz")
    assert seg.shape == (64, 64, 64) and hdr["pixdim"] == pytest.approx((1.5, 1.5, 1.5))
    seg2, hdr2 = read_nifti(out / "ct02.nii.gz")
    assert seg2.shape == (40, 76, 74) and hdr2["pixdim"] == pytest.approx((1.1, 1.1, 2.5))
    outside = np.ones(seg2.shape, bool)
    outside[3:37, 6:70, 5:69] = False
    assert (seg2[outside] == 0).all()
    assert set(np.unique(seg2).tolist()) <= {0, 1, 2}
