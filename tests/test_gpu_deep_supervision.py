"""Deep supervision on the GPU: the head kernels for more than 32 input channels and the accumulating data gradient through the
C ABI, DC+CE against a strided view of the full-resolution label map, and the network / loss / trainer against plain torch on
the CPU (F.conv3d in float64, a restatement of DC+CE on labels[:, sd//2::sd, sh//2::sh, sw//2::sw], the repo's torch
restatement of the network extended by the auxiliary heads)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_anisotropic_plans import aniso_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}


# ------------------------------------------------------------------------------------------------ head kernels, C ABI
@pytest.mark.parametrize("cin,nsel,dt,use_sel", [(c, n, dt, False) for c in (64, 96, 320) for n in (3, 105) for dt in (1, 2)] +
                         [(16, 105, 0, False), (16, 3, 0, False), (64, 40, 2, True), (16, 40, 0, True)])
def test_head_kernels_vs_float64(cin, nsel, dt, use_sel):
    _check_head_kernels(cin, nsel, dt, use_sel, (6, 10, 14))


@pytest.mark.parametrize("cin,dt", [(64, 2), (128, 1)])
def test_head_kernels_many_tiles_and_splits(cin, dt):
    """The same checks on B = 2 volumes of 22 x 40 x 41 voxels: 72160 rows are 1127.5 tiles of 64 rows, more than the 1024
    workgroups the forward and the data gradient launch at the most - some workgroups take a second tile through the buffer they
    just multiplied from - and 36 splits of the weight gradient (32 tiles each, the last one 8 with a half-filled tile at the end),
    added up by the split reduction.  Two 32-row halves, four (Cin 128: eight) 32-channel blocks."""
    _check_head_kernels(cin, 105, dt, False, (22, 40, 41))


def _check_head_kernels(cin, nsel, dt, use_sel, vol):
    """dgtta_seghead_fwd / dgtta_seghead_bwd_acc on B = 2 volumes of `vol` voxels (6 x 10 x 14: 1680 rows, no multiple of any tile), x rows
    read with a pitch of Cin + 32: the matrix-core path (16-bit storage, Cin a multiple of 32) and the general kernels (fp32, Cin =
    16) against float64 on the same rounded inputs.  Limits: those of the Cin = 32 head test of the same storage type
    (tests/test_gpu_conv_mfma.py::test_head_fast_paths) - the same arithmetic with a longer K."""
    from dg_tta_amd import _lib
    from dg_tta_amd._lib import check, ptr, stream_of
    lib = _lib.load()
    g = torch.Generator().manual_seed(cin * 1000 + nsel * 10 + dt + vol[0])
    tdt = TDT[dt]
    B, V, ncls, ldx = 2, vol[0] * vol[1] * vol[2], 105, cin + 32
    rows = B * V
    xbuf = torch.randn(rows, ldx, generator=g).to(tdt).to(DEV)
    w = torch.randn(ncls, cin, generator=g).to(DEV)
    bias = torch.randn(ncls, generator=g).to(DEV)
    sel = torch.randperm(ncls, generator=g)[:nsel].int().to(DEV) if use_sel else None      # a non-contiguous subset of the rows
    if not use_sel and nsel != ncls:
        w, bias, ncls = w[:nsel].contiguous(), bias[:nsel].contiguous(), nsel
    wsel = (w if sel is None else w[sel.long()]).double().cpu()
    bsel = (bias if sel is None else bias[sel.long()]).double().cpu()
    x64 = xbuf[:, :cin].double().cpu()
    # ---- forward
    out = torch.full((rows, nsel), float("nan"), device=DEV)
    check(lib.dgtta_seghead_fwd(ptr(xbuf), ldx, ptr(w), ptr(bias), ptr(sel), nsel, ptr(out), 1, nsel, B, cin, V, dt, stream_of()),
          "head fwd")
    ref = F.conv3d(x64.t().reshape(1, cin, rows, 1, 1), wsel.reshape(nsel, cin, 1, 1, 1), bsel)[0, :, :, 0, 0].t()
    err = float((out.double().cpu() - ref).abs().max())
    print(f"\nhead fwd Cin {cin} nsel {nsel} dt {dt}: err {err:.3e} / max {float(ref.abs().max()):.2f}")
    assert err < 2e-5 * float(ref.abs().max()) + 1e-5
    # ---- backward: dx += dout . W on rows that hold random values, then dx = on NaN-filled rows
    dout = torch.randn(rows, nsel, generator=g).to(DEV)
    dx_ref = dout.double().cpu() @ wsel
    dx0 = torch.randn(rows, cin, generator=g).to(tdt).to(DEV)
    nb = lib.dgtta_seghead_bwd_ws_bytes(B, cin, nsel, V)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    tol = 2e-5 if dt == 0 else 1e-2
    wtol = 3e-5 if dt == 0 else 2e-2
    dw_ref = dout.double().cpu().t() @ x64
    db_ref = dout.double().cpu().sum(0)

    def bwd(dx, dw, db, acc, acc_dx):
        check(lib.dgtta_seghead_bwd_acc(ptr(xbuf), ldx, ptr(dout), nsel, ptr(w), ptr(sel), nsel, ptr(dx), cin, ptr(dw), ptr(db),
                                        ptr(ws), nb, B, cin, V, acc, acc_dx, dt, stream_of()), "head bwd")
    dx = dx0.clone()
    dw, db = torch.full((nsel, cin), float("nan"), device=DEV), torch.full((nsel,), float("nan"), device=DEV)
    bwd(dx, dw, db, 0, 1)
    want = dx0.double().cpu() + dx_ref
    e_acc = float((dx.double().cpu() - want).abs().max())
    assert e_acc < tol * float(want.abs().max()) + 1e-5, e_acc
    e_w = float((dw.double().cpu() - dw_ref).abs().max())
    assert e_w < wtol * float(dw_ref.abs().max()) + 1e-4, e_w
    assert torch.allclose(db.double().cpu(), db_ref, rtol=1e-5, atol=1e-4)
    dx2 = torch.full((rows, cin), float("nan"), device=DEV).to(tdt)
    bwd(dx2, dw, db, 1, 0)                # every element of dx is written; dw / db accumulate
    e_plain = float((dx2.double().cpu() - dx_ref).abs().max())
    assert e_plain < tol * float(dx_ref.abs().max()) + 1e-5, e_plain
    assert float((dw.double().cpu() - 2 * dw_ref).abs().max()) < 2 * wtol * float(dw_ref.abs().max()) + 2e-4
    assert torch.allclose(db.double().cpu(), 2 * db_ref, rtol=1e-5, atol=2e-4)
    print(f"head bwd Cin {cin} nsel {nsel} dt {dt}: dx+= {e_acc:.3e}, dx= {e_plain:.3e} / {float(dx_ref.abs().max()):.2f}, "
          f"dw {e_w:.3e} / {float(dw_ref.abs().max()):.2f}")
    # the existing entry point is the same call without the flag
    dx3 = torch.full((rows, cin), float("nan"), device=DEV).to(tdt)
    check(lib.dgtta_seghead_bwd(ptr(xbuf), ldx, ptr(dout), nsel, ptr(w), ptr(sel), nsel, ptr(dx3), cin, None, None, ptr(ws), nb, B,
                                cin, V, 0, dt, stream_of()), "head bwd (plain)")
    assert torch.equal(dx3, dx2)


# ------------------------------------------------------------------------------------------------ strided DC+CE
def _dc_ce_torch(logits, labels, strides, smooth=1e-5):
    """DC+CE (per-sample soft Dice without background + cross-entropy, labels outside [0, C) ignored) of low-resolution logits
    against the strided view of the full-resolution label map [B, D, H, W]."""
    sd, sh, sw = strides
    lab = labels[:, sd // 2::sd, sh // 2::sh, sw // 2::sw].unsqueeze(1)
    c = logits.shape[1]
    valid = (lab >= 0) & (lab < c)
    safe = lab.clamp(0, c - 1)
    ce = -(torch.log_softmax(logits, 1).gather(1, safe) * valid).sum() / valid.sum()
    p = logits.softmax(1) * valid
    oh = F.one_hot(safe[:, 0], c).permute(0, 4, 1, 2, 3).to(logits.dtype) * valid
    dice = (2 * (p * oh).sum((2, 3, 4)) + smooth) / (p.sum((2, 3, 4)) + oh.sum((2, 3, 4)) + smooth)
    return ce - dice[:, 1:].mean(), ce, dice


def _labels(c, gen, shape=(8, 16, 24)):
    labels = torch.randint(0, c, (2, *shape), generator=gen)
    labels[0, 1, :, :5] = -1                       # ignored
    labels[1, :, 3, 2:9] = c + 5                   # ignored
    labels[0][labels[0] == c - 1] = 0              # a class absent from one sample
    return labels


@pytest.mark.parametrize("c", [3, 105])
@pytest.mark.parametrize("shape,strides", [((4, 8, 12), (2, 2, 2)), ((8, 8, 12), (1, 2, 2)), ((2, 4, 6), (4, 4, 4))])
def test_strided_dice_ce_matches_torch(c, shape, strides):
    """dgtta_dice_ce_ds_fwd / _bwd: loss3, dice and the logit gradient against the torch restatement's autograd, at the limits of
    tests/test_pretraining.py::test_dice_ce_loss_matches_torch."""
    from dg_tta_amd import _lib
    from dg_tta_amd._lib import check, ptr, stream_of
    lib = _lib.load()
    gen = torch.Generator().manual_seed(c * 7 + strides[0])
    labels = _labels(c, gen)
    logits = (torch.randn(2, c, *shape, generator=gen) * 3).requires_grad_(True)
    ref, ce, dice = _dc_ce_torch(logits, labels, strides)
    (ref * 0.37).backward()
    d, h, w = shape
    x = logits.detach().permute(0, 2, 3, 4, 1).contiguous().to(DEV)          # [B][d][h][w][C]
    lab = labels.to(DEV)
    loss3, dc = torch.empty(3, device=DEV), torch.empty(2, c, device=DEV)
    nb = lib.dgtta_dice_ce_ds_ws_bytes(2, c, d, h, w)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    check(lib.dgtta_dice_ce_ds_fwd(ptr(x), c, ptr(lab), ptr(loss3), ptr(dc), ptr(ws), nb, 2, c, d, h, w, *strides, 1e-5, 0,
                                   stream_of()), "ds fwd")
    gs = torch.tensor([0.5], device=DEV)
    grad = torch.full_like(x, float("nan"))
    check(lib.dgtta_dice_ce_ds_bwd(ptr(x), c, ptr(lab), ptr(ws), 0.74, ptr(gs), ptr(grad), c, 2, c, d, h, w, *strides, stream_of()),
          "ds bwd")
    assert abs(float(loss3[0]) - float(ref)) < 2e-5 * max(1.0, abs(float(ref)))
    assert abs(float(loss3[1]) - float(ce)) < 2e-5 * max(1.0, float(ce))
    assert abs(float(loss3[0]) - float(loss3[1]) - float(loss3[2])) < 1e-6
    assert (dc.cpu() - dice.detach()).abs().max() < 2e-5
    gerr = (grad.permute(0, 4, 1, 2, 3).cpu() - logits.grad).abs().max() / logits.grad.abs().max()
    assert float(gerr) < 2e-4, float(gerr)


@pytest.mark.parametrize("c", [3, 105])
def test_strided_dice_ce_with_unit_strides_is_the_plain_loss(c):
    from dg_tta_amd import ops
    gen = torch.Generator().manual_seed(c)
    labels = _labels(c, gen).to(DEV)
    logits = (torch.randn(2, c, 8, 16, 24, generator=gen) * 3).to(DEV)
    a = logits.clone().requires_grad_(True)
    la, da, pa = ops.dice_ce_loss(a, labels)
    (la * 0.37).backward()
    b = logits.clone().requires_grad_(True)
    lb, db, pb = ops._DiceCEStrided.apply(b, labels, (1, 1, 1), 1e-5, False)
    (lb * 0.37).backward()
    assert torch.equal(la, lb) and torch.equal(da, db) and torch.equal(pa, pb) and torch.equal(a.grad, b.grad)
    assert float(a.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ network
ISO_CFG = dict(features=(32, 64, 128), strides=(1, 2, 2), n_conv_enc=(2, 2, 2), n_conv_dec=(2, 2), in_channels=12, num_classes=11)
ANISO_CFG = dict(features=(8, 16, 24), strides=((1, 1, 1), (1, 2, 2), (2, 2, 2)), kernel_sizes=((1, 3, 3), (3, 3, 3), (3, 3, 3)),
                 n_conv_enc=(2, 2, 2), n_conv_dec=(2, 2), in_channels=12, num_classes=11)
CASES = {"iso": (ISO_CFG, (16, 16, 16)), "aniso": (ANISO_CFG, (8, 16, 16))}


def _oracle_outputs(om, x):
    """The torch restatement of the network, extended by the auxiliary heads: logits, highest resolution first."""
    skips = om.encoder(x)
    dec, y, outs = om.decoder, skips[-1], []
    for s in range(len(dec.stages)):
        y = dec.stages[s](torch.cat((dec.transpconvs[s](y), skips[-(s + 2)]), 1))
        outs.append(dec.seg_layers[s](y))
    return outs[::-1]


# The issue's two configurations have three stages, i.e. TWO outputs, and nnU-Net's default weights for two outputs are [1, 0]
# (the lowest resolution is always dropped): the whole-network comparisons therefore pass explicit weights, so that the
# auxiliary head takes part; the default weights on a net with three outputs are covered by the test after them.
WTS = (2.0 / 3.0, 1.0 / 3.0)


def _oracle_loss(om, x, labels):
    outs = _oracle_outputs(om, x)
    wts = WTS
    loss = 0.0
    for o, wt in zip(outs, wts):
        if wt:
            st = tuple(f // s for f, s in zip(labels.shape[1:], o.shape[2:]))
            loss = loss + wt * _dc_ce_torch(o, labels, st)[0]
    return outs, loss


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(oracle state dict, input, labels, float64 outputs / loss / gradients, fp32 oracle's gradients), computed once per cfg."""
    from oracle import unet as ounet
    cfg, patch = CASES[case]
    om = aniso_oracle(cfg) if "kernel_sizes" in cfg else ounet.PlainConvUNetOracle(cfg)
    om = ounet.perturb_affine(ounet.init_he(om, 3), 4)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for s in om.decoder.seg_layers:                 # (He init leaves head biases at zero)
            s.bias.add_(0.1 * torch.randn(s.bias.shape, generator=g))
    x = torch.randn(2, 12, *patch, generator=g)
    labels = torch.randint(0, 11, (2, *patch), generator=g)
    labels[0, 0, :2] = -1
    labels[1][labels[1] == 7] = 0
    sd = copy.deepcopy(om.state_dict())
    om32 = copy.deepcopy(om)
    _oracle_loss(om32, x, labels)[1].backward()
    g32 = {n: p.grad for n, p in om32.named_parameters()}
    om64 = om.double()
    outs, loss = _oracle_loss(om64, x.double(), labels)
    loss.backward()
    g64 = {n: p.grad for n, p in om64.named_parameters()}
    return sd, x, labels, [o.detach() for o in outs], float(loss), g64, g32


def _hip_net(case, adt, **kw):
    from dg_tta_amd.unet import HipPlainConvUNet
    hm = HipPlainConvUNet(CASES[case][0], act_dtype=adt, **kw)
    hm.load_state_dict(_reference(case)[0])
    return hm.to(DEV)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / (float(b.double().abs().max()) + 1e-30)


@pytest.mark.parametrize("case,dtype", [("iso", "fp32"), ("iso", "fp16"), ("aniso", "fp32")])
def test_network_outputs_loss_and_gradients_vs_torch(case, dtype):
    """All outputs, the weighted loss and the gradient of EVERY parameter (the auxiliary heads' included, and non-zero) against
    the float64 torch restatement; limits of tests/test_gpu_full_topology.py for the storage type."""
    from dg_tta_amd import ops
    adt = {"fp32": torch.float32, "fp16": torch.float16}[dtype]
    sd, x, labels, outs_ref, loss_ref, g64, g32 = _reference(case)
    hm = _hip_net(case, adt, deep_supervision=True)
    outs = hm(x.to(DEV))
    assert isinstance(outs, tuple) and len(outs) == len(outs_ref) == 2
    for o, r in zip(outs, outs_ref):
        assert tuple(o.shape) == tuple(r.shape)
        rng = float(r.max() - r.min())
        err = float((o.detach().double().cpu() - r).abs().max())
        assert err < {"fp32": 2e-4, "fp16": 4e-3}[dtype] * rng, f"{dtype} output {tuple(r.shape)}: err {err:.3e} (range {rng:.2f})"
    loss, per_scale = ops.deep_supervision_loss(outs, labels.to(DEV), weights=WTS)
    assert len(per_scale) == 2 and abs(float(loss) - sum(w * float(l) for w, l in zip(WTS, per_scale))) < 1e-6
    l_def, per_def = ops.deep_supervision_loss(outs, labels.to(DEV))      # default weights of two outputs: [1, 0]
    assert per_def[1] is None and float(l_def) == float(per_def[0])
    assert abs(float(loss) - loss_ref) < {"fp32": 2e-5, "fp16": 2e-4}[dtype] * max(1.0, abs(loss_ref)), (float(loss), loss_ref)
    scale = float(hm.loss_scale)
    torch.autograd.backward(loss, grad_tensors=torch.full((), scale, device=DEV))
    torch.cuda.synchronize()
    checked = 0
    for n, p in hm.named_parameters():
        gr = g64[n]
        if n.endswith("conv.bias") and "seg_layers" not in n and "transpconvs" not in n:
            continue        # a conv bias in front of InstanceNorm: identically zero gradient, rounding noise on both sides
        assert gr is not None and float(gr.abs().max()) > 0, n
        if "seg_layers" in n:
            assert float(p.grad.abs().max()) > 0, n      # the auxiliary head is trained
        got = p.grad.double().cpu() / scale
        cos = float(F.cosine_similarity(got.flatten(), gr.flatten(), dim=0))
        if dtype == "fp32":
            cond = _rel(g32[n], gr)
            assert _rel(got, gr) < 15.0 * cond + 1e-3, f"fp32 grad {n}: {_rel(got, gr):.3e} (fp32 reference {cond:.3e})"
            assert cos > 0.9995, f"fp32 grad {n}: cosine {cos:.6f}"
        else:
            assert torch.isfinite(got).all() and cos > 0.98, f"fp16 grad {n}: cosine {cos:.5f}"
        checked += 1
    assert checked > 30


def test_three_scales_weights_and_nonzero_auxiliary_gradients():
    """A 4-stage net (3 outputs, weights [2/3, 1/3, 0]): the loss is the weighted sum of its scales, the heads of the two upper
    resolutions get a non-zero gradient, the head of the lowest none."""
    from dg_tta_amd import ops
    from dg_tta_amd.synthetic import he_init_
    from dg_tta_amd.unet import HipPlainConvUNet
    cfg = dict(features=(8, 16, 32, 64), strides=(1, 2, 2, 2), n_conv_enc=(1, 1, 1, 1), n_conv_dec=(1, 1, 1), in_channels=12,
               num_classes=5)
    net = he_init_(HipPlainConvUNet(cfg, deep_supervision=True), seed=2).to(DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 12, 16, 16, 16, generator=g).to(DEV)
    labels = torch.randint(0, 5, (2, 1, 16, 16, 16), generator=g).to(DEV)
    outs = net(x)
    assert [tuple(o.shape[2:]) for o in outs] == [(16, 16, 16), (8, 8, 8), (4, 4, 4)]
    loss, per = ops.deep_supervision_loss(outs, labels)
    assert per[2] is None and abs(float(loss) - (2 / 3 * float(per[0]) + 1 / 3 * float(per[1]))) < 1e-6
    for o, st in zip(outs[:2], [(1, 1, 1), (2, 2, 2)]):
        ref = _dc_ce_torch(o.detach().cpu().double(), labels[:, 0].cpu(), st)[0]
        assert abs(float(per[0 if st == (1, 1, 1) else 1]) - float(ref)) < 2e-5
    loss.backward()
    segs = net.decoder.seg_layers
    assert float(segs[2].weight.grad.abs().max()) > 0 and float(segs[1].weight.grad.abs().max()) > 0
    assert float(segs[1].bias.grad.abs().max()) > 0
    assert segs[0].weight.grad is None or float(segs[0].weight.grad.abs().max()) == 0.0
    # only an auxiliary output in the loss: the full-resolution head gets zeros, everything below still a gradient
    net.zero_grad(set_to_none=True)
    outs = net(x)
    ops.deep_supervision_loss(outs, labels, weights=[0.0, 1.0, 0.0])[0].backward()
    assert float(segs[1].weight.grad.abs().max()) > 0 and float(segs[2].weight.grad.abs().max()) == 0.0
    assert float(net.encoder.stages[0][0].convs[0].conv.weight.grad.abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_main_loss_only_is_the_plain_network_bit_for_bit(dtype):
    """With only element 0 in the loss every gradient equals the deep_supervision=False run bit for bit (nothing is launched for
    an unused output); with the flag off the output is element 0 of the flag-on forward, bit for bit, and a tensor."""
    from dg_tta_amd import ops
    _, x, labels, *_ = _reference("iso")
    xs, lab = x.to(DEV), labels.to(DEV)
    off, on = _hip_net("iso", dtype), _hip_net("iso", dtype, deep_supervision=True)
    y_off = off(xs)
    y_on = on(xs)
    assert isinstance(y_off, torch.Tensor) and isinstance(y_on, tuple)
    assert torch.equal(y_off, y_on[0])
    ops.dice_ce_loss(y_off, lab)[0].backward()
    ops.dice_ce_loss(y_on[0], lab)[0].backward()
    torch.cuda.synchronize()
    for (n, a), (_, b) in zip(off.named_parameters(), on.named_parameters()):
        if a.grad is None:
            assert b.grad is None or float(b.grad.abs().max()) == 0.0, n
            assert "seg_layers.0" in n
        else:
            assert torch.equal(a.grad, b.grad), n
    on.deep_supervision = False            # a plain attribute: toggled after construction
    assert torch.equal(on(xs), y_off)


def test_fusion_contexts_refuse_deep_supervision():
    on = _hip_net("iso", torch.float16, deep_supervision=True)
    th = torch.eye(3, 4).repeat(2, 1, 1)
    with pytest.raises(ValueError, match="deep_supervision"):
        with on.fuse_output_warp(th.to(DEV), th):
            pass
    acc, nsum, gauss = torch.zeros(16, 16, 16, 11, device=DEV), torch.zeros(16, 16, 16, device=DEV), torch.ones(16, 16, 16, device=DEV)
    with pytest.raises(ValueError, match="deep_supervision"):
        with on.fuse_window_accumulate(acc, nsum, gauss, [(0, 0, 0)]):
            pass
    with pytest.raises(ValueError, match="deep_supervision"):
        with on.fuse_window_feature_accumulate(torch.zeros(16, 16, 16, 32, device=DEV), nsum, gauss, [(0, 0, 0)]):
            pass
    # switched on INSIDE a context: the forward refuses
    on.deep_supervision = False
    with on.fuse_output_warp(th.to(DEV), th):
        on.deep_supervision = True
        with pytest.raises(ValueError, match="deep_supervision"):
            on(torch.zeros(2, 12, 16, 16, 16, device=DEV))


def test_pretraining_with_deep_supervision():
    """pretrain_supervised(deep_supervision=True): 3 steps on two synthetic 24^3 cases - finite losses, the flag restored, the
    auxiliary head trained (this cfg has two outputs, whose default weights are [1, 0]: explicit weights bring the second one
    in; with the defaults the lowest head stays as it was); deep_supervision=False is the call without the argument (same seed,
    same weights), also on a net whose flag was on before the call."""
    from dg_tta_amd.pretraining.hooks import register_dg_hooks
    from dg_tta_amd.pretraining.supervised import pretrain_supervised
    from dg_tta_amd.synthetic import atlas_case, he_init_
    from dg_tta_amd.tta.torch_utils import release_resident
    from dg_tta_amd.unet import HipPlainConvUNet
    from dg_tta_amd.utils import disable_internal_augmentation
    cases = [atlas_case(24, 4, s, "source") for s in range(2)]
    lut = torch.tensor([0, 3, 8, 2, 5])

    def train(net_flag=False, **kw):
        net = he_init_(HipPlainConvUNet(ISO_CFG, deep_supervision=net_flag), seed=7)
        handles = register_dg_hooks(net, "nnUNetTrainer_GIN_MIND")
        net = net.to(DEV)
        before = copy.deepcopy(net.state_dict())
        torch.manual_seed(5)
        torch.cuda.manual_seed(5)
        np.random.seed(5)
        losses = pretrain_supervised(net, cases, [16, 16, 16], lut, steps=3, batch=2, lr=3e-3, device=DEV, **kw)
        for h in handles:
            h.remove()
        return net, before, losses
    try:
        net, before, losses = train(deep_supervision=True, ds_weights=WTS)
        assert losses.shape == (3,) and torch.isfinite(losses).all()
        assert net.deep_supervision is False
        after = net.state_dict()
        assert not torch.equal(after["decoder.seg_layers.0.weight"], before["decoder.seg_layers.0.weight"])
        assert not torch.equal(after["decoder.seg_layers.1.weight"], before["decoder.seg_layers.1.weight"])
        net, before, losses = train(deep_supervision=True)            # nnU-Net's weights: the lowest resolution is not trained
        assert torch.isfinite(losses).all() and net.deep_supervision is False
        assert torch.equal(net.state_dict()["decoder.seg_layers.0.weight"], before["decoder.seg_layers.0.weight"])
        assert not torch.equal(net.state_dict()["decoder.seg_layers.1.weight"], before["decoder.seg_layers.1.weight"])
        n0, b0, l0 = train()
        n1, _, l1 = train(deep_supervision=False)
        assert torch.equal(l0, l1)
        for k, v in n0.state_dict().items():
            assert torch.equal(v, n1.state_dict()[k]), k
        assert torch.equal(n0.state_dict()["decoder.seg_layers.0.weight"], b0["decoder.seg_layers.0.weight"])      # untrained without
        n2, _, l2 = train(net_flag=True, deep_supervision=False)      # a net that came with the flag on: off for the duration
        assert n2.deep_supervision is True and torch.equal(l0, l2)
        for k, v in n0.state_dict().items():
            assert torch.equal(v, n2.state_dict()[k]), k
    finally:
        disable_internal_augmentation()
        release_resident()
