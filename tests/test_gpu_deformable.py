"""GPU tests of spatial_aug_type="deformable" (csrc/deform.hip and its wiring).

Tolerances.  The kernels differ from torch's fp32 only in contraction and summation order, so every kernel comparison is
measured against the fp64 CPU restatement (tests/deformable_ref.py) and bounded by FACTOR = 4 times the fp32 CPU restatement's
own distance to fp64 on the same input (both are computed here and printed).  No voxel is left out; the zero-padded share of
the logits warp (about 1 %) must be exactly 0.  The backward of the dense sampler sums with fp32 atomics: the same rule holds
for it, whatever the order of arrival.  The assembled step inherits the bounds of the existing step tests (the network
kernels dominate its error): |loss| 2e-4, head-weight gradient 1e-3 of its maximum (as __graft_entry__.smoke)."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import deformable_ref as dref
from conftest import load_golden, SMALL_CFG, state_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 4.0

LABEL_MAPPING = {"background": (0, 0), "a": (2, 1), "b": (3, 2), "c": (5, 3), "d": (8, 4)}
OPTIMIZED = ["background", "a", "b", "c", "d"]
UNIT_MAPPING = {"background": (0, 0), "a": (2, 3), "b": (3, 1), "c": (5, 4), "d": (8, 2)}     # of tests/golden/tta_unit_trained.npz


def _bounded(name, got, ref32, ref64, floor=0.0):
    """|got - fp64| <= FACTOR * |fp32 restatement - fp64| (max norm), printed before it is asserted."""
    e_gpu = float((got.detach().cpu().double() - ref64).abs().max())
    e_cpu = float((ref32.double() - ref64).abs().max())
    print(f"{name}: gpu vs fp64 {e_gpu:.3e}, cpu fp32 vs fp64 {e_cpu:.3e}, ratio {e_gpu / max(e_cpu, 1e-300):.2f}")
    assert e_gpu <= FACTOR * max(e_cpu, floor), f"{name}: {e_gpu:.3e} > {FACTOR} x {e_cpu:.3e}"


# ------------------------------------------------------------------------------------------------ 1. fields
def test_fields_against_the_fixture():
    from dg_tta_amd.tta.augmentation_utils import calc_consistent_diffeomorphic_field, get_disp_field, get_rf_field
    g = load_golden("deformable")
    size = [int(v) for v in g["size"]]
    draw = g["draw"]
    f64 = dref.rf_field(draw.double(), size)
    field = get_rf_field(1, size, interpolation_factor=5, num_fields=3, device=DEV, draw=draw.to(DEV))
    _bounded("field", field, g["field"], f64)
    # the integration on the FIXTURE's field, so that its error is not mixed with the field's
    d64, i64 = dref.diffeo_fields(g["field"].double())
    d, i = calc_consistent_diffeomorphic_field(g["field"].to(DEV) * 0.5, None, 5, True)
    d32, i32 = dref.diffeo_fields(g["field"])
    assert torch.equal(d32, g["disp"]) and torch.equal(i32, g["inverse"])
    _bounded("disp", d.permute(0, 2, 3, 4, 1), g["disp"], d64)
    _bounded("inverse", i.permute(0, 2, 3, 4, 1), g["inverse"], i64)
    # the composition, end to end from the draw
    d64, i64 = dref.disp_fields(draw.double(), size)
    d, i = get_disp_field(1, size, factor=0.5, interpolation_factor=5, device=DEV, draw=draw.to(DEV))
    assert d.shape == (1, *size, 3) and d.is_contiguous()
    _bounded("disp from draw", d, g["disp"], d64)
    _bounded("inverse from draw", i, g["inverse"], i64)


def test_fields_at_a_larger_size_and_batch():
    from dg_tta_amd.tta.augmentation_utils import get_disp_field, get_rf_field
    size, b = [40, 52, 66], 3
    draw = dref.hash_noise([b, 3] + [s // 5 for s in size], 7).float()
    f32, f64 = dref.rf_field(draw, size), dref.rf_field(draw.double(), size)
    _bounded("field", get_rf_field(b, size, 5, 3, DEV, draw=draw.to(DEV)), f32, f64)
    d32, i32 = dref.diffeo_fields(f32)
    d64, i64 = dref.disp_fields(draw.double(), size)
    d, i = get_disp_field(b, size, factor=0.5, interpolation_factor=5, device=DEV, draw=draw.to(DEV))
    _bounded("disp", d, d32, d64)
    _bounded("inverse", i, i32, i64)
    # without a draw: the device generator, reproducible from its seed, every sample its own field
    torch.cuda.manual_seed(5)
    a = get_disp_field(2, size, factor=0.5, interpolation_factor=5, device=DEV)[0]
    torch.cuda.manual_seed(5)
    assert torch.equal(a, get_disp_field(2, size, factor=0.5, interpolation_factor=5, device=DEV)[0])
    assert not torch.equal(a[0], a[1]) and bool(torch.isfinite(a).all()) and 0.01 < float(a.abs().max()) < 0.5


# ------------------------------------------------------------------------------------------------ 2. dense sampler
def test_dense_warp_against_the_fixture():
    from dg_tta_amd import ops
    g, gl = load_golden("deformable"), load_golden("deformable_logits")
    size = [int(v) for v in g["size"]]
    disp, inv = g["disp"], g["inverse"]
    image = dref.hash_noise([1, 1] + size, 1)
    out = ops.dense_warp(image.float().to(DEV), disp.to(DEV), "border")
    _bounded("image warp", out, g["image_warped"], dref.dense_warp(image, disp.double(), "border"))
    logits, weight = dref.hash_noise([1, 5] + size, 2), dref.hash_noise([1, 5] + size, 3)
    o64, g64 = dref.warp_and_grad(logits, inv.double(), weight)
    x = logits.float().to(DEV).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    y = ops.dense_warp(x, inv.to(DEV), "zeros")
    assert y.is_contiguous(memory_format=torch.channels_last_3d)
    (y * weight.float().to(DEV)).sum().backward()
    _bounded("logits warp", y, gl["logits_warped"], o64)
    _bounded("logits grad", x.grad, gl["logits_grad"], g64)
    zero = gl["logits_warped"] == 0
    assert 0.005 < float(zero.float().mean()) < 0.05 and bool((y.detach().cpu()[zero] == 0).all())


@pytest.mark.parametrize("padding_mode", ["zeros", "border"])
@pytest.mark.parametrize("layout,channels", [("ncdhw", 1), ("ncdhw", 3), ("ndhwc", 5), ("ndhwc", 16)])
def test_dense_warp_forward_and_backward(padding_mode, layout, channels):
    """Both paddings, both layouts (vector and scalar channel paths), batch of 2, against F.grid_sample + autograd on the CPU."""
    from dg_tta_amd import ops
    size, b = [26, 31, 37], 2
    draw = dref.hash_noise([b, 3] + [s // 5 for s in size], 11).float()
    disp = dref.disp_fields(draw, size)[1] * 1.5          # some samples leave the volume on every side
    src, weight = dref.hash_noise([b, channels] + size, 12), dref.hash_noise([b, channels] + size, 13)

    def cpu(dtype):
        s = src.to(dtype).clone().requires_grad_(True)
        o = dref.dense_warp(s, disp.to(dtype), padding_mode)
        (o * weight.to(dtype)).sum().backward()
        return o.detach(), s.grad

    (o32, g32), (o64, g64) = cpu(torch.float32), cpu(torch.float64)
    x = src.float().to(DEV)
    if layout == "ndhwc":
        x = x.contiguous(memory_format=torch.channels_last_3d)
    x.requires_grad_(True)
    y = ops.dense_warp(x, disp.to(DEV), padding_mode)
    (y * weight.float().to(DEV)).sum().backward()
    _bounded("forward", y, o32, o64)
    _bounded("backward", x.grad, g32, g64)
    if padding_mode == "zeros":
        zero = o32 == 0        # (the fp32 coordinates decide which corners are inside: the kernel evaluates the same ones)
        assert float(zero.float().mean()) > 0.005 and bool((y.detach().cpu()[zero] == 0).all())
    with pytest.raises(ValueError):
        ops.dense_warp(x, disp.to(DEV)[:, :-1], padding_mode)


# ------------------------------------------------------------------------------------------------ 3. one accumulation step
@contextlib.contextmanager
def _cpu_draws():
    """oracle.replay.cpu_rng_for_device_draws plus the field draw: every device draw comes from the CPU generator."""
    from dg_tta_amd.tta import augmentation_utils as au
    from oracle.replay import cpu_rng_for_device_draws
    real = au.draw_field_noise_
    with cpu_rng_for_device_draws():
        au.draw_field_noise_ = lambda slot: slot.copy_(torch.randn(slot.shape))
        try:
            yield
        finally:
            au.draw_field_noise_ = real


def _plan(**over):
    from dg_tta_amd.tta.config_log_utils import TEMPLATE_PLAN
    cfg = dict(TEMPLATE_PLAN)
    cfg.update(do_intensity_aug_in="both", do_spatial_aug_in="both", spatial_aug_type="deformable",
               patches_to_be_accumulated=2, lr=1e-3, optimized_labels=OPTIMIZED)
    cfg.update(over)
    return cfg


def _product_model(g, **kw):
    from dg_tta_amd.gin import gin_hook
    from dg_tta_amd.mind import mind_hook
    from dg_tta_amd.tta.config_log_utils import ModifierFunctions
    from dg_tta_amd.tta.model_utils import get_model_from_network
    from dg_tta_amd.unet import HipPlainConvUNet
    from dg_tta_amd.utils import disable_internal_augmentation
    net = HipPlainConvUNet(SMALL_CFG, conv_impl=kw.pop("conv_impl", 1), **kw)
    assert not net.load_state_dict(state_from_golden(g), strict=False).unexpected_keys
    net = net.to(DEV)
    net.register_forward_pre_hook(gin_hook)
    net.register_forward_pre_hook(mind_hook)
    modmod = SimpleNamespace(ModifierFunctions=ModifierFunctions)
    model = get_model_from_network(net, modmod, None)
    disable_internal_augmentation()
    return model, modmod


PATCH = [32, 28, 36]        # divisible by the net's stride 4, every axis >= 25, non-cubic


def _patch_images(n=1):
    return (dref.hash_noise([n, 1] + PATCH, 21) * 100.0 - 300.0).float()


def test_step_against_the_restated_step():
    """calc_branch a + b, consistency loss, backward: loss and head-weight gradient against the same step in torch on the
    CPU (oracle GIN / MIND / network, tests/deformable_ref.py for the spatial part), from one CPU draw stream in the
    reference's order: GIN, field, MIND noise per branch."""
    from dg_tta_amd import ops
    from dg_tta_amd.gin import gin_aug
    from dg_tta_amd.tta.tta import START_CLASS, _fuse_head_if_possible, calc_branch
    from oracle import gin as ogin, mind as omind, tta as otta, unet as ounet
    g = load_golden("calc_branch")
    imgs = _patch_images()
    om = ounet.PlainConvUNetOracle(SMALL_CFG)
    om.load_state_dict({**om.state_dict(), **state_from_golden(g)})
    om.train()
    map_idxs = otta.get_map_idxs(LABEL_MAPPING, OPTIMIZED, "pretrain_labels")
    torch.manual_seed(31)
    targets = []
    for _ in range(2):
        x = ogin.gin_chain(imgs, *ogin.draw_gin_params(1))
        disp, inv = dref.disp_fields(torch.randn(1, 3, *[s // 5 for s in PATCH]), PATCH)
        x = omind.mind3d(dref.dense_warp(x, disp, "border"), torch.randn(1, 12, *PATCH))
        targets.append(dref.dense_warp(otta.map_label(om(x), map_idxs, "logits"), inv, "zeros"))
    ref_loss = otta.consistency_loss(*targets)
    ref_loss.backward()
    ref_grad = om.decoder.seg_layers[-1].weight.grad[map_idxs]

    model, modmod = _product_model(g)
    assert _fuse_head_if_possible(model, modmod, LABEL_MAPPING, OPTIMIZED)
    a = (_plan(), model, gin_aug, None, PATCH, 1, LABEL_MAPPING, OPTIMIZED, modmod, imgs.to(DEV), torch.device(DEV), True)
    with _cpu_draws():
        torch.manual_seed(31)
        ta, tb = calc_branch("branch_a", *a), calc_branch("branch_b", *a)
    assert ta.requires_grad and not hasattr(ta, "_dgtta_grad16")
    loss, _ = ops.consistency_loss(ta, tb, START_CLASS)
    loss.backward()
    grad = model.decoder.seg_layers[-1].weight.grad.cpu()[map_idxs]
    e_t = max(float((t.detach().cpu() - r.detach()).abs().max()) for t, r in zip((ta, tb), targets))
    e_l, e_g = abs(float(loss.detach()) - float(ref_loss.detach())), float((grad - ref_grad).abs().max()) / float(ref_grad.abs().max())
    print(f"step: targets {e_t:.3e}, loss {float(loss.detach()):.6f} vs {float(ref_loss.detach()):.6f} ({e_l:.3e}), head-grad rel {e_g:.3e}")
    assert e_l < 2e-4 and e_g < 1e-3


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("spatial_in", ["both", "branch_b"])
def test_batched_path_equals_sequential_branches(steps, spatial_in):
    """calc_both_branches (fields of all branches and steps in one launch) == calc_branch a, b per step from the same seeds
    on both generators: pins the draw order (GIN on the CPU generator; field, then MIND noise on the device generator)."""
    from dg_tta_amd import ops
    from dg_tta_amd.gin import gin_aug
    from dg_tta_amd.tta.tta import START_CLASS, _fuse_head_if_possible, calc_both_branches, calc_branch
    g = load_golden("calc_branch")
    cfg = _plan(do_spatial_aug_in=spatial_in)
    dev = torch.device(DEV)
    pool = _patch_images(steps).to(DEV)
    results = []
    for batched in (False, True):
        model, modmod = _product_model(g)
        assert _fuse_head_if_possible(model, modmod, LABEL_MAPPING, OPTIMIZED)
        torch.manual_seed(77)
        torch.cuda.manual_seed(78)
        it = iter(range(steps))
        next_imgs = lambda: pool[next(it)][None]          # noqa: E731
        losses = []
        if batched:
            ta, tb = calc_both_branches(cfg, model, gin_aug, PATCH, 1, LABEL_MAPPING, OPTIMIZED, modmod, next_imgs, dev,
                                        head_is_fused=True, steps=steps)
            loss, dice = ops.consistency_loss(ta, tb, START_CLASS)
            losses = (1.0 - dice[:, START_CLASS:].mean(1)).tolist()
            torch.autograd.backward(loss, grad_tensors=torch.full((), 1.0, device=DEV))
        else:
            for _ in range(steps):
                a = (cfg, model, gin_aug, None, PATCH, 1, LABEL_MAPPING, OPTIMIZED, modmod, next_imgs(), dev, True)
                ta, tb = calc_branch("branch_a", *a), calc_branch("branch_b", *a)
                loss, _ = ops.consistency_loss(ta, tb, START_CLASS)
                losses.append(float(loss))
                torch.autograd.backward(loss, grad_tensors=torch.full((), 1.0 / steps, device=DEV))
        grads = {n: p.grad.detach().float().cpu().clone() for n, p in model.named_parameters() if p.grad is not None}
        results.append((losses, grads))
    (l0, g0), (l1, g1) = results
    print("losses", l0, l1)
    # (the bounds of the affine counterparts of this test in tests/test_gpu_tta.py)
    assert max(abs(a - b) for a, b in zip(l0, l1)) < 2e-6, (l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 10
    for n in g0:
        assert (g0[n] - g1[n]).abs().max().item() < 3e-4 * g0[n].abs().max().item() + 1e-7, n


# ------------------------------------------------------------------------------------------------ 4. a short unit
@pytest.mark.parametrize("storage", [None, torch.float16])
def test_short_unit_runs_to_the_end(storage):
    """3 epochs x 4 steps of tta_unit with the deformable plan: finite losses of the order of the first one and adapted
    parameters, as an affine run of the same set-up gives (its losses are printed beside for comparison)."""
    from dg_tta_amd.optim import HipAdamW
    from dg_tta_amd.tta.tta import _fuse_head_if_possible, tta_unit
    from dg_tta_amd.tta.torch_utils import release_resident
    g = load_golden("tta_unit_trained")
    data = g["data"]
    size = (40, 36, 44)         # the fixture's case (image + one-hot labels), enlarged so that a >= 25-voxel patch fits
    vol = torch.cat([torch.nn.functional.interpolate(data[None, :1], size=size, mode="trilinear"),
                     torch.nn.functional.interpolate(data[None, 1:], size=size, mode="nearest")], dim=1)[0]
    out = {}
    for kind in ("affine", "deformable"):
        model, modmod = _product_model(g, conv_impl=0, **({} if storage is None else {"act_dtype": storage}))
        assert _fuse_head_if_possible(model, modmod, UNIT_MAPPING, OPTIMIZED)
        model.accumulate_grads_in_place = True
        model.exact_zero_bias_grad = True
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        cfg = _plan(spatial_aug_type=kind, epochs=3, patches_to_be_accumulated=4, lr=3e-4, start_tta_at_epoch=1)
        opt = HipAdamW(model.parameters(), lr=cfg["lr"], grad_scale=model.loss_scale)
        release_resident()
        torch.manual_seed(3)
        torch.cuda.manual_seed(4)
        np.random.seed(3)
        losses, dices = tta_unit(model, opt, cfg, [vol], PATCH, UNIT_MAPPING, modmod, torch.device(DEV), True)
        release_resident()
        moved = sum(int((p.detach() != before[n]).any()) for n, p in model.named_parameters())
        out[kind] = (losses, dices, moved, int(opt.skipped_steps))
        print(kind, storage, "losses", losses.tolist(), "dice", dices.tolist(), "tensors moved", moved)
    la, da, ma, sa = out["affine"]
    ld, dd, md, sd = out["deformable"]
    assert ld.shape == la.shape == (3,) and dd.shape == da.shape
    assert bool(torch.isfinite(ld).all()) and sd == 0 and sa == 0
    assert md == ma and md > 10
    assert float(ld.min()) > 0.0 and float(ld.max()) <= 1.0           # 1 - soft Dice
    assert float(ld[1:].max()) <= 2.0 * float(ld[0]) + 1e-3          # decreasing, or at least of the first loss's order
