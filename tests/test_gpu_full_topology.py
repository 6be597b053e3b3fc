"""GPU parity on the REAL network: nnUNet 3d_fullres (plans.json:279-401: 32/64/128/256/320 features, 12 -> 105 channels)
running the product's default kernels (conv_impl=0: MFMA implicit GEMM, row-reuse conv, transposed-read weight gradients,
concat buffers, fused statistics) in fp32 and in bf16 storage, against

* tests/golden/full_{32,64}.npz — one accumulation step (calc_branch a + b, loss, backward) produced by the REFERENCE's
  calc_branch / soft_dice_loss on torch CPU (tests/golden/make_golden_r2.py), and
* the CPU oracle run in the test at 128^3 (BASELINE config 2's patch size), forward.

Tolerances: fp32 2e-4 of the tensor's range (different summation order); bf16 storage: loss within 1e-3 (north_star's
Dice tolerance), logits within 3 % of their range, label maps identical wherever the reference's top-2 margin exceeds the
measured logit error."""
import pytest
import torch

from conftest import load_golden, reload_kernel_switches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _nets(w_seed, dtype, conv_impl=0):
    from dg_tta_amd.unet import HipPlainConvUNet
    from oracle import unet as ounet
    om = ounet.perturb_affine(ounet.init_he(ounet.PlainConvUNetOracle(), w_seed), w_seed + 1)
    hm = HipPlainConvUNet(act_dtype=dtype, conv_impl=conv_impl)          # default cfg = PLANS_3D_FULLRES
    hm.load_state_dict(om.state_dict())
    return om, hm.to(DEV)


def _hip_branch(model, imgs, d):
    from dg_tta_amd import ops
    from dg_tta_amd.mind import MIND3D
    from oracle import tta as otta
    alpha, ks, kers, shifts = d["gin_draw"]
    x = ops.gin_chain(imgs, alpha.to(DEV), ks, [k.to(DEV) for k in kers], [s.to(DEV) for s in shifts])
    r, rinv = otta.rand_affine_from_draw(d["affine_draw"])
    x = ops.affine_warp(x, r.to(DEV), padding_mode="border", tta_grid_algebra=True)
    x = MIND3D()(x, d["mind_noise"].to(DEV), out_dtype=model.act_dtype)
    return ops.affine_warp(model(x), rinv.to(DEV), padding_mode="zeros", tta_grid_algebra=True)


@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_full_topology_step_golden(size, dtype):
    from dg_tta_amd import ops
    from oracle import tta as otta
    g = load_golden(f"full_{size}")
    adt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    _, hm = _nets(int(g["w_seed"]), adt)
    sel = torch.arange(int(g["copt"])) * 3
    hm.set_selected_classes(sel)
    torch.manual_seed(int(g["img_seed"]))
    imgs = torch.randn(1, 1, size, size, size)
    assert abs(imgs.double().sum().item() - float(g["imgs_sum"])) < 1e-9      # same draw as the generator's
    imgs = imgs.to(DEV)
    st = int(g["slice_step"])
    outs = {}
    for br in ("a", "b"):
        torch.manual_seed(int(g[f"seed_{br}"]))
        d = otta.draw_branch(1, [size] * 3)
        outs[br] = out = _hip_branch(hm, imgs, d)
        ref = g[f"out_{br}_slice"]
        rng = float(g[f"out_{br}_absmax"])
        err = (out.detach().cpu()[:, :, ::st, ::st, ::st] - ref).abs().max().item()
        tol = {"fp32": 2e-4, "bf16": 3e-2, "fp16": 4e-3}[dtype]         # 24 / 8 / 11 mantissa bits in storage
        assert err < tol * rng, f"{dtype} {size}^3 branch {br}: logits err {err:.3e} (range {rng:.2f})"
        csum = out.detach().double().sum((0, 2, 3, 4)).cpu()
        cabs = g[f"out_{br}_chanabs"]
        assert ((csum - g[f"out_{br}_chansum"]).abs() < {"fp32": 2e-5, "bf16": 4e-3, "fp16": 5e-4}[dtype] * cabs).all()
        margin = g[f"out_{br}_margin"].float()
        safe = margin > (1e-3 if dtype == "fp32" else max(4 * err, 1e-2 if dtype == "bf16" else 2e-3))
        am = out.detach().argmax(1).cpu().to(torch.uint8)
        assert torch.equal(am[safe], g[f"out_{br}_argmax"][safe])
        if dtype == "fp32":
            assert (am == g[f"out_{br}_argmax"]).float().mean() > 0.9995
    loss, dice = ops.consistency_loss(outs["a"], outs["b"], 1)
    ltol = {"fp32": 2e-5, "bf16": 1e-3, "fp16": 2e-4}[dtype]
    assert abs(float(loss.detach()) - float(g["loss"])) < ltol, f"loss {float(loss.detach()):.6f} vs {float(g['loss']):.6f}"
    assert (dice.cpu() - g["dice"]).abs().max() < {"fp32": 5e-5, "bf16": 2e-3, "fp16": 4e-4}[dtype]
    # fp16 storage: the loss gradient is multiplied by the model's static loss scale (as tta_epoch does) so that the
    # activation gradients stay inside fp16's range; parameter gradients are divided by it again below
    scale = float(hm.loss_scale)
    assert (scale > 1.0) == (dtype == "fp16")
    torch.autograd.backward(loss, grad_tensors=torch.full((), scale, device=DEV))
    # ---- gradients.  LeakyReLU's kink makes the gradient of this net discontinuous in the activations: a pre-activation
    # within rounding distance of zero takes the other slope (1 vs 0.01), and with ~10^7 activations per pass a handful do
    # in ANY fp32 evaluation.  The REFERENCE's own fp32 gradients therefore deviate from a float64 evaluation of the same
    # graph by up to 2-4 % of a tensor's range in the layers with few voxels (`gcond::<name>`, measured by
    # make_golden_r2.py; profiles/tools/dbg_block.py shows torch-CPU and the HIP kernels each hitting such flips on 2-stage nets
    # while agreeing to 3e-6 otherwise).  fp32 kernels are checked against the float64 values (`g64::`) with the
    # reference's own deviation as the yardstick (the MFMA K-loop accumulates 8640 terms in sequence: ~4x torch's forward
    # rounding, hence more flips), plus direction (cosine) and sign agreement, which is what Adam consumes.
    # bf16 storage (8 mantissa bits): direction and sign agreement per layer.
    from make_slices import GRAD_SLICES
    named = dict(hm.named_parameters())
    rows, worst = [], 0.0
    for key in [k for k in g if k.startswith("g::")]:
        name = key[3:]
        ref32, ref64 = g[key], g[f"g64::{name}"]
        got = named[name].grad.detach().cpu() / scale
        if name in GRAD_SLICES:
            got = got[GRAD_SLICES[name]]
        gmax = float(g[f"gmax::{name}"])
        cond = float(g[f"gcond::{name}"])
        rel32 = (got - ref32).abs().max().item() / gmax
        rel64 = (got.double() - ref64).abs().max().item() / gmax
        cos = torch.nn.functional.cosine_similarity(got.double().flatten(), ref64.flatten(), dim=0).item()
        sign = (torch.sign(got.double()) == torch.sign(ref64)).float().mean().item()
        rows.append(f"  {name:48s} vs f64 {rel64:.2e} (reference's own {cond:.2e})  vs ref {rel32:.2e}  cos {cos:.5f}  sign {sign:.4f}")
        if dtype == "fp32":
            assert rel64 < 15.0 * cond + 1e-3, f"fp32 {size}^3 grad {name}: {rel64:.3e} from float64, reference {cond:.3e}"
            assert rel32 < 16.0 * cond + 1e-3, f"fp32 {size}^3 grad {name}: {rel32:.3e} from the reference"
            assert cos > 0.9995, f"fp32 {size}^3 grad {name}: cosine {cos:.6f}"
            assert sign > 0.99 or got.numel() < 1024, f"fp32 {size}^3 grad {name}: sign agreement {sign:.4f}"
        elif dtype == "fp16":       # 11 mantissa bits: direction within 1 %, sign agreement within a few %
            assert torch.isfinite(got).all(), f"fp16 {size}^3 grad {name}: overflow (loss scale {scale})"
            assert cos > 0.98, f"fp16 {size}^3 grad {name}: cosine {cos:.5f}"      # measured >= 0.989 (bf16: 0.90)
            assert sign > 0.95 or got.numel() < 1024, f"fp16 {size}^3 grad {name}: sign agreement {sign:.4f}"
        else:
            top = name.startswith("decoder.stages.3") or name.startswith("decoder.seg_layers") or \
                name.startswith("decoder.transpconvs.3")
            assert cos > (0.995 if top else 0.85), f"bf16 {size}^3 grad {name}: cosine {cos:.4f}"
            assert sign > (0.97 if top else 0.80) or got.numel() < 1024, f"bf16 {size}^3 grad {name}: sign {sign:.4f}"
        worst = max(worst, rel64 / (cond + 1e-4))
    # every parameter's gradient: abs-sum checksum against the reference's
    for name, p in named.items():
        if f"gabs::{name}" not in g or (name.endswith("conv.bias") and ".convs." in name):
            continue            # conv bias in front of InstanceNorm: exactly zero in exact arithmetic, noise in autograd
        gabs, cond = float(g[f"gabs::{name}"]), float(g[f"gcond::{name}"])
        got = p.grad.detach().double().abs().sum().item() / scale
        tol = (8.0 * cond + 2e-3) if dtype == "fp32" else (0.25 if dtype == "bf16" else 0.05)
        assert abs(got - gabs) < tol * gabs + 1e-12, f"{dtype} {size}^3 |grad| checksum {name}: {got:.6e} vs {gabs:.6e}"
    print(f"\nfull {size}^3 {dtype}: loss {float(loss.detach()):.6f} (ref {float(g['loss']):.6f}); worst gradient error = "
          f"{worst:.2f} x the reference's own fp32 rounding error\n" + "\n".join(r for r in rows if ".norm." not in r))


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_full_topology_forward_128_vs_cpu_oracle(dtype):
    """BASELINE config 2's patch: one 128^3 forward of the full net (MIND features in, C_opt rows out) against the CPU
    oracle evaluated in the test (torch CPU conv3d / InstanceNorm3d; ~20 s of host time)."""
    import os
    from dg_tta_amd.mind import MIND3D
    from oracle import mind as omind
    adt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    om, hm = _nets(7, adt)
    sel = torch.arange(16) * 3
    hm.set_selected_classes(sel)
    torch.manual_seed(3)
    img = torch.randn(1, 1, 128, 128, 128)
    noise = torch.randn(1, 12, 128, 128, 128)
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    with torch.no_grad():
        ref = om(omind.mind3d(img, noise))[:, sel]
        out = hm(MIND3D()(img.to(DEV), noise.to(DEV), out_dtype=adt)).cpu()
    rng = ref.abs().max().item()
    err = (out - ref).abs().max().item()
    assert err < {"fp32": 2e-4, "bf16": 3e-2, "fp16": 4e-3}[dtype] * rng, f"{dtype}: err {err:.3e}, range {rng:.2f}"
    top2 = ref.topk(2, dim=1).values
    safe = (top2[:, 0] - top2[:, 1]) > (1e-3 if dtype == "fp32" else max(4 * err, 1e-2 if dtype == "bf16" else 2e-3))
    assert torch.equal(out.argmax(1)[safe], ref.argmax(1)[safe])
    agree = (out.argmax(1) == ref.argmax(1)).float().mean().item()
    assert agree > {"fp32": 0.9995, "bf16": 0.97, "fp16": 0.995}[dtype]
    print(f"128^3 {dtype}: max logit err {err:.3e} of range {rng:.2f}; label agreement {agree:.5f}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_noncubic_batch_16bit_kernels_vs_reference_kernels(dtype):
    """A non-cubic patch (64 x 96 x 160: different tile counts per axis, ragged 32-voxel blocks at the coarse levels) with
    batch 2 through the full 3d_fullres topology: the product's 16-bit kernels (row-reuse conv with the XCD job order,
    register-operand stride-2 and transposed-conv kernels, transposed-read weight gradients sweeping several units) against
    the general VALU kernels in fp32 (conv_impl=1) on the same weights and inputs - logits and every parameter gradient."""
    adt = torch.bfloat16 if dtype == "bf16" else torch.float16
    _, ref = _nets(11, torch.float32, conv_impl=1)
    _, hm = _nets(11, adt)
    sel = torch.arange(16) * 5
    for m in (ref, hm):
        m.set_selected_classes(sel)
    torch.manual_seed(3)
    x = torch.randn(2, 12, 64, 96, 160, device=DEV)
    gout = torch.randn(2, 16, 64, 96, 160, device=DEV) * 1e-3
    outs, grads = [], []
    for m in (ref, hm):
        xin = x.to(m.act_dtype) if m.act_dtype != torch.float32 else x
        out = m(xin)
        scale = float(getattr(m, "loss_scale", 1.0))
        (out.float() * gout * scale).sum().backward()
        outs.append(out.float())
        grads.append({n: p.grad.float() / scale for n, p in m.named_parameters() if p.grad is not None})
    rng = float(outs[0].abs().max())
    tol = 0.03 if dtype == "bf16" else 0.005
    assert float((outs[1] - outs[0]).abs().max()) < tol * rng
    assert set(grads[0]) == set(grads[1])
    cosines = {}
    for n, gr in grads[0].items():
        # a conv bias in front of InstanceNorm has an identically-zero gradient in exact arithmetic (rounding noise in both)
        if gr.numel() < 2 or (n.endswith("conv.bias") and "seg_layers" not in n and "transpconvs" not in n):
            continue
        cosines[n] = float(torch.nn.functional.cosine_similarity(gr.flatten().double(), grads[1][n].flatten().double(), dim=0))
    bad = {n: round(c, 4) for n, c in cosines.items() if c < (0.85 if dtype == "bf16" else 0.97)}
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("nsel", [16, 8])
def test_head_fused_with_the_inverse_warp_matches_head_then_warp(dtype, nsel, monkeypatch):
    """Round 3: dgtta_seghead_warp_fwd / _bwd (head + inverse logit warp in one launch each way, csrc/warp.hip) against the
    two-step path (dgtta_seghead_* then dgtta_affine_warp3d_*) on the full 3d_fullres net: same logits up to fp32
    association, the SAME feature-map gradient and head weight gradient bit for bit (identical gather order and FMA chain),
    the bias gradient up to its reduction order; every other parameter gradient follows from gz and must be identical too."""
    from dg_tta_amd import ops
    from dg_tta_amd.synthetic import he_init_
    from dg_tta_amd.unet import HipPlainConvUNet
    from oracle import tta as otta
    torch.manual_seed(3)
    net = he_init_(HipPlainConvUNet(act_dtype=dtype), seed=7)
    net.decoder.seg_layers[-1].bias.data.normal_()
    net = net.to(DEV)
    net.set_selected_classes(torch.arange(nsel) * 5 + 1)
    x = torch.rand(2, 12, 32, 32, 32, device=DEV)
    _, rinv = otta.rand_affine_from_draw(torch.randn(2, 3, 4), 0.08)
    rinv = rinv.float().contiguous()
    gout = torch.randn(2, nsel, 32, 32, 32, device=DEV).contiguous(memory_format=torch.channels_last_3d)
    assert net.can_fuse_output_warp(x.shape, rinv)

    def run(fused):
        net.zero_grad()
        if fused:
            with net.fuse_output_warp(rinv.to(DEV), rinv):
                y = net(x)
        else:
            y = ops.affine_warp(net(x), rinv.to(DEV), padding_mode="zeros", tta_grid_algebra=True)
        y.backward(gout)
        torch.cuda.synchronize()
        return y.detach().clone(), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}

    y0, g0 = run(False)
    y1, g1 = run(True)
    # round 6: the fused FORWARD's head products run on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain);
    # DGTTA_HEADWARP_MFMA=0 selects the FMA chain + quad butterfly it replaced: the same logits to fp32 association (the
    # backward is one kernel either way)
    monkeypatch.setenv("DGTTA_HEADWARP_MFMA", "0")
    reload_kernel_switches()
    y2, g2 = run(True)
    monkeypatch.delenv("DGTTA_HEADWARP_MFMA")
    reload_kernel_switches()
    assert float((y2 - y1).abs().max()) < 2e-6 * float(y0.max() - y0.min()) + 1e-6 and not torch.equal(y2, y1)
    for n in g1:
        if n != "decoder.seg_layers.3.bias":
            assert torch.equal(g1[n], g2[n]), n
    rng = float(y0.max() - y0.min())
    assert tuple(y1.shape) == tuple(y0.shape) and float((y1 - y0).abs().max()) < 2e-6 * rng + 1e-6
    assert set(g0) == set(g1)
    for n in g0:
        if n == "decoder.seg_layers.3.bias":
            assert float((g0[n] - g1[n]).abs().max()) < 1e-4 * float(g0[n].abs().max()) + 1e-6, n
        else:
            assert torch.equal(g0[n], g1[n]), f"{n}: fused backward differs"
    # maps the owner-computes gather declines are not offered the fused pair
    assert not net.can_fuse_output_warp(x.shape, torch.zeros(2, 3, 4))
    assert not net.can_fuse_output_warp(x.shape, rinv * 0.05)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_level0_concat_buffer_as_planes_matches_the_interleaved_layout(dtype, monkeypatch):
    """Round 6: the level-0 concat buffer as two dense 32-channel planes [up | skip] (the decoder conv and its
    weight gradient read them as channel BLOCKS: dgtta_conv3d_k3_fwd_blocked / _wgrad_blocked on the ring kernels) against the
    interleaved [voxel][64] layout (DGTTA_PLANAR_CAT=0): the same kernels in the same order - logits and every parameter
    gradient bit for bit.  The query says where the layout applies; outside it the blocked calls refuse instead of mis-reading."""
    from dg_tta_amd import _lib, ops
    from dg_tta_amd._lib import ptr, stream_of
    from dg_tta_amd.synthetic import he_init_
    from dg_tta_amd.unet import HipPlainConvUNet
    lib = _lib.load()
    dt = ops.dtype_code(dtype)
    B, N = 4, 64
    assert lib.dgtta_conv3d_k3_blocked_supported(B, 64, 32, N, N, N, dt) == 1           # the layout is really offered at this size
    assert lib.dgtta_conv3d_k3_blocked_supported(2, 64, 32, N, N, N, dt) == 0           # (too few columns for the weight-gradient sweep)
    assert lib.dgtta_conv3d_k3_blocked_supported(B, 64, 32, 16, 16, 16, dt) == 0          # small launches stay with the tile kernels
    assert lib.dgtta_conv3d_k3_blocked_supported(B, 128, 64, N, N, N, dt) == 0 and lib.dgtta_conv3d_k3_blocked_supported(B, 64, 32, N, N, N, 0) == 0
    x16 = torch.zeros(2, 1, 16, 16, 16, 32, dtype=dtype, device=DEV)
    y16 = torch.empty(1, 16, 16, 16, 32, dtype=dtype, device=DEV)
    wp = torch.zeros(lib.dgtta_conv3d_packed_bytes(64, 32, dt) // 2, dtype=dtype, device=DEV)
    rc = lib.dgtta_conv3d_k3_fwd_blocked(ptr(x16), x16[0].numel(), ptr(wp), None, ptr(y16), 32, None, 1, 64, 32, 64, 32, 16, 16, 16, dt,
                                         stream_of())
    assert rc == -2 and b"ring" in lib.dgtta_last_error()                           # DGTTA_ERR_UNSUPPORTED, nothing launched
    torch.manual_seed(9)
    net = he_init_(HipPlainConvUNet(act_dtype=dtype), seed=7)
    for m in net.modules():
        if m.__class__.__name__ == "HipInstanceNorm3d":
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)
    net = net.to(DEV)
    net.set_selected_classes(torch.arange(16) * 5 + 1)
    x = torch.rand(B, 12, N, N, N, device=DEV)
    gout = torch.randn(B, 16, N, N, N, device=DEV).contiguous(memory_format=torch.channels_last_3d) * 64.0

    def run():
        net.zero_grad()
        y = net(x)
        y.backward(gout)
        torch.cuda.synchronize()
        return y.detach().clone(), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    y1, g1 = run()
    monkeypatch.setenv("DGTTA_PLANAR_CAT", "0")
    y0, g0 = run()
    monkeypatch.delenv("DGTTA_PLANAR_CAT")
    assert torch.equal(y0, y1) and set(g0) == set(g1) and float(y1.abs().max()) > 0
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_logit_gradient_in_the_storage_type_through_the_sink(dtype, monkeypatch):
    """Round 6: between the loss backward and the fused head + warp backward the logit gradient travels in the
    network's 16-bit storage type (dgtta_softdice_bwd_t -> unet.Grad16Sink -> dgtta_seghead_warp_bwd_g16).
    (i) kernel level: the 16-bit rows are the fp32 gradient rounded once, and the gather on them equals the fp32 gather on the
    widened values bit for bit; (ii) network level: the product's batched pair with the sink on / off (DGTTA_GRAD16=0): same
    loss, parameter gradients within the rounding of one more 16-bit tensor; a second consumer of the output is summed, not lost."""
    from dg_tta_amd import _lib, ops
    from dg_tta_amd._lib import check, ptr, stream_of
    from dg_tta_amd.synthetic import he_init_
    from dg_tta_amd.unet import HipPlainConvUNet
    from oracle import tta as otta
    lib = _lib.load()
    dt = ops.dtype_code(dtype)
    torch.manual_seed(5)
    B, N, C = 2, 32, 16
    # ---- (i) kernels
    both = torch.randn(2 * B, N, N, N, C, device=DEV) * 3
    b2, v = 2 * B, N ** 3
    nbytes = lib.dgtta_softdice_ws_bytes(B, C, v)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dice, loss = torch.empty(B, C, device=DEV), torch.empty((), device=DEV)
    check(lib.dgtta_softdice_fwd(ptr(both[:B]), ptr(both[B:]), ptr(dice), ptr(loss), ptr(ws), nbytes, B, C, v, C, 1, 1, stream_of()), "fwd")
    g32 = torch.empty_like(both)
    g16 = torch.empty(b2, N, N, N, C, dtype=dtype, device=DEV)
    check(lib.dgtta_softdice_bwd(ptr(both[:B]), ptr(both[B:]), ptr(g32[:B]), ptr(g32[B:]), ptr(ws), 4096.0, None, B, C, v, C, 1, stream_of()), "bwd")
    check(lib.dgtta_softdice_bwd_t(ptr(both[:B]), ptr(both[B:]), ptr(g16[:B]), ptr(g16[B:]), ptr(ws), 4096.0, None, B, C, v, C, 1, dt,
                                   stream_of()), "bwd_t")
    # the fp32 value rounded ONCE: equal to torch's cast except where hipcc folds the last multiply into the conversion
    # (v_fma_mix*: the exact product rounded straight to fp16 - fp32 ties then fall the other way, 14 of 2 M values measured)
    ref = g32.to(dtype)
    assert float((g16 != ref).float().mean()) < 1e-4 and float(g32.abs().max()) > 0
    ulp = 2.0 ** (-10 if dtype == torch.float16 else -7)
    assert bool(((g16.float() - g32).abs() <= ulp * g32.abs() + 6e-8).all())
    z = torch.randn(b2, N, N, N, 32, device=DEV).to(dtype)
    w, sel = torch.randn(105, 32, device=DEV) * 0.1, (torch.arange(C) * 3).to(torch.int32).to(DEV)
    _, rinv = otta.rand_affine_from_draw(torch.randn(b2, 3, 4), 0.08)
    rinv = rinv.float().contiguous()
    nb = lib.dgtta_seghead_warp_bwd_ws_bytes(b2, 32, C, N, N, N)
    outs = []
    for use16 in (True, False):          # the 16-bit gather against the fp32 gather on the widened values
        ws2 = torch.empty(nb, dtype=torch.uint8, device=DEV)
        gz = torch.empty(b2, N, N, N, 32, dtype=dtype, device=DEV)
        dws, dbs = torch.empty(C, 32, device=DEV), torch.empty(C, device=DEV)
        gin = g16 if use16 else g16.float()
        fn = lib.dgtta_seghead_warp_bwd_g16 if use16 else lib.dgtta_seghead_warp_bwd
        check(fn(ptr(z), ptr(gin), ptr(rinv.to(DEV)), ptr(rinv), ptr(w), ptr(sel), C, ptr(gz), ptr(dws), ptr(dbs), ptr(ws2), nb, b2, 32,
                 N, N, N, 1, 0, dt, stream_of()), "head_warp_bwd")
        torch.cuda.synchronize()
        outs.append((gz, dws, dbs))
    for o in outs[:-1]:
        for a, b in zip(o, outs[-1]):
            assert torch.equal(a, b)
    assert float(outs[0][0].float().abs().max()) > 0
    # ---- (ii) the network's batched pair
    net = he_init_(HipPlainConvUNet(act_dtype=dtype), seed=7).to(DEV)
    net.set_selected_classes(torch.arange(C) * 5 + 1)
    x = torch.rand(b2, 12, N, N, N, device=DEV)

    def run(extra_consumer=False):
        net.zero_grad()
        with net.fuse_output_warp(rinv.to(DEV), rinv):
            y = net(x)
        ta, tb = y[:B], y[B:]
        ta._dgtta_pair = tb._dgtta_pair = y
        ta._dgtta_guard_items = tb._dgtta_guard_items = 1
        loss, _ = ops.consistency_loss(ta, tb, 1)
        total = loss * 1024.0 + (y.sum() * 1e-6 if extra_consumer else 0.0)
        total.backward()
        torch.cuda.synchronize()
        return float(loss), {n: p.grad.detach().float().clone() for n, p in net.named_parameters() if p.grad is not None}
    l1, ga = run()
    monkeypatch.setenv("DGTTA_GRAD16", "0")
    l0, gb = run()
    monkeypatch.delenv("DGTTA_GRAD16")
    assert l1 == l0 and set(ga) == set(gb)
    lim = 2e-2 if dtype == torch.bfloat16 else 3e-3
    differs = 0
    for n in ga:
        sc = float(gb[n].abs().max())
        if sc == 0.0 or (n.endswith("conv.bias") and ".convs." in n):
            continue
        assert float((ga[n] - gb[n]).abs().max()) <= lim * sc, n
        cos = float((ga[n].double().flatten() @ gb[n].double().flatten()) / (ga[n].double().norm() * gb[n].double().norm()))
        assert cos > (0.999 if dtype == torch.bfloat16 else 0.99999), (n, cos)
        differs += int(not torch.equal(ga[n], gb[n]))
    assert differs > 0                       # the 16-bit channel really ran
    # a second consumer of the output: its dense gradient and the sink's are summed (nothing is dropped)
    _, gc = run(extra_consumer=True)
    hb = "decoder.seg_layers.3.bias"
    assert float((gc[hb] - ga[hb]).abs().max()) > 0
    # two sink-aware losses on ONE output: the second takes the fp32 route, the gradients add up (2x one loss's, to 16-bit rounding)
    net.zero_grad()
    with net.fuse_output_warp(rinv.to(DEV), rinv):
        y = net(x)
    ta, tb = y[:B], y[B:]
    ta._dgtta_pair = tb._dgtta_pair = y
    ta._dgtta_guard_items = tb._dgtta_guard_items = 1
    l_a, _ = ops.consistency_loss(ta, tb, 1)
    l_b, _ = ops.consistency_loss(ta, tb, 1)
    ((l_a + l_b) * 1024.0).backward()
    torch.cuda.synchronize()
    g2 = net.decoder.seg_layers[-1].weight.grad.detach().float()
    gw = ga["decoder.seg_layers.3.weight"]
    assert float((g2 - 2 * gw).abs().max()) <= lim * 2 * float(gw.abs().max())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_dgrad_with_fused_instancenorm_statistics_matches_the_reduction_pass(dtype, monkeypatch):
    """Round 3 (VERDICT r2 #3 i): the row-reuse data gradient leaves sum g' and sum g' y of the previous block's InstanceNorm
    backward (conv_rows.hip GST + in_bwd_finalize_kernel with mean_rstd) instead of a reduction pass over y and gz
    (DGTTA_IN_GSTATS=0).  That the finalize step and the apply pass turn such sums into the reduction pass's results to a few
    fp32 roundings is asserted against float64 in tests/test_gpu_instnorm.py::test_backward_from_gstats_partials; inside the
    net the last-bit differences of the mean terms move single fp16 roundings of dy, which the LeakyReLU kinks of the layers
    below amplify (gradient conditioning): every parameter gradient agrees to 3e-3 of its scale, cosine > 0.9999.
    The fused path really ran: some tensor differs in its bits."""
    from conftest import reload_kernel_switches
    from dg_tta_amd.synthetic import he_init_
    from dg_tta_amd.unet import HipPlainConvUNet
    torch.manual_seed(4)
    net = he_init_(HipPlainConvUNet(act_dtype=dtype), seed=7)
    for m in net.modules():          # non-trivial affine parameters
        if m.__class__.__name__ == "HipInstanceNorm3d":
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)
    net = net.to(DEV)
    net.set_selected_classes(torch.arange(16) * 3)
    net.exact_zero_bias_grad = True      # (a conv bias in front of InstanceNorm has a zero gradient: pure rounding noise otherwise)
    x = torch.rand(2, 12, 64, 64, 64, device=DEV)
    gout = torch.randn(2, 16, 64, 64, 64, device=DEV).contiguous(memory_format=torch.channels_last_3d)

    def run(flag):
        monkeypatch.setenv("DGTTA_IN_GSTATS", flag)
        reload_kernel_switches()
        net.zero_grad()
        net(x).backward(gout)
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}

    g1, g0 = run("1"), run("0")
    tol, min_cos = (3e-3, 0.9999) if dtype == torch.float16 else (4e-2, 0.998)      # bf16 roundings are 8x coarser
    differs = 0
    for n in g0:
        scale = float(g0[n].abs().max())
        if scale == 0.0:              # exact zeros of the conv biases in front of InstanceNorm
            assert float(g1[n].abs().max()) == 0.0
            continue
        assert float((g1[n] - g0[n]).abs().max()) <= tol * scale + 1e-9, n
        cos = float((g1[n].double().flatten() @ g0[n].double().flatten()) /
                    (g1[n].double().norm() * g0[n].double().norm()).clamp_min(1e-300))
        assert cos > min_cos, (n, cos)
        differs += int(not torch.equal(g1[n], g0[n]))
    assert differs > 0          # the fused statistics were in use (another summation order somewhere)


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_full_topology_unit_with_optimizer_steps_golden(dtype):
    """Round 5: the product's tta_unit on the FULL 3d_fullres topology against a REFERENCE RUN WITH OPTIMIZER
    STEPS (tests/golden/full_unit_32.npz: tta.py:189-340 around the reference's own get_batch / calc_branch / soft_dice_loss /
    dice_coeff and torch AdamW, 4 epochs x 4 accumulation steps on 32^3 patches at the plan's lr 1e-5, make_golden_r5.py), driven by the same
    draw stream: per-epoch losses, pseudo-Dice, the adapted parameters (checksums of every tensor's update and strided slices) and
    the final label map on the first noise draw."""
    import numpy as np
    from types import SimpleNamespace
    from dg_tta_amd.gin import gin_hook
    from dg_tta_amd.mind import MIND3D, mind_hook
    from dg_tta_amd.optim import HipAdamW
    from dg_tta_amd.synthetic import synthetic_case
    from dg_tta_amd.tta.config_log_utils import ModifierFunctions, TEMPLATE_PLAN
    from dg_tta_amd.tta.model_utils import get_model_from_network
    from dg_tta_amd.tta.torch_utils import get_batch, release_resident
    from dg_tta_amd.tta.tta import _fuse_head_if_possible, tta_unit
    from dg_tta_amd.utils import disable_internal_augmentation
    from make_slices import GRAD_SLICES
    from oracle.replay import cpu_rng_for_device_draws
    g = load_golden("full_unit_32")
    adt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    om, hm = _nets(int(g["w_seed"]), adt)
    hm.register_forward_pre_hook(gin_hook)
    hm.register_forward_pre_hook(mind_hook)
    copt, size = int(g["copt"]), int(g["size"])
    names = ["background"] + [f"structure_{i:02d}" for i in range(1, copt)]
    mapping = {n: (3 * i, i) for i, n in enumerate(names)}
    modmod = SimpleNamespace(ModifierFunctions=ModifierFunctions)
    model = get_model_from_network(hm, modmod, None)
    assert _fuse_head_if_possible(model, modmod, mapping, names)
    model.accumulate_grads_in_place = True
    model.exact_zero_bias_grad = True
    cfg = dict(TEMPLATE_PLAN)
    cfg.update(do_intensity_aug_in="both", do_spatial_aug_in="both", patches_to_be_accumulated=int(g["accum"]), lr=float(g["lr"]),
               epochs=int(g["epochs"]), optimized_labels=names)
    data = synthetic_case(size=int(g["vol"]), k=int(g["k"]), seed=int(g["data_seed"]))
    assert abs(data.double().sum().item() - float(g["data_sum"])) < 1e-6 * abs(float(g["data_sum"])) + 1e-6
    opt = HipAdamW(model.parameters(), lr=cfg["lr"], grad_scale=model.loss_scale)
    disable_internal_augmentation()
    release_resident()
    with cpu_rng_for_device_draws():
        torch.manual_seed(int(g["seed"]))
        np.random.seed(int(g["seed"]))
        losses, dices = tta_unit(model, opt, cfg, [data], [size] * 3, mapping, modmod, torch.device(DEV), True)
    assert int(opt.skipped_steps) == 0
    # measured on MI355X (loss / pseudo-Dice / slice elements following the reference / labels equal where the margin > 1e-3 / overall):
    #   fp32 1.8e-6 / 1.3e-6 / 0.963 / 1.0 / 0.99963;  fp16 1.2e-5 / 1.4e-4 / 0.804 / 0.9977 / 0.9968;  bf16 4.2e-5 / 3.1e-4 / 0.660 / 0.981 / 0.980
    # (seeded He-initialised weights: near-tied logits and noise-level gradients in 4-7 % of the elements)
    lim = {"fp32": dict(loss=1e-5, dice=1e-4, agree=0.94, safe=1.0, overall=0.999),
           "fp16": dict(loss=5e-5, dice=5e-4, agree=0.75, safe=0.995, overall=0.994),
           "bf16": dict(loss=2e-4, dice=1e-3, agree=0.58, safe=0.97, overall=0.97)}[dtype]
    dl, dd = float((losses - g["tta_losses"]).abs().max()), float((dices - g["eval_dices"]).abs().max())
    # adapted parameters: Adam's first steps are ~lr * sign(gradient); |update| summed over a tensor is insensitive to the sign
    # flips of noise-level gradients, the strided slices count elements that follow the reference's update
    pre = dict(om.named_parameters())
    worst_abs, moved, agree = 0.0, 0, 0
    for name, p in model.named_parameters():
        if name.endswith("conv.bias") and ".convs." in name:
            continue            # exact-zero gradient in the product, rounding noise in autograd
        d = (p.detach().cpu() - pre[name].detach()).double()
        ref_abs = float(g[f"dabs::{name}"])
        if ref_abs > 0:
            worst_abs = max(worst_abs, abs(float(d.abs().sum()) - ref_abs) / ref_abs)
        if name in GRAD_SLICES:
            ds, rs = d[GRAD_SLICES[name]].float(), g[f"d::{name}"]
            moved += rs.numel()
            agree += int(((ds - rs).abs() <= 0.1 * rs.abs() + 2e-8).sum())
    # final prediction on the stored first noise draw
    torch.manual_seed(int(g["noise_seed"]))
    noise = torch.randn(1, 12, size, size, size)
    with torch.no_grad():
        model.eval()
        imgs, _ = get_batch([data], [0], [size] * 3, "center", DEV)
        logits = model.forward(MIND3D()(imgs[0], noise.to(DEV), out_dtype=adt)).float().cpu()
    same = logits.argmax(1) == g["eval_argmax"].long()
    safe = g["eval_margin"].float() > 1e-3
    lerr = float((logits[:, :, ::2, ::2, ::2] - g["eval_logits_slice"]).abs().max()) / float(g["eval_absmax"])
    print(f"\nfull unit {dtype}: loss delta {dl:.2e}, pseudo-Dice delta {dd:.2e}, |update| checksum worst {worst_abs:.3f}, slice elements "
          f"following the reference {agree / moved:.4f}, labels equal {float(same.float().mean()):.5f} "
          f"({float(same[safe].float().mean()):.5f} where the margin > 1e-3), logits {lerr:.2e} of their range")
    assert dl < lim["loss"] and dd < lim["dice"]
    assert worst_abs < 0.25 and agree / moved > lim["agree"]
    assert float(same[safe].float().mean()) >= lim["safe"] and float(same.float().mean()) >= lim["overall"]
    release_resident()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("size", [(32, 32, 32), (64, 32, 96)])
def test_concat_gradient_as_two_dense_halves_is_bit_identical(dtype, size, monkeypatch):
    """Round 5: in 16-bit storage the gradient of the 32-channel-level concat buffer is produced as two dense 32-channel tensors (two
    data-gradient launches on the weight halves) instead of one [voxel][64] tensor, so that the kernels reading ONE half of it touch
    whole 128-byte lines.  Same arithmetic per output channel: where both forms run the same kernel every parameter gradient is equal bit for bit
    (DGTTA_SPLIT_CAT_GRAD=0 is the single-tensor form)."""
    _, net = _nets(5, dtype)
    net.train()
    net.exact_zero_bias_grad = True      # (a conv bias in front of InstanceNorm has a zero gradient: without this, rounding noise)
    for p in net.parameters():
        p.requires_grad_(True)
    torch.manual_seed(3)
    x = torch.randn(2, 12, *size, device=DEV)
    gout = torch.randn(2, 105, *size, device=DEV)

    def run(flag):
        monkeypatch.setenv("DGTTA_SPLIT_CAT_GRAD", flag)
        for p in net.parameters():
            p.grad = None
        out = net(x)
        out.backward(gout)
        torch.cuda.synchronize()
        return [p.grad.clone() for n, p in net.named_parameters() if p.grad is not None]

    g1, g0 = run("1"), run("0")
    assert len(g1) == len(g0) > 60
    assert all(torch.isfinite(a).all() for a in g1) and max(float(a.abs().max()) for a in g1) > 0
    if size == (32, 32, 32):      # both forms run the same kernel: the same bits
        assert all(torch.equal(a, b) for a, b in zip(g1, g0))
    else:
        # (here the dispatcher picks the ring kernel for the 64-channel call - twice the jobs - and the row-reuse kernel for the
        # halves: other fp32 summation orders, so 16-bit roundings of the gradient differ in a few elements; at 128^3 both take the
        # ring kernel and bench.py's loss trajectory is unchanged to the last digit, profiles/r05_ab.txt)
        for a, b in zip(g1, g0):
            if float(b.abs().max()) > 0:
                cos = float((a.double().flatten() @ b.double().flatten()) / (a.double().norm() * b.double().norm()))
                assert cos > 0.9999, cos
