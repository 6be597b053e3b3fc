"""GPU, network level: the InstanceNorm backward of the full-resolution block in front of the head with its gz never stored
(DGTTA_HEAD_GZ_FOLD, dgtta_seghead_warp_bwd_g16_d16 + dgtta_instnorm_lrelu_bwd_head) against the path that writes gz and reads
it back (DGTTA_HEAD_GZ_FOLD=0).

Pattern and limits of tests/test_gpu_full_topology.py::test_dgrad_with_fused_instancenorm_statistics_matches_the_reduction_pass:
the two paths differ by where one 16-bit rounding sits (gz = W^T float(round(acc)) unrounded instead of round(W^T acc)), which
moves single roundings of dy that the LeakyReLU kinks of the layers below amplify - every parameter gradient
agrees to 3e-3 of its scale with cosine > 0.9999 in fp16, 4e-2 / 0.998 in bf16 - and some tensor differs in its bits: the
new path really ran."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_head_gz_fold_matches_the_stored_gz_path(dtype, monkeypatch):
    from dg_tta_amd import ops
    from dg_tta_amd.synthetic import he_init_
    from dg_tta_amd.unet import HipPlainConvUNet
    from oracle import tta as otta
    torch.manual_seed(4)
    net = he_init_(HipPlainConvUNet(act_dtype=dtype), seed=7)
    for m in net.modules():          # non-trivial affine parameters
        if m.__class__.__name__ == "HipInstanceNorm3d":
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)
    net = net.to(DEV)
    net.set_selected_classes(torch.arange(16) * 3)
    net.exact_zero_bias_grad = True      # (a conv bias in front of InstanceNorm has a zero gradient: pure rounding noise otherwise)
    B, N = 2, 64                          # one pair of branches
    x = torch.rand(B, 12, N, N, N, device=DEV)
    _, rinv = otta.rand_affine_from_draw(torch.randn(B, 3, 4), 0.08)
    rinv = rinv.float().contiguous()
    assert net.can_fuse_output_warp(x.shape, rinv)

    def run(flag):
        monkeypatch.setenv("DGTTA_HEAD_GZ_FOLD", flag)
        net.zero_grad()
        with net.fuse_output_warp(rinv.to(DEV), rinv):
            y = net(x)
        ta, tb = y[:B // 2], y[B // 2:]
        ta._dgtta_pair = tb._dgtta_pair = y
        ta._dgtta_guard_items = tb._dgtta_guard_items = 1
        loss, _ = ops.consistency_loss(ta, tb, 1)
        (loss * 1024.0).backward()
        torch.cuda.synchronize()
        return float(loss.detach()), {n: p.grad.detach().float().clone() for n, p in net.named_parameters() if p.grad is not None}

    (l1, g1), (l0, g0) = run("1"), run("0")
    assert l1 == l0 and set(g1) == set(g0)
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
    assert differs > 0          # gz was rebuilt from d16 (one rounding moved somewhere)
    # the head's own gradient does not depend on the switch: the same d16 rows feed the same kernels
    for n in ("decoder.seg_layers.3.weight", "decoder.seg_layers.3.bias"):
        assert torch.equal(g1[n], g0[n]), n
