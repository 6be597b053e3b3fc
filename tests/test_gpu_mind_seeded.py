"""Seeded in-kernel MIND noise on the GPU: dgtta_mind3d_noise_fill against the numpy restatement of the definition
(tests/philox_ref.py), its statistics, and dgtta_mind3d_fwd_seeded / ops.mind3d(seed=...) / mind.kernel_noise against the
tensor path fed with the same field.  Shapes: the smallest that span 2 x 2 x 2 tiles of 8 x 8 x 32 with a ragged edge."""
import math

import numpy as np
import pytest
import torch

import philox_ref
from conftest import SMALL_CFG

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 20240704


def _close(a, b, atol, rtol=0.0, what=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    err = (a - b).abs()
    worst = float((err - rtol * b.abs()).max())
    print(f"{what}: max abs err {float(err.max()):.3e}, max (err - {rtol:g}|ref|) {worst:.3e}, limit {atol:g}")
    assert worst <= atol, f"{what}: max err {float(err.max()):.3e} (limit {atol:g}+{rtol:g}*|ref|)"


def test_noise_fill_matches_the_definition():
    """Limit 1e-5: the uniforms are exact, the radius is <= 5.77, and full-precision logf / sincos leave a few 1e-6 (a float32
    numpy evaluation of the same formula is 1.3e-6 from the float64 one)."""
    from dg_tta_amd import ops
    seed, offset = 0x123456789ABCDEF0, 2 ** 32 + 5          # both high words in use
    got = ops.mind3d_noise(2, 9, 10, 37, seed, offset=offset, b0=3, device=DEV)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 12, 9, 10, 37) and got.is_contiguous()
    ref = philox_ref.mind_noise(seed, offset, 3, 2, 9, 10, 37)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    print(f"noise_fill vs float64 definition: max abs err {err:.3e} (limit 1e-5)")
    assert err <= 1e-5


def test_noise_is_a_function_of_seed_offset_sample_channel_voxel():
    from dg_tta_amd import ops
    two = ops.mind3d_noise(2, 9, 10, 37, SEED, offset=1, b0=0, device=DEV)
    assert torch.equal(two[1], ops.mind3d_noise(1, 9, 10, 37, SEED, offset=1, b0=1, device=DEV)[0])      # bitwise
    assert torch.equal(two, ops.mind3d_noise(2, 9, 10, 37, SEED, offset=1, device=DEV))
    assert not torch.equal(two[0], two[1])
    for seed, offset in ((SEED, 2), (SEED + 1, 1), (SEED + 2 ** 32, 1), (SEED, 1 + 2 ** 32)):
        assert not torch.equal(ops.mind3d_noise(2, 9, 10, 37, seed, offset=offset, device=DEV), two)
    # the voxel enters as its linear index: the same V under another shape is the same field
    assert torch.equal(ops.mind3d_noise(2, 9 * 10, 1, 37, SEED, offset=1, device=DEV).reshape(two.shape), two)


@pytest.mark.parametrize("seed", [20240704, 7, 0])
def test_noise_moments(seed):
    """N = 2 x 12 x 16 x 16 x 40 = 245 760 values; every bound is 5 sigma of the statistic under the hypothesis of independent
    standard normals (mean: 5/sqrt(N); variance: 5 sqrt(2/N); correlation of two channels of N/12 values: 5/sqrt(N/12);
    Kolmogorov distance: 1.95/sqrt(N))."""
    from dg_tta_amd import ops
    n = ops.mind3d_noise(2, 16, 16, 40, seed, device=DEV).cpu().double()
    n4 = ops.mind3d_noise(2, 16, 16, 40, seed, offset=4, device=DEV).cpu().double()
    N = n.numel()
    assert N == 245760 and bool(torch.isfinite(n).all())
    stats = dict(mean=float(n.mean()), var=float(n.var(unbiased=False)))
    c = torch.corrcoef(n.permute(1, 0, 2, 3, 4).reshape(12, -1))
    stats["corr"] = float((c - torch.eye(12, dtype=c.dtype)).abs().max())
    stats["lag_w"] = float((n[..., 1:] * n[..., :-1]).mean())
    stats["lag_h"] = float((n[..., 1:, :] * n[..., :-1, :]).mean())
    stats["lag_d"] = float((n[:, :, 1:] * n[:, :, :-1]).mean())
    stats["samples"] = float((n[0] * n[1]).mean())
    stats["offsets"] = float((n * n4).mean())
    flat = n.reshape(-1).sort().values
    cdf = 0.5 * (1 + torch.erf(flat / math.sqrt(2)))
    k = torch.arange(N, dtype=torch.float64)
    stats["ks"] = float(torch.maximum(((k + 1) / N - cdf).max(), (cdf - k / N).max()))
    print(f"seed {seed}: " + ", ".join(f"{a} {b:.5f}" for a, b in stats.items()))
    assert abs(stats["mean"]) <= 0.0101
    assert abs(stats["var"] - 1) <= 0.0143
    assert stats["corr"] <= 0.035
    for key in ("lag_w", "lag_h", "lag_d", "samples", "offsets"):
        assert abs(stats[key]) <= 0.0101, key
    assert stats["ks"] <= 0.00393


_IMG = {}


def _img(shape):
    if shape not in _IMG:
        _IMG[shape] = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))) * 1.5 + 0.5
    return _IMG[shape]


@pytest.mark.parametrize("shape", [(2, 1, 16, 16, 40), (1, 1, 9, 10, 37)])
@pytest.mark.parametrize("delta,sigma", [(1, 1.0), (1, 0.5), (2, 2.0)])      # (2, 2): the R = 3, CG = 2 kernel, second-pass columns
def test_fwd_seeded_equals_fwd_on_the_filled_noise(shape, delta, sigma):
    """The limits are the ones tests/test_gpu_ops.py holds the tensor kernel to against the oracle."""
    from dg_tta_amd import ops
    from oracle import mind as omind
    b, _, d, h, w = shape
    offset, b0 = 3, 1
    img = _img(shape)
    tol = dict(atol=2e-6, rtol=2e-5) if (delta, sigma) == (1, 1.0) else dict(atol=3e-5)
    noise = ops.mind3d_noise(b, d, h, w, SEED, offset=offset, b0=b0, device=DEV)
    via_tensor = ops.mind3d(img.to(DEV), noise, delta=delta, sigma=sigma)
    seeded = ops.mind3d(img.to(DEV), seed=SEED, offset=offset, b0=b0, delta=delta, sigma=sigma)
    _close(seeded, via_tensor, what=f"seeded vs tensor path {shape} delta={delta} sigma={sigma}", **tol)
    ref = omind.mind3d(img, torch.from_numpy(philox_ref.mind_noise(SEED, offset, b0, b, d, h, w)).float(), delta=delta, sigma=sigma)
    _close(seeded, ref, what=f"seeded vs oracle on philox_ref noise {shape} delta={delta} sigma={sigma}", **tol)
    assert not torch.equal(seeded, ops.mind3d(img.to(DEV), seed=SEED, offset=offset + 1, b0=b0, delta=delta, sigma=sigma))


def test_fwd_seeded_fp16_channels_last_output():
    from dg_tta_amd import ops
    shape = (2, 1, 16, 16, 40)
    img = _img(shape).to(DEV)
    noise = ops.mind3d_noise(2, 16, 16, 40, SEED, device=DEV)
    kw = dict(out_format="ndhwc", out_ldc=16, out_dtype=torch.float16)
    a = ops.mind3d(img, seed=SEED, **kw)
    b = ops.mind3d(img, noise, **kw)
    assert a.dtype == torch.float16 and tuple(a.shape) == (2, 16, 16, 40, 16) and float(a[..., 12:].abs().max()) == 0.0
    _close(a[..., :12], b[..., :12], atol=4e-3, what="seeded fp16 ndhwc vs tensor path")


def test_grouping_keeps_every_samples_noise():
    """groups = 2 of a seeded call = two calls of B/2 samples with b0 = 0 and b0 = 2 (one variance-clamp mean per group, as
    `groups` always implied); flat regions put voxels on the clamp, so the groups = 1 result (one mean) differs."""
    from dg_tta_amd import ops
    img = torch.randn(4, 1, 16, 16, 40, generator=torch.Generator().manual_seed(1))
    img[:, :, :, :8] = 0.25                      # flat half: var there is noise only, far below 1e-3 x the call's mean
    img[2:] *= 30.0                              # the second group's mean is far from the first's
    img = img.to(DEV)
    grouped = ops.mind3d(img, seed=SEED, offset=2, groups=2)
    parts = [ops.mind3d(img[:2], seed=SEED, offset=2, b0=0), ops.mind3d(img[2:], seed=SEED, offset=2, b0=2)]
    assert torch.equal(grouped, torch.cat(parts))
    assert not torch.equal(grouped, ops.mind3d(img, seed=SEED, offset=2))
    assert not torch.equal(parts[1], ops.mind3d(img[2:], seed=SEED, offset=2, b0=0))
    assert torch.equal(ops.mind3d_noise(4, 16, 16, 40, SEED, offset=2, device=DEV)[2:],
                       ops.mind3d_noise(2, 16, 16, 40, SEED, offset=2, b0=2, device=DEV))


def test_defaults_unchanged_and_kernel_noise_context():
    from dg_tta_amd import ops
    from dg_tta_amd.mind import MIND3D, kernel_noise, mind_hook
    x = _img((2, 1, 16, 16, 40)).to(DEV)

    def default_path():
        torch.manual_seed(5)
        out = MIND3D()(x)
        torch.manual_seed(5)
        assert torch.equal(out, ops.mind3d(x, torch.randn(2, 12, 16, 16, 40, device=DEV)))
        return out

    before = default_path()
    torch.manual_seed(6)
    state = torch.cuda.get_rng_state(DEV)
    with kernel_noise(SEED):
        a0 = MIND3D()(x)                       # offset 0
        a1 = mind_hook(None, (x,))             # offset 1
        given = MIND3D()(x, torch.zeros(2, 12, 16, 16, 40, device=DEV))      # a tensor handed in is used
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)
    assert torch.equal(a0.contiguous(), ops.mind3d(x, seed=SEED, offset=0))
    assert torch.equal(a1.contiguous(), ops.mind3d(x, seed=SEED, offset=1)) and not torch.equal(a0, a1)
    assert torch.equal(given.contiguous(), ops.mind3d(x, torch.zeros(2, 12, 16, 16, 40, device=DEV)))
    assert torch.equal(default_path(), before)


def test_inference_inside_kernel_noise_is_reproducible_and_matches_the_cpu(monkeypatch):
    """The small network of tests/test_inference.py over a volume of 20 windows (two window batches, the second ragged), two
    ensemble members: inside kernel_noise(s) the accumulators and label maps do not depend on the torch seed set before the
    run or on the side-stream prefetch, the device generator is left alone, and the accumulated logits are those of the CPU
    members on oracle.mind.mind3d(window, philox_ref noise at offset = the MIND call's rank, b = the window's index in it)."""
    from dg_tta_amd.mind import kernel_noise, mind_hook
    from dg_tta_amd.tta import inference as pinf
    from dg_tta_amd.unet import HipPlainConvUNet
    from oracle import inference as oinf, mind as omind, unet as ounet
    patch = [16, 16, 16]
    data = torch.randn(1, 24, 24, 44, generator=torch.Generator().manual_seed(0))
    members = [ounet.perturb_affine(ounet.init_he(ounet.PlainConvUNetOracle(SMALL_CFG), s), s + 1) for s in (1, 2)]
    params = [m.state_dict() for m in members]
    net = HipPlainConvUNet(SMALL_CFG, conv_impl=1).to(DEV)
    net.register_forward_pre_hook(mind_hook)
    nwin = 2 * 2 * 5
    nbatch = -(-nwin // pinf.WINDOW_BATCH)
    assert nbatch >= 2

    def run(torch_seed, prefetch):
        monkeypatch.setenv("DGTTA_INFER_PREFETCH", prefetch)
        assert pinf._mind_ahead_ok(net, DEV) == (prefetch == "1")
        torch.manual_seed(torch_seed)
        state = torch.cuda.get_rng_state(DEV)
        with kernel_noise(SEED):
            acc, nsum, crop = pinf.predict_ensemble(data, net, params, patch)
        assert torch.equal(torch.cuda.get_rng_state(DEV), state)
        seg = torch.as_tensor(pinf.export_segmentation(acc, nsum, crop, None, None, None))
        return acc.clone(), nsum.clone(), crop, seg

    acc, nsum, crop, seg = run(1, "1")
    for torch_seed, prefetch in ((2, "1"), (3, "0")):
        acc2, nsum2, _, seg2 = run(torch_seed, prefetch)
        assert torch.equal(acc2, acc) and torch.equal(nsum2, nsum) and torch.equal(seg2, seg)
    with kernel_noise(SEED + 1):
        other = pinf.predict_ensemble(data, net, params, patch)[0]
    assert not torch.equal(other, acc)

    calls = [0]

    def cpu_model(m, member):
        def f(x):
            j = calls[0] - member * nwin                  # window index of this member, in the product's batch order
            calls[0] += 1
            k, b = member * nbatch + j // pinf.WINDOW_BATCH, j % pinf.WINDOW_BATCH
            noise = torch.from_numpy(philox_ref.mind_noise(SEED, k, b, 1, *patch)).float()
            return m(omind.mind3d(x, noise))
        return f

    ref = oinf.ensemble_logits([cpu_model(m, i) for i, m in enumerate(members)], data, patch)
    assert calls[0] == 2 * nwin
    got = (acc / nsum[..., None] / len(members))[tuple(crop)].permute(3, 0, 1, 2).cpu()
    err = float((got - ref).abs().max())
    print(f"accumulated logits vs CPU members on philox_ref noise: max abs err {err:.3e}, limit {2e-4 * float(ref.abs().max()):.3e}")
    assert err < 2e-4 * float(ref.abs().max())
    ref_seg = ref.argmax(0)
    top2 = ref.topk(2, dim=0).values
    safe = (top2[0] - top2[1]) > 1e-3
    assert torch.equal(seg[safe], ref_seg[safe]) and (seg == ref_seg).float().mean() > 0.999
