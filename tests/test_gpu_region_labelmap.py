"""GPU: the two label-map kernels of region heads - dgtta_feature_head_regions (csrc/window_features.hip, feature-space
accumulators, matrix cores) and dgtta_logits_regions (csrc/region_map.hip, logits-space accumulator) - against
region_ref.region_label_map, in EVERY voxel.

Features, weights and biases are small multiples of 2^-6 and the window weights n(v) multiples of 2^-2: every product is a
multiple of 2^-14 and every partial sum of a voxel's 32 M + 1 terms stays below 2^6, i.e. exact in fp32 IN ANY ORDER (20 bits) -
the matrix-core accumulation, the float64 reference and any other order see the same number, exact zeros included (asserted:
_assert_exact_sums).  A logit of exactly 0 is not in the region.

Then through run_inference on a two-stage network with mirroring on and off: the feature-space and the logits-space path give
the same map outside the voxels whose smallest |logit| is below 1e-5 of the largest |logit| of the float64 reference (at most
0.1 % of the voxels, asserted on the reference alone)."""
import functools

import numpy as np
import pytest
import torch

import region_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _assert_exact_sums(terms):
    """terms [T][V][R] float64 (a voxel's T addends per output): multiples of 2^-14 whose fp32 sums equal the float64 one in
    three orders."""
    assert np.array_equal(np.round(terms * 2 ** 14), terms * 2 ** 14) and np.abs(terms).sum(axis=0).max() < 64
    t32 = terms.astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), terms)
    want = terms.sum(axis=0)
    fwd, rev = t32[0].copy(), t32[-1].copy()
    for k in range(1, terms.shape[0]):
        fwd, rev = fwd + t32[k], rev + t32[-1 - k]
    assert fwd.dtype == np.float32 and np.array_equal(fwd, want) and np.array_equal(rev, want)
    assert np.array_equal(t32.sum(axis=0, dtype=np.float32), want)


@functools.lru_cache(maxsize=None)
def _accumulators(M, R, V):
    """(facc [M][V][32], nsum [V], w [M][R][32], b [M][R], logits [V][R] float64 = sum_m w_m . facc_m + nsum bsum) on the exact grid."""
    rng = np.random.RandomState(1000 * M + 10 * R + V % 97)
    facc = rng.randint(-24, 25, size=(M, V, 32)) / 64.0
    w = rng.randint(-24, 25, size=(M, R, 32)) / 64.0
    b = rng.randint(-16, 17, size=(M, R)) / 64.0
    nsum = rng.randint(1, 9, size=V) / 4.0
    if V >= 8:                                   # exact-zero logits: no features and a zero bias sum in output 0
        facc[:, ::5] = 0.0
        b[:, 0] = 0.0
    terms = np.concatenate([(facc[m][:, None, :] * w[m][None, :, :]).transpose(2, 0, 1) for m in range(M)] +
                           [(nsum[:, None] * b.sum(0)[None, :])[None]])
    _assert_exact_sums(terms)
    logits = terms.sum(axis=0)
    if V >= 8:
        assert (logits == 0).any() and (logits > 0).any() and (logits < 0).any()
    return facc, nsum, w, b, logits


def _orders(R):
    asc = list(range(1, R + 1))
    if R == 1:
        return [[1], [9]]
    if R == 3:
        return [asc, [2, 7, 1], [4, 4, 9]]
    desc = asc[::-1]
    return [asc, desc, [5] * 2 + desc[2:]]


def _feature_map(facc, nsum, w, b, order):
    from dg_tta_amd import ops
    M, V = facc.shape[:2]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    out = ops.feature_head_regions(dev(facc).reshape(M, V, 1, 1, 32), dev(nsum).reshape(V, 1, 1), dev(w), dev(b).sum(0), order)
    assert out.dtype == torch.int64 and tuple(out.shape) == (V, 1, 1)
    return out.reshape(V).cpu().numpy()


@pytest.mark.parametrize("V", [1, 31, 32, 33, 4129])
@pytest.mark.parametrize("R", [1, 3, 32])
@pytest.mark.parametrize("M", [1, 3])
def test_both_kernels_equal_the_reference_in_every_voxel(M, R, V):
    """V: below, at and above one 32-voxel tile of a wave; 4129 = 130 tiles, more than the 4 waves of one workgroup, ragged."""
    from dg_tta_amd import ops
    facc, nsum, w, b, logits = _accumulators(M, R, V)
    for order in _orders(R):
        want = region_ref.region_label_map(logits, order)
        assert np.array_equal(_feature_map(facc, nsum, w, b, order), want), f"feature space, order {order}"
        for dt in (torch.float32, torch.float16):            # (the fp16 rounding keeps every sign and every zero)
            acc = torch.from_numpy(logits).to(DEV).to(dt)
            got = ops.logits_regions(acc.reshape(V, 1, 1, R), order)
            assert got.dtype == torch.int64 and np.array_equal(got.reshape(V).cpu().numpy(), want), f"logits space {dt}, order {order}"
    if V >= 8 and R > 1:                                         # (the inputs exercise the rule: several labels occur)
        assert len(np.unique(region_ref.region_label_map(logits, _orders(R)[0]))) > 2


@pytest.mark.parametrize("R", [1, 3, 32])
def test_single_label_regions_with_one_positive_output_are_the_argmax(R):
    """R single-label regions ordered by label, exactly one positive output per voxel: the map is argmax + 1 mapped through the
    order (here the order is 1 .. R, so argmax + 1 itself)."""
    from dg_tta_amd import ops
    V = 333
    rng = np.random.RandomState(R)
    hot = rng.randint(0, R, size=V)
    facc = -np.ones((1, V, 32)) * 0.5
    facc[0, np.arange(V), hot] = 0.75                        # channel r carries output r
    w = np.zeros((1, R, 32))
    w[0, np.arange(R), np.arange(R)] = 1.0
    b, nsum = np.zeros((1, R)), np.ones(V)
    logits = facc[0][:, :R].copy()
    assert np.array_equal((logits > 0).sum(1), np.ones(V))
    order = list(range(1, R + 1))
    want = logits.argmax(1) + 1
    assert np.array_equal(region_ref.region_label_map(logits, order), want)
    assert np.array_equal(_feature_map(facc, nsum, w, b, order), want)
    got = ops.logits_regions(torch.from_numpy(logits).float().to(DEV), order)
    assert np.array_equal(got.cpu().numpy(), want)


def test_argument_checks():
    from dg_tta_amd import _lib, ops
    from dg_tta_amd._lib import DgttaError
    import ctypes
    lib, st = _lib.load(), _lib.stream_of(torch.device(DEV))
    facc, nsum, w, b, logits = _accumulators(1, 3, 33)
    with pytest.raises(ValueError, match="regions_class_order"):
        _feature_map(facc, nsum, w, b, [1, 2])
    with pytest.raises(ValueError, match="regions_class_order"):
        _feature_map(facc, nsum, w, b, [1, 0, 2])
    with pytest.raises(ValueError, match="regions_class_order"):
        ops.logits_regions(torch.zeros(4, 3, device=DEV), [1, 2, 3, 4])
    assert ops.feature_head_regions_supported(3, 32) and ops.feature_head_regions_supported(35, 1)
    assert not ops.feature_head_regions_supported(36, 3) and not ops.feature_head_regions_supported(1, 33)
    t = torch.zeros(36 * 64 * 32, dtype=torch.float32, device=DEV)
    o = torch.zeros(64, dtype=torch.int64, device=DEV)
    p, good, bad = t.data_ptr(), (ctypes.c_int * 3)(1, 2, 3), (ctypes.c_int * 3)(1, -2, 3)

    def feat(M=1, Cin=32, R=3, V=64, order=good, stride=64 * 32, facc=p):
        return lib.dgtta_feature_head_regions(facc, stride, p, p, p, M, Cin, R, V, order, o.data_ptr(), st)
    assert feat() == 0
    assert feat(R=0) == -1 and feat(V=0) == -1 and feat(order=bad) == -1 and feat(facc=None) == -1 and feat(facc=p + 4) == -1
    assert feat(M=2, stride=64 * 32 - 4) == -1 and feat(Cin=16) == -2 and feat(M=36) == -2
    assert lib.dgtta_feature_head_regions(p, 0, p, p, p, 1, 32, 33, 64, (ctypes.c_int * 33)(*range(1, 34)), o.data_ptr(), st) == -2
    assert lib.dgtta_logits_regions(p, 0, 3, 64, good, o.data_ptr(), st) == 0
    assert lib.dgtta_logits_regions(p, 0, 3, 64, bad, o.data_ptr(), st) == -1
    assert lib.dgtta_logits_regions(p, 0, 0, 64, good, o.data_ptr(), st) == -1
    assert lib.dgtta_logits_regions(p, 0, 3, 0, good, o.data_ptr(), st) == -1
    assert lib.dgtta_logits_regions(p, 1, 3, 64, good, o.data_ptr(), st) == -2            # bf16 rows
    with pytest.raises(DgttaError, match=r"code -1\)"):
        _lib.check(lib.dgtta_logits_regions(None, 0, 3, 64, good, o.data_ptr(), st), "dgtta_logits_regions")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ through run_inference
REGION_NET = dict(features=(32, 40), strides=(1, 2), n_conv_enc=(1, 1), n_conv_dec=(1,), in_channels=1, num_classes=3)
SEED = 3             # (chosen so that the float64 reference sets aside 0.013 % / 0.005 % of the voxels and every label occurs)
MIRROR = (0, 2)      # four passes per window, the last axis (reversed runs) among them
ORDER = [2, 7, 1]


@functools.lru_cache(maxsize=None)
def _network_case():
    """(data, patch, state dict, float64 reference logits [R, X, Y, Z] without and with mirroring) - computed once on the CPU."""
    import mirror_ref as mr
    from oracle import inference as oinf, unet as ounet
    torch.manual_seed(SEED)
    data = torch.randn(1, 40, 33, 48)
    patch = [24, 24, 32]
    model = ounet.perturb_affine(ounet.init_he(ounet.PlainConvUNetOracle(REGION_NET), SEED), SEED + 1)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    m64 = model.double()
    with torch.no_grad():
        plain = oinf.ensemble_logits([lambda x: m64(x.double())], data, patch).double()
        mirrored = oinf.ensemble_logits([mr.mirrored(lambda x: m64(x.double()), MIRROR)], data, patch).double()
    return data, patch, state, plain, mirrored


@pytest.mark.parametrize("mirror_axes", [None, MIRROR])
def test_run_inference_feature_and_logits_space_agree(mirror_axes, monkeypatch):
    from dg_tta_amd.tta import inference as pinf
    from dg_tta_amd.unet import HipPlainConvUNet
    data, patch, state, plain, mirrored = _network_case()
    ref = (plain if mirror_axes is None else mirrored).permute(1, 2, 3, 0).numpy()
    near = np.abs(ref).min(axis=-1) < 1e-5 * np.abs(ref).max()
    print(f"\nmirror {mirror_axes}: {near.mean():.4%} of the voxels set aside; positive outputs per region "
          f"{(ref > 0).mean(axis=(0, 1, 2)).round(3).tolist()}")
    assert near.mean() <= 0.001
    want = region_ref.region_label_map(ref, ORDER)
    assert len(np.unique(want)) == 4                                      # every label of the order and the background occur
    net = HipPlainConvUNet(REGION_NET, conv_impl=1).to(DEV)
    maps = {}
    for mode in ("features", "fp32"):
        monkeypatch.setenv("DGTTA_WINDOW_ACC", mode)
        with torch.no_grad():
            assert pinf._can_accumulate_features(net, 1, regions=True)
        acc, _, _ = pinf.predict_ensemble(data, net, [state], patch, mirror_axes, regions=True)
        assert isinstance(acc, pinf.WindowFeatures) == (mode == "features")
        seg = pinf.run_inference(data, net, [state], patch, mirror_axes=mirror_axes, regions_class_order=ORDER)
        assert tuple(seg.shape) == (40, 33, 48) and seg.dtype == torch.int64
        maps[mode] = seg.numpy()
        assert set(np.unique(maps[mode]).tolist()) <= {0, *ORDER}
    assert np.array_equal(maps["features"][~near], maps["fp32"][~near])
    safe = np.abs(ref).min(axis=-1) > 1e-3 * np.abs(ref).max()             # (fp32 network against the float64 one: a wider margin)
    assert safe.mean() > 0.9 and np.array_equal(maps["features"][safe], want[safe])
    with pytest.raises(ValueError, match="regions_class_order"):
        pinf.run_inference(data, net, [state], patch, regions_class_order=[1, 2])


@pytest.mark.parametrize("act", [torch.float32, torch.float16])
def test_a_head_of_one_region_through_the_network(act, monkeypatch):
    """R = 1 through the layers the kernel tests do not reach: the head's forward and backward under the region loss, and both
    window accumulators of run_inference (16-bit storage takes the fused head + accumulate in logits space)."""
    from dg_tta_amd import ops
    from dg_tta_amd.synthetic import he_init_
    from dg_tta_amd.tta import inference as pinf
    from dg_tta_amd.unet import HipPlainConvUNet
    net = he_init_(HipPlainConvUNet(dict(REGION_NET, num_classes=1), act_dtype=act, deep_supervision=True), seed=5).to(DEV)
    for p in net.parameters():
        p.requires_grad_(True)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 1, 16, 16, 16, generator=g).to(DEV)
    y = (torch.rand(2, 16, 16, 16, generator=g) > 0.7).long().to(DEV)
    outs = net(x)
    assert all(o.shape[1] == 1 for o in outs)
    loss, _ = ops.deep_supervision_region_loss(outs, y, np.array([0, 1], dtype=np.uint32))
    torch.autograd.backward(loss, grad_tensors=torch.full((), float(net.loss_scale), dtype=torch.float32, device=DEV))
    head = net.decoder.seg_layers[-1]
    assert np.isfinite(float(loss.detach())) and all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)
    assert float(head.weight.grad.abs().max()) > 0 and tuple(head.weight.shape[:2]) == (1, 32)
    net.deep_supervision = False
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    data = torch.randn(1, 24, 20, 28, generator=g)
    patch, maps = [16, 16, 16], {}
    for mode in ("features", "fp32"):
        monkeypatch.setenv("DGTTA_WINDOW_ACC", mode)
        with torch.no_grad():
            assert pinf._can_accumulate_features(net, 1, regions=True)
            if mode == "fp32":
                assert pinf._can_fuse_head_accumulate(net) == (act == torch.float16)
        maps[mode] = pinf.run_inference(data, net, [state], patch, regions_class_order=[5]).numpy()
        assert set(np.unique(maps[mode]).tolist()) == {0, 5}
    acc, nsum, crop = pinf.predict_ensemble_logits(data, net, [state], patch)
    logit = (acc / nsum[..., None])[tuple(crop)][..., 0].float().cpu().numpy()
    near = np.abs(logit) < (1e-2 if act == torch.float16 else 1e-4) * np.abs(logit).max()
    print(f"\nR = 1, {act}: {near.mean():.3%} of the voxels near zero")
    assert near.mean() < 0.05
    assert np.array_equal(maps["fp32"], np.where(logit > 0, 5, 0))
    assert np.array_equal(maps["features"][~near], maps["fp32"][~near])
