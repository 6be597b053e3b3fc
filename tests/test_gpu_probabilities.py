"""GPU: the softmax end of the ensemble prediction - dgtta_feature_head_softmax (fused head + softmax on the matrix cores),
dgtta_softmax_merge_f64 / dgtta_softmax_finalize_f64 (class-group export path), inference.export_probabilities and the plan keys
`inference_save_probabilities` / `inference_save_uncertainty` - against the float64 restatement tests/softmax_ref.py, which
tests/test_softmax_ref.py licenses against torch.softmax in float64.

Every comparison is against float64 with a bound derived in softmax_ref.py from the number formats (asserted with a factor of 2 for
second-order terms); no kernel is compared with itself or with fp32 torch.  Labels are compared as integers with the argmax
kernels the product already has."""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import softmax_ref as ref      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]
PLANS = json.loads((ROOT / "dg_tta_amd" / "__resources__" / "model_skeleton" / "plans.json").read_text())

# (M, C, V): a tail tile (V % 32 != 0) with 1 and 3 members at the plan's 105 classes; 31 padding classes in the second block; one
# block with few classes; two classes; the widest head (four full blocks); no tail and no padding
SHAPES = [(1, 105, 64 * 40 + 17), (3, 105, 5000), (2, 33, 777), (4, 7, 300), (1, 2, 255), (2, 128, 513), (3, 32, 1024)]
FAMILIES = ["spread", "large", "overflow", "zero", "dominant"]


def _inputs(M, C, V, family, seed=0):
    """fp32 numpy inputs (facc [M,V,32], nsum [V], w [M,C,32], bsum [C]); nsum spread over [1e-3, 40] in every family."""
    rng = np.random.default_rng(seed + 131 * C + V)
    nsum = np.exp(rng.uniform(np.log(1e-3), np.log(40.0), V)).astype(np.float32)
    feat = rng.standard_normal((M, V, 32)).astype(np.float32)
    facc = (feat * nsum[None, :, None]).astype(np.float32)
    w = (rng.standard_normal((M, C, 32)) * 0.3).astype(np.float32)
    bsum = rng.standard_normal(C).astype(np.float32)
    if family == "large":          # |l| reaches about 60 on some voxels: a forgotten 1 / (M n) cannot hide
        l, _ = ref.head_logits(facc, nsum, w, bsum)
        s = np.float32(60.0 / np.abs(l).max())
        w, bsum = w * s, bsum * s
    elif family == "overflow":     # a logit near +300: exp overflows without the max subtraction
        bsum[C // 2] = 300.0 * M
    elif family == "zero":         # p = 1 / C exactly to rounding, entropy ln C, label 0 - padding classes must stay out of S
        w[:], bsum[:] = 0.0, 0.0
    elif family == "dominant":     # one class far ahead: entropy must stay >= 0 and finite
        w *= 0.05
        bsum[C - 1] = 30.0 * M
    return facc, nsum, w, bsum


def _sel(C, K, seed):
    """K distinct classes (all of them when C < K), unsorted, class C - 1 in front of class 0."""
    if K == 1:
        return [C - 1]
    rest = [c for c in np.random.default_rng(seed).permutation(C).tolist() if c not in (0, C - 1)][:min(K, C) - 2]
    return rest[:len(rest) // 2] + [C - 1] + rest[len(rest) // 2:] + [0]


def _to_dev(facc, nsum, w, bsum):
    M, V = facc.shape[:2]
    return (torch.from_numpy(facc).reshape(M, 1, 1, V, 32).to(DEV), torch.from_numpy(nsum).reshape(1, 1, V).to(DEV),
            torch.from_numpy(w).to(DEV), torch.from_numpy(bsum).to(DEV))


def _ratio(err, bound):
    return float((err / bound).max())


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M,C,V", SHAPES)
def test_fused_head_softmax_against_float64(M, C, V, family):
    """dgtta_feature_head_softmax on every shape x input family, K in {1, 16} (unsorted, with class 0 and class C - 1), fp32 and
    fp16 planes: the label is feature_head_argmax's integer for integer; P, confidence and entropy lie within twice the derived
    bound of the float64 restatement (measured max(err / bound): P 0.61 with fp32 planes, 1.00 with fp16 planes - the storage
    rounding itself -, confidence 0.04, entropy 0.11)."""
    from dg_tta_amd import ops
    facc, nsum, w, bsum = _inputs(M, C, V, family)
    l, delta = ref.head_logits(facc, nsum, w, bsum)
    st = ref.softmax_stats(l)
    dev = _to_dev(facc, nsum, w, bsum)
    want_label = ops.feature_head_argmax(*dev).reshape(V).cpu().numpy()
    for K in (1, 16):
        sel = _sel(C, K, K + C)
        assert len(set(sel)) == len(sel) == min(K, C) and (K == 1 or (0 in sel and C - 1 in sel))
        for pt, npt in ((torch.float32, np.float32), (torch.float16, np.float16)):
            label, conf, ent, probs = ops.feature_head_softmax(*dev, sel, prob_dtype=pt)
            assert probs.dtype == pt and tuple(probs.shape) == (len(sel), 1, 1, V) and label.dtype == torch.int64
            label, conf, ent = (t.reshape(V).cpu().numpy() for t in (label, conf, ent))
            probs = probs.reshape(len(sel), V).cpu().numpy().astype(np.float64)
            assert np.array_equal(label, want_label)                      # the argmax kernel's integers
            pb32, hb = ref.bounds(st, delta, np.float32)
            pb, _ = ref.bounds(st, delta, npt)
            top = st["label"]
            r_p = _ratio(np.abs(probs - st["p"][:, sel].T), pb[:, sel].T)
            r_c = _ratio(np.abs(conf - st["confidence"]), pb32[np.arange(V), top])
            r_h = _ratio(np.abs(ent - st["entropy"]), hb)
            print(f"err/bound M={M} C={C} V={V} {family} K={len(sel)} {npt.__name__}: P {r_p:.3f} conf {r_c:.3f} entropy {r_h:.3f}")
            assert np.isfinite(conf).all() and np.isfinite(ent).all() and np.isfinite(probs).all()
            assert (ent >= 0).all() and (conf > 0).all() and (conf <= 1).all()
            assert r_p <= 2.0 and r_c <= 2.0 and r_h <= 2.0, (r_p, r_c, r_h)
    if family == "zero":
        assert (want_label == 0).all() and abs(float(ent.max()) - np.log(C)) < 1e-5 and abs(float(conf.min()) - 1.0 / C) < 1e-6


def test_fused_kernel_argument_checks():
    from dg_tta_amd import _lib, ops
    lib = _lib.load()
    facc, nsum, w, bsum = _to_dev(*_inputs(2, 150, 64, "spread"))
    out = [torch.empty(64, dtype=d, device=DEV) for d in (torch.int64, torch.float32, torch.float32, torch.float32)]

    def call(C, sel, M=2):
        return lib.dgtta_feature_head_softmax(facc.data_ptr(), facc.stride(0), nsum.data_ptr(), w.data_ptr(), bsum.data_ptr(), M, 32, C, 64,
                                              (ctypes.c_int * len(sel))(*sel), len(sel), ops.F32, *[o.data_ptr() for o in out], None)
    assert call(150, [0]) == -2 and b"128 classes" in lib.dgtta_last_error()            # DGTTA_ERR_UNSUPPORTED: the class-group path
    assert call(105, [3, 3]) == -1 and b"twice" in lib.dgtta_last_error()                # DGTTA_ERR_BADARG
    assert call(105, [105]) == -1 and call(105, [-1]) == -1
    with pytest.raises(ValueError):
        ops.feature_head_softmax(facc, nsum, w, bsum, [0, 0])
    with pytest.raises(_lib.DgttaError, match="128 classes"):
        ops.feature_head_softmax(facc, nsum, w, bsum, [0, 149])


# ------------------------------------------------------------------------------------------------ class-group path
def _group_values(acc, nsum, crop):
    """The float64 chunk values the export loop itself forms (dgtta_*_chunk_f64, tested in tests/test_inference.py): [V, C]."""
    from dg_tta_amd.tta import inference as pinf
    cs, cur = pinf._crop_extents(acc, crop)
    vals = [v.reshape(-1, cg).cpu().numpy() for _, cg, v in pinf._resampled_class_groups(acc, nsum, cs, cur, [0, 0, 0])]
    return np.concatenate(vals, axis=1)


@pytest.mark.parametrize("kind", ["logits_fp32", "logits_fp16", "features"])
@pytest.mark.parametrize("M,C,shape", [(2, 150, (3, 9, 19)), (3, 105, (10, 10, 20))])
def test_class_group_path_against_float64(M, C, shape, kind, monkeypatch):
    from dg_tta_amd.tta import inference as pinf
    V = int(np.prod(shape))
    facc, nsum, w, bsum = _inputs(M, C, V, "large", seed=5)
    crop = [slice(0, s) for s in shape]
    nsum_d = torch.from_numpy(nsum).reshape(shape).to(DEV)
    if kind == "features":
        b = np.zeros((M, C), np.float32)
        b[0] = bsum
        acc = pinf.WindowFeatures(torch.from_numpy(facc).reshape(M, *shape, 32).to(DEV), nsum_d, crop, torch.from_numpy(w).to(DEV),
                                  torch.from_numpy(b).to(DEV))
        assert pinf.can_fuse_head_softmax(acc) == (C <= 128)              # C = 150 goes to the class-group loop by itself
        monkeypatch.setattr(pinf, "can_fuse_head_softmax", lambda a: False)
    else:
        l, _ = ref.head_logits(facc, nsum, w, bsum)
        acc = torch.from_numpy((l * M * nsum[:, None]).astype(np.float32)).reshape(*shape, C)      # sum over members x weights
        acc = acc.to(DEV).to(torch.float16 if kind == "logits_fp16" else torch.float32)
    assert pinf.EXPORT_CLASS_GROUP == 8
    st = ref.softmax_stats(_group_values(acc, nsum_d, crop) / M)
    want_seg = pinf.export_segmentation(acc, nsum_d, crop, None, None, None)
    for npt in (np.float32, np.float16):
        sel = _sel(C, 16, 3)
        out = pinf.export_probabilities(acc, nsum_d, crop, None, None, None, M, sel, prob_dtype=npt)
        assert np.array_equal(out["segmentation"], want_seg)
        assert out["probabilities"].dtype == npt and out["probabilities"].shape == (16, *shape)
        assert out["confidence"].dtype == out["entropy"].dtype == np.float32
        pb, hb = ref.f64_path_bounds(st, 0.0, npt)
        pb32, _ = ref.f64_path_bounds(st, 0.0, np.float32)
        r_p = _ratio(np.abs(out["probabilities"].reshape(16, V).astype(np.float64) - st["p"][:, sel].T), pb[:, sel].T)
        r_c = _ratio(np.abs(out["confidence"].reshape(V) - st["confidence"]), pb32[np.arange(V), st["label"]])
        r_h = _ratio(np.abs(out["entropy"].reshape(V) - st["entropy"]), hb)
        print(f"err/bound class groups M={M} C={C} {kind} {npt.__name__}: P {r_p:.3f} conf {r_c:.3f} entropy {r_h:.3f}")
        assert r_p <= 2.0 and r_c <= 2.0 and r_h <= 2.0, (r_p, r_c, r_h)


def test_export_probabilities_takes_the_fused_kernel_when_it_can(monkeypatch):
    """A WindowFeatures the fused kernel supports, no resampling: one fused pass, cropped back from the padding; labels are
    export_segmentation's, values within the fp32 bound of float64."""
    from dg_tta_amd import ops
    from dg_tta_amd.tta import inference as pinf
    M, C, shape = 2, 19, (8, 9, 10)
    V = int(np.prod(shape))
    facc, nsum, w, bsum = _inputs(M, C, V, "spread", seed=9)
    crop = [slice(1, 7), slice(0, 9), slice(2, 10)]
    feats = pinf.WindowFeatures(torch.from_numpy(facc).reshape(M, *shape, 32).to(DEV), torch.from_numpy(nsum).reshape(shape).to(DEV),
                                crop, torch.from_numpy(w).to(DEV), torch.from_numpy(np.stack([bsum, np.zeros_like(bsum)])).to(DEV))
    calls = []
    real = ops.feature_head_softmax
    monkeypatch.setattr(ops, "feature_head_softmax", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    sel = [7, 0, 18]
    out = pinf.export_probabilities(feats, feats.nsum, crop, None, None, None, M, sel, prob_dtype=np.float32)
    assert calls == [1]
    assert np.array_equal(out["segmentation"], pinf.export_segmentation(feats, feats.nsum, crop, None, None, None))
    l, delta = ref.head_logits(facc, nsum, w, bsum)
    st = ref.softmax_stats(l)
    pb, hb = ref.bounds(st, delta)
    inside = np.zeros(shape, bool)
    inside[tuple(crop)] = True
    inside = inside.reshape(V)
    got = out["probabilities"].reshape(3, -1).astype(np.float64)
    assert out["probabilities"].shape == (3, 6, 9, 8)
    assert (np.abs(got - st["p"][inside][:, sel].T) <= 2 * pb[inside][:, sel].T).all()
    assert (np.abs(out["entropy"].reshape(-1) - st["entropy"][inside]) <= 2 * hb[inside]).all()


# ------------------------------------------------------------------------------------------------ resampled geometry
@pytest.mark.parametrize("case", ["linear", "separate_z", "linear_features"])
def test_resampled_export_against_float64(case):
    """A 6 x 10 x 12 crop resampled to 9 x 10 x 17 (linear), and to 10 x 10 x 17 with nearest slices along the strongly anisotropic
    first axis (6 -> 10 has no sample at a rounding tie): logits are resampled FIRST, then the softmax - against the float64 softmax
    of the logits resampled by the CPU routine of tests/test_preprocessing.py.  The logit tolerance is the one that test holds the
    resampling passes to (1e-9 of the largest value)."""
    from dg_tta_amd.tta import inference as pinf
    from oracle import preprocessing as op
    M, C, shape = 2, 19, (6, 10, 12)
    sep = case == "separate_z"
    tgt = (10, 10, 17) if sep else (9, 10, 17)
    spacing = [5.0, 0.9, 0.9] if sep else [1.5, 1.5, 1.5]
    before, bbox = (tgt[0] + 2, tgt[1] + 3, tgt[2] + 2), [[1, tgt[0] + 1], [2, tgt[1] + 2], [0, tgt[2]]]
    props = {"shape_before_cropping": before, "bbox_used_for_cropping": bbox, "shape_after_cropping_and_before_resampling": tgt,
             "spacing": spacing}
    V = int(np.prod(shape))
    facc, nsum, w, bsum = _inputs(M, C, V, "spread", seed=21)
    crop = [slice(0, s) for s in shape]
    nsum_d = torch.from_numpy(nsum).reshape(shape).to(DEV)
    if case == "linear_features":
        acc = pinf.WindowFeatures(torch.from_numpy(facc).reshape(M, *shape, 32).to(DEV), nsum_d, crop, torch.from_numpy(w).to(DEV),
                                  torch.from_numpy(np.stack([bsum, np.zeros_like(bsum)])).to(DEV))
    else:
        l, _ = ref.head_logits(facc, nsum, w, bsum)
        acc = torch.from_numpy((l * M * nsum[:, None]).astype(np.float32)).reshape(*shape, C).to(DEV)
    src = _group_values(acc, nsum_d, crop).reshape(*shape, C).transpose(3, 0, 1, 2)      # [C, x, y, z] float64, sum over members
    conf = PLANS["configurations"]["3d_fullres"]
    do_sep, axis = op.separate_z(list(conf["spacing"]), spacing)
    assert do_sep == sep and (not sep or axis == 0)
    res = op.resample_data_or_seg(src, tgt, False, axis, 1, do_sep, 0)
    assert res.dtype == np.float64 and res.shape == (C, *tgt)
    lr = res.reshape(C, -1).T / M
    st = ref.softmax_stats(lr)
    sel = [18, 4, 0, 9]
    want = ref.paste_full(st["label"].reshape(tgt), st["p"][:, sel].T.reshape(len(sel), *tgt), st["confidence"].reshape(tgt),
                          st["entropy"].reshape(tgt), sel, before, bbox, PLANS["transpose_backward"])
    delta = 1e-9 * np.abs(lr).max()
    pb, hb = ref.f64_path_bounds(st, delta, np.float16)
    pb32, _ = ref.f64_path_bounds(st, delta, np.float32)
    bounds = ref.paste_full(np.zeros(tgt), pb[:, sel].T.reshape(len(sel), *tgt), pb32[np.arange(len(lr)), st["label"]].reshape(tgt),
                            hb.reshape(tgt), [-1] * len(sel), before, bbox, PLANS["transpose_backward"])
    out = pinf.export_probabilities(acc, nsum_d, crop, props, PLANS, "3d_fullres", M, sel)
    assert out["probabilities"].dtype == np.float16 and out["probabilities"].shape == want[1].shape
    assert np.array_equal(out["segmentation"], pinf.export_segmentation(acc, nsum_d, crop, props, PLANS, "3d_fullres"))
    top2 = np.sort(lr, axis=1)[:, -2:]
    safe = ref.paste_full((top2[:, 1] - top2[:, 0] > 4 * delta).reshape(tgt), np.zeros((0, *tgt)), np.zeros(tgt), np.zeros(tgt), [],
                          before, bbox, PLANS["transpose_backward"])[0].astype(bool)      # (outside the top-2 ties of the logit tolerance)
    assert np.array_equal(out["segmentation"][safe], want[0][safe]) and safe.sum() > 0.95 * len(lr)
    inside = np.zeros(before, bool)
    inside[tuple(slice(a, b) for a, b in bbox)] = True
    inside = inside.transpose(PLANS["transpose_backward"])
    # outside the box: background with probability 1, confidence 1, entropy 0, label 0
    k0 = sel.index(0)
    assert (out["probabilities"][k0][~inside] == 1).all() and (np.delete(out["probabilities"], k0, 0)[:, ~inside] == 0).all()
    assert (out["confidence"][~inside] == 1).all() and (out["entropy"][~inside] == 0).all() and (out["segmentation"][~inside] == 0).all()
    # (outside the box the pasted bounds are 0 / 1 and the values are exact)
    r_p = _ratio(np.abs(out["probabilities"].astype(np.float64) - want[1])[:, inside], bounds[1][:, inside])
    r_c = _ratio(np.abs(out["confidence"] - want[2])[inside], bounds[2][inside])
    r_h = _ratio(np.abs(out["entropy"] - want[3])[inside], bounds[3][inside])
    print(f"err/bound resampled {case}: P {r_p:.3f} conf {r_c:.3f} entropy {r_h:.3f}")
    assert r_p <= 2.0 and r_c <= 2.0 and r_h <= 2.0, (r_p, r_c, r_h)


# ------------------------------------------------------------------------------------------------ end to end
def test_export_probabilities_end_to_end_against_the_cpu_ensemble():
    """Two members of the feat32 configuration of test_ensemble_sliding_window_matches_cpu_restatement (fp32 activations) over
    3 x 2 x 3 windows: export_probabilities against the float64 softmax of oracle.inference.ensemble_logits.  That test holds the
    re-formed ensemble logits to 2e-4 of the largest logit; the same figure is the logit error delta of the derived bound here."""
    from test_inference import FEAT32_CFG
    from dg_tta_amd.mind import MIND3D
    from dg_tta_amd.tta import inference as pinf
    from dg_tta_amd.unet import HipPlainConvUNet
    from oracle import inference as oinf, mind as omind, unet as ounet
    torch.manual_seed(0)
    data = torch.randn(1, 28, 20, 30)
    patch = [16, 16, 16]
    members = [ounet.perturb_affine(ounet.init_he(ounet.PlainConvUNetOracle(FEAT32_CFG), s), s + 1) for s in (1, 2)]
    zeros = torch.zeros(1, 12, *patch)
    cpu_models = [lambda x, m=m: m(omind.mind3d(x, zeros, randn_weighting=0.0)) for m in members]
    lref = oinf.ensemble_logits(cpu_models, data, patch)                      # [C, X, Y, Z], mean over members
    net = HipPlainConvUNet(FEAT32_CFG, conv_impl=1).to(DEV)
    net.register_forward_pre_hook(lambda mod, inp: MIND3D(randn_weighting=0.0).forward(*inp))
    acc, nsum, crop = pinf.predict_ensemble(data, net, [m.state_dict() for m in members], patch)
    assert isinstance(acc, pinf.WindowFeatures)
    C = lref.shape[0]
    sel = [C - 1, 2, 0]
    out = pinf.export_probabilities(acc, nsum, crop, None, None, None, len(members), sel, prob_dtype=np.float32)
    assert np.array_equal(out["segmentation"], pinf.export_segmentation(acc, nsum, crop, None, None, None))
    l = lref.double().reshape(C, -1).T.numpy()
    st = ref.softmax_stats(l)
    delta = np.full(len(l), 2e-4 * float(lref.abs().max()))
    pb, hb = ref.bounds(st, delta)
    r_p = _ratio(np.abs(out["probabilities"].reshape(3, -1).astype(np.float64) - st["p"][:, sel].T), pb[:, sel].T)
    r_c = _ratio(np.abs(out["confidence"].reshape(-1) - st["confidence"]), pb[np.arange(len(l)), st["label"]])
    r_h = _ratio(np.abs(out["entropy"].reshape(-1) - st["entropy"]), hb)
    print(f"err/bound end to end: P {r_p:.3f} conf {r_c:.3f} entropy {r_h:.3f}")
    assert r_p <= 2.0 and r_c <= 2.0 and r_h <= 2.0, (r_p, r_c, r_h)
    assert float(out["entropy"].max()) > 0.1                                  # (not a degenerate comparison)


# ------------------------------------------------------------------------------------------------ plan level
def test_run_tta_writes_probabilities_beside_unchanged_labels(tmp_path):
    """tta_main on one synthetic case with `inference_save_probabilities` and `inference_save_uncertainty`: three files in the
    sibling directory; the label file and the summary are those of a run without the keys (same seed, in-kernel MIND noise)."""
    from types import SimpleNamespace as NS

    from conftest import load_golden
    from test_gpu_tta import _network_with_hooks, _plan, _synthetic_case

    from dg_tta_amd.tta import tta as tta_mod
    from dg_tta_amd.tta.config_log_utils import ModifierFunctions
    names = ["background", "a", "b", "c"]
    mapping = {"background": (0, 0), "a": (2, 1), "b": (3, 2), "c": (5, 3)}
    files = {}
    for run, keys in (("with", True), ("without", False)):
        net = _network_with_hooks(load_golden("calc_branch"))
        cfg = _plan(epochs=1, ensemble_count=2, patches_to_be_accumulated=2, tta_data_filepaths=[], seed=3,
                    pretrained_weights_filepath="unused", lr=1e-4, inference_mind_noise="kernel")
        cfg["optimized_labels"] = names
        if keys:
            cfg["inference_save_probabilities"] = True
            cfg["inference_save_uncertainty"] = True
        data = iter([{"data": _synthetic_case(1), "data_properties": {}, "ofile": "tta_outputTs/case1"}]), 1
        bundle = (NS(), [16, 16, 16], net, [{k: v.clone() for k, v in net.state_dict().items()}])
        torch.manual_seed(0)
        np.random.seed(0)
        res = tta_mod.tta_main(run, cfg, tmp_path, tmp_path, mapping, NS(ModifierFunctions=ModifierFunctions), DEV,
                               network_bundle=bundle, tta_data=data)
        files[run] = Path(res[("tta_outputTs/case1", "prediction")])
    soft_dir = tmp_path / "with" / "tta_outputTs_probabilities"
    assert sorted(p.name for p in soft_dir.iterdir()) == ["case1.npz", "case1_confidence.npy", "case1_entropy.npy"]
    assert not (tmp_path / "without" / "tta_outputTs_probabilities").exists()
    assert sorted(p.name for p in files["with"].parent.iterdir()) == sorted(p.name for p in files["without"].parent.iterdir())
    assert files["with"].read_bytes() == files["without"].read_bytes()
    summaries = [(tmp_path / run / "summary_Ts.json").read_text().replace(str(tmp_path / run), "<run>") for run in ("with", "without")]
    assert json.loads(summaries[0]) == json.loads(summaries[1]) and "<run>" in summaries[0]      # (equal but for the run directory)
    label = np.load(files["with"])
    npz = np.load(soft_dir / "case1.npz")
    probs, conf, ent = npz["probabilities"], np.load(soft_dir / "case1_confidence.npy"), np.load(soft_dir / "case1_entropy.npy")
    assert probs.dtype == np.float16 and probs.shape == (4, *label.shape) and list(npz["class_names"]) == names
    assert conf.dtype == ent.dtype == np.float32 and conf.shape == ent.shape == label.shape
    assert float(probs.astype(np.float32).sum(0).max()) <= 1 + 1e-3
    from dg_tta_amd.tta.inference import _num_classes
    C = int(_num_classes(net))
    assert (conf > 0).all() and (conf <= 1).all() and (ent >= 0).all() and float(ent.max()) <= np.log(C) + 1e-6
