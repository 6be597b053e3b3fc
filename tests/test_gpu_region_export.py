"""GPU: the region end of the class-group export loop - dgtta_regions_merge_f64 (csrc/resample.hip), inference._RunningRegions,
export_segmentation(..., regions_class_order=...) with a case's geometry and export_region_probabilities - against the float64
restatement tests/region_export_ref.py, which tests/test_region_export_ref.py licenses against a voxel loop of nnU-Net's rule.

Labels are compared as integers.  A stored probability may differ from the float64 value by one unit in the last place of its type
(region_export_ref.prob_bound: the double evaluation errs by a few 1e-16, the final rounding by half a unit) - derived, not measured;
resampled exports add delta / 4, delta = 1e-9 of the largest logit being what tests/test_preprocessing.py holds the resampling
passes to and 1 / 4 the largest slope of the sigmoid."""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import region_export_ref as xref      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]
PLANS = dict(json.loads((ROOT / "dg_tta_amd" / "__resources__" / "model_skeleton" / "plans.json").read_text()),
             transpose_forward=[2, 0, 1], transpose_backward=[1, 2, 0])      # (the skeleton's own is the identity)
BADARG, UNSUPPORTED = -1, -2
SPECIALS = [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 745.0, -745.0, np.inf, -np.inf, np.nan]
V_KERNEL = 1237            # neither a multiple of 64 nor of 256: five workgroups, the last one ragged
GUARD = 64
LABEL_FILL = 0x7fffffff


def _order(R, seed):
    """R distinct positive labels up to 1000, not sorted."""
    order = (np.random.default_rng(seed).permutation(1000)[:R] + 1).tolist()
    if R > 2 and order == sorted(order):
        order[0], order[-1] = order[-1], order[0]
    return order


def _kernel_values(R, V):
    rng = np.random.default_rng(17 + R)
    vals = rng.standard_normal((V, R)) * 2.0
    for j in range(R):                      # every special value in every output, at voxels that move with the output
        for k, s in enumerate(SPECIALS):
            vals[(37 * j + 101 * k + 5) % V, j] = s
    return vals


def _guarded(n, dtype, fill):
    """(whole buffer, the n elements between two guard runs); the guards hold 77, the inside `fill`."""
    buf = torch.full((n + 2 * GUARD,), 77, dtype=dtype, device=DEV)
    buf[GUARD:GUARD + n] = fill
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    return bool((buf[:GUARD] == 77).all()) and bool((buf[GUARD + n:] == 77).all())


def _merge_all(lib, vals_d, V, R, order, scale, label, probs, code, group):
    h_order = (ctypes.c_int * R)(*order)
    for c0 in range(0, R, group):
        cg = min(group, R - c0)
        chunk = vals_d[:, c0:c0 + cg].contiguous()
        rc = lib.dgtta_regions_merge_f64(chunk.data_ptr(), V, cg, c0, scale, h_order, R, label.data_ptr(),
                                         None if probs is None else probs.data_ptr(), code, int(c0 == 0), None)
        assert rc == 0, lib.dgtta_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("R", [1, 3, 8, 9, 19, 32])
def test_regions_merge_kernel_against_the_restatement(R):
    """Merged in groups of EXPORT_CLASS_GROUP = 8 (the last groups of R = 9 and R = 19 hold 1 and 3 outputs), fp32 and fp16 planes,
    one and two members; the label buffer starts from 0x7fffffff (first != 0 must reset it) and every output lies between guard
    words."""
    from dg_tta_amd import _lib, ops
    from dg_tta_amd.tta.inference import EXPORT_CLASS_GROUP
    assert EXPORT_CLASS_GROUP == 8
    lib = _lib.load()
    V = V_KERNEL
    order = _order(R, R)
    assert len(set(order)) == R and min(order) > 0 and max(order) <= 1000 and (R < 3 or order != sorted(order))
    vals = _kernel_values(R, V)
    vals_d = torch.from_numpy(vals).to(DEV)
    for scale in (1.0, 0.5):
        want_label, want_p = xref.region_export(vals, order, scale, group=EXPORT_CLASS_GROUP)
        assert np.isnan(want_p).sum() == R and (want_label[np.isnan(vals).any(axis=1)] >= 0).all()
        lbuf0, label0 = _guarded(V, torch.int32, LABEL_FILL)
        _merge_all(lib, vals_d, V, R, order, scale, label0, None, 0, EXPORT_CLASS_GROUP)          # probs_out = NULL
        assert _guards_intact(lbuf0, V) and np.array_equal(label0.cpu().numpy(), want_label)
        for tdt, npt, code in ((torch.float32, np.float32, ops.F32), (torch.float16, np.float16, ops.F16)):
            lbuf, label = _guarded(V, torch.int32, LABEL_FILL)
            pbuf, probs = _guarded(R * V, tdt, -7.0)
            _merge_all(lib, vals_d, V, R, order, scale, label, probs, code, EXPORT_CLASS_GROUP)
            assert _guards_intact(lbuf, V) and _guards_intact(pbuf, R * V)
            assert np.array_equal(label.cpu().numpy(), want_label)                                 # bit-equal, NaN not positive
            got = probs.reshape(R, V).cpu().numpy().astype(np.float64)
            nan = np.isnan(want_p)
            assert np.array_equal(np.isnan(got), nan)                                              # sigmoid(NaN) is NaN, nothing else is
            err, bound = np.abs(got - want_p)[~nan], xref.prob_bound(want_p, npt)[~nan]
            print(f"regions_merge R={R} scale={scale} {npt.__name__}: max err / bound {float((err / bound).max()):.3f}")
            assert (err <= bound).all()
            assert (got[~nan] >= 0).all() and (got[~nan] <= 1).all()


def test_regions_merge_argument_checks_leave_the_outputs_untouched():
    from dg_tta_amd import _lib, ops
    lib = _lib.load()
    V, R, cg = 300, 5, 3
    vals = torch.randn(V, cg, dtype=torch.float64, device=DEV).abs() + 1.0      # all positive: any launch would change the label
    lbuf, label = _guarded(V, torch.int32, LABEL_FILL)
    pbuf, probs = _guarded(R * V, torch.float32, -7.0)
    good = dict(vals=vals.data_ptr(), V=V, cg=cg, c0=1, scale=0.5, order=[4, 9, 2, 7, 1], R=R, label=label.data_ptr(),
                probs=probs.data_ptr(), code=ops.F32, first=1)

    def call(**kw):
        a = dict(good, **kw)
        h = None if a["order"] is None else (ctypes.c_int * max(len(a["order"]), 1))(*a["order"])
        return lib.dgtta_regions_merge_f64(a["vals"], a["V"], a["cg"], a["c0"], a["scale"], h, a["R"], a["label"], a["probs"], a["code"],
                                           a["first"], None)

    bad = [dict(vals=None), dict(order=None), dict(label=None), dict(R=0, order=[]), dict(R=-1), dict(R=33, order=list(range(1, 34))),
           dict(c0=-1), dict(c0=3), dict(c0=5, cg=1), dict(cg=0), dict(cg=6, c0=0), dict(V=0), dict(V=-5),
           dict(order=[4, 9, 0, 7, 1]), dict(order=[4, 9, 2, 7, -1]), dict(order=[0, 9, 2, 7, 1], c0=1),      # (a label outside the group too)
           dict(code=ops.BF16), dict(code=7), dict(code=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan"))]
    for kw in bad:
        assert call(**kw) == BADARG, kw
        assert lib.dgtta_last_error().startswith(b"regions_merge"), kw
    assert call(V=(1 << 31) * 256) == UNSUPPORTED and b"too many voxels" in lib.dgtta_last_error()
    assert call(V=(1 << 31) * 256, probs=None) == UNSUPPORTED
    assert call(code=7, probs=None, V=(1 << 31) * 256) == UNSUPPORTED      # (the type is not read without planes)
    torch.cuda.synchronize()
    assert bool((label == LABEL_FILL).all()) and bool((probs == -7.0).all()) and _guards_intact(lbuf, V) and _guards_intact(pbuf, R * V)
    assert call() == 0                       # ... and the good call is a good call: planes 1..3 written, 0 and 4 left alone
    torch.cuda.synchronize()
    assert bool((label == 7).all())          # every value positive: the last output of the group, order[3], wins
    p = probs.reshape(R, V)
    assert bool((p[0] == -7.0).all()) and bool((p[4] == -7.0).all()) and bool(((p[1:4] > 0.5) & (p[1:4] < 1)).all())
    assert _guards_intact(lbuf, V) and _guards_intact(pbuf, R * V)


# ------------------------------------------------------------------------------------------------ accumulators
def _accumulator(kind, M, R, shape, seed, zeros=0):
    """(acc, nsum on the GPU): a logits accumulator (fp32 / fp16) or a WindowFeatures of M members with R outputs over `shape`;
    nsum spread over [1e-2, 40]; logits of unit scale.  zeros: that many accumulated logits set to exactly 0 (logits kinds)."""
    from dg_tta_amd.tta import inference as pinf
    rng = np.random.default_rng(seed)
    V = int(np.prod(shape))
    nsum = np.exp(rng.uniform(np.log(1e-2), np.log(40.0), V)).astype(np.float32)
    nsum_d = torch.from_numpy(nsum).reshape(shape).to(DEV)
    crop = [slice(0, s) for s in shape]
    if kind == "features":
        facc = (rng.standard_normal((M, V, 32)).astype(np.float32) * nsum[None, :, None]).astype(np.float32)
        w = (rng.standard_normal((M, R, 32)) * 0.2).astype(np.float32)
        b = (rng.standard_normal((M, R)) * 0.3).astype(np.float32)
        acc = pinf.WindowFeatures(torch.from_numpy(facc).reshape(M, *shape, 32).to(DEV), nsum_d, crop, torch.from_numpy(w).to(DEV),
                                  torch.from_numpy(b).to(DEV))
    else:
        l = rng.standard_normal((V, R)) * 1.5
        a = (l * M * nsum[:, None]).astype(np.float32)
        if zeros:
            a.reshape(-1)[rng.permutation(a.size)[:zeros]] = 0.0
        acc = torch.from_numpy(a).reshape(*shape, R).to(DEV).to(torch.float16 if kind == "logits_fp16" else torch.float32)
    return acc, nsum_d


def _group_values(acc, nsum, crop):
    """The float64 chunk values the export loop itself forms (dgtta_*_chunk_f64, tested in tests/test_inference.py): [V, R], the sum
    over members of the window-normalised logits."""
    from dg_tta_amd.tta import inference as pinf
    cs, cur = pinf._crop_extents(acc, crop)
    return np.concatenate([v.reshape(-1, cg).cpu().numpy() for _, cg, v in pinf._resampled_class_groups(acc, nsum, cs, cur, [0, 0, 0])],
                          axis=1)


ORDERS = {3: [1, 3, 2], 19: [11, 300, 7, 2, 19, 5, 3, 254, 255, 13, 17, 1, 23, 29, 31, 37, 41, 43, 47]}


@pytest.mark.parametrize("kind", ["logits_fp32", "logits_fp16", "features"])
@pytest.mark.parametrize("case", ["linear", "separate_z"])
@pytest.mark.parametrize("R", [3, 19])
def test_resampled_region_export_against_float64(R, case, kind):
    """The geometry of test_resampled_export_against_float64: a 6 x 10 x 12 crop resampled to 9 x 10 x 17 (linear) and to
    10 x 10 x 17 with nearest slices along the strongly anisotropic first axis, pasted into a larger box, transposed back.  Two
    members.  Reference: oracle.preprocessing.resample_data_or_seg on the float64 group values, then the restatement.  Labels are
    equal wherever every |l_i| > 4 delta (at least 99 % of the voxels: for continuous logits of unit scale the excluded share is of
    order 1e-8); probabilities within one fp16 unit + delta / 4; outside the box label 0 and probability 0 exactly."""
    from dg_tta_amd import ops
    from dg_tta_amd.tta import inference as pinf
    from oracle import preprocessing as op
    M, shape, order = 2, (6, 10, 12), ORDERS[R]
    assert ops.feature_head_regions_supported(M, R)      # (R allows a WindowFeatures accumulator in both cases)
    sep = case == "separate_z"
    tgt = (10, 10, 17) if sep else (9, 10, 17)
    spacing = [5.0, 0.9, 0.9] if sep else [1.5, 1.5, 1.5]
    before, bbox = (tgt[0] + 2, tgt[1] + 3, tgt[2] + 2), [[1, tgt[0] + 1], [2, tgt[1] + 2], [0, tgt[2]]]
    props = {"shape_before_cropping": before, "bbox_used_for_cropping": bbox, "shape_after_cropping_and_before_resampling": tgt,
             "spacing": spacing}
    tb = PLANS["transpose_backward"]
    assert list(tb) != [0, 1, 2]
    acc, nsum = _accumulator(kind, M, R, shape, seed=31 + R)
    crop = [slice(0, s) for s in shape]
    src = _group_values(acc, nsum, crop).reshape(*shape, R).transpose(3, 0, 1, 2)      # [R, x, y, z] float64, sum over members
    do_sep, axis = op.separate_z(list(PLANS["configurations"]["3d_fullres"]["spacing"]), spacing)
    assert do_sep == sep and (not sep or axis == 0)
    res = op.resample_data_or_seg(src, tgt, False, axis, 1, do_sep, 0)
    assert res.dtype == np.float64 and res.shape == (R, *tgt)
    vals = res.reshape(R, -1).T
    lab, p = xref.region_export(vals, order, 1.0 / M, group=pinf.EXPORT_CLASS_GROUP)
    want_seg, want_p = xref.paste_full(lab.reshape(tgt), p.reshape(R, *tgt), before, bbox, tb)
    l = vals / M
    delta = 1e-9 * np.abs(l).max()
    safe = xref.paste_full((np.abs(l) > 4 * delta).all(axis=1).reshape(tgt), np.zeros((0, *tgt)), before, bbox, tb)[0].astype(bool)
    assert safe.sum() >= 0.99 * len(l)
    inside = np.zeros(before, bool)
    inside[tuple(slice(a, b) for a, b in bbox)] = True
    inside = inside.transpose(tb)

    seg = pinf.export_segmentation(acc, nsum, crop, props, PLANS, "3d_fullres", regions_class_order=order)
    assert seg.dtype == (np.uint16 if R == 19 else np.uint8) and seg.shape == want_seg.shape
    assert np.array_equal(seg[safe], want_seg[safe]) and (seg[~inside] == 0).all()
    assert set(np.unique(seg).tolist()) <= {0, *order} and len(np.unique(seg)) > 2
    out = pinf.export_region_probabilities(acc, nsum, crop, props, PLANS, "3d_fullres", M, order)
    assert sorted(out) == ["probabilities", "segmentation"]
    assert out["segmentation"].dtype == seg.dtype and np.array_equal(out["segmentation"], seg)      # array for array
    probs = out["probabilities"]
    assert probs.dtype == np.float16 and probs.shape == want_p.shape == (R, *seg.shape)
    assert (probs[:, ~inside] == 0).all()
    err = np.abs(probs.astype(np.float64) - want_p)[:, inside]
    bound = xref.prob_bound(want_p, np.float16)[:, inside] + delta / 4
    print(f"resampled region export R={R} {case} {kind}: max err / bound {float((err / bound).max()):.3f}, "
          f"excluded {1 - safe.sum() / len(l):.2e}")
    assert (err <= bound).all()
    p32 = pinf.export_region_probabilities(acc, nsum, crop, props, PLANS, "3d_fullres", M, order, prob_dtype=np.float32)
    assert p32["probabilities"].dtype == np.float32 and np.array_equal(p32["segmentation"], seg)
    err32 = np.abs(p32["probabilities"].astype(np.float64) - want_p)[:, inside]
    assert (err32 <= xref.prob_bound(want_p, np.float32)[:, inside] + delta / 4).all()
    with pytest.raises(ValueError, match="members"):
        pinf.export_region_probabilities(acc, nsum, crop, props, PLANS, "3d_fullres", 0, order)
    if kind == "features":
        with pytest.raises(ValueError, match="members"):
            pinf.export_region_probabilities(acc, nsum, crop, props, PLANS, "3d_fullres", 3, order)


@pytest.mark.parametrize("kind", ["logits_fp32", "logits_fp16", "features"])
def test_unresampled_export_with_properties_is_the_label_map_kernels_own(kind):
    """Properties whose target shape is the current one: the pasted map equals the pasted _label_map_fn map in every voxel, with
    and without probabilities - also where an accumulated logit is exactly 0 (dividing a non-zero fp32 sum by a positive weight in
    double cannot change its sign; 0 stays 0)."""
    from dg_tta_amd.tta import inference as pinf
    M, R, shape, order = 2, 19, (8, 9, 10), ORDERS[19]
    acc, nsum = _accumulator(kind, M, R, shape, seed=77, zeros=200)
    crop = [slice(1, 7), slice(0, 9), slice(2, 10)]
    tgt = (6, 9, 8)
    before, bbox = (9, 9, 11), [[2, 8], [0, 9], [1, 9]]
    props = {"shape_before_cropping": before, "bbox_used_for_cropping": bbox, "shape_after_cropping_and_before_resampling": tgt,
             "spacing": [1.5, 1.5, 1.5]}
    tb = PLANS["transpose_backward"]
    own = pinf._label_map_fn(acc, order)()[tuple(crop)].cpu().numpy()
    want, _ = xref.paste_full(own, np.zeros((0, *tgt)), before, bbox, tb)
    seg = pinf.export_segmentation(acc, nsum, crop, props, PLANS, "3d_fullres", regions_class_order=order)
    assert seg.dtype == np.uint16 and np.array_equal(seg, want) and len(np.unique(seg)) > 2
    out = pinf.export_region_probabilities(acc, nsum, crop, props, PLANS, "3d_fullres", M, order)
    assert np.array_equal(out["segmentation"], want) and out["segmentation"].dtype == np.uint16
    # the probabilities of the same export, against the restatement on the loop's own group values (nothing is resampled: delta = 0)
    vals = _group_values(acc, nsum, crop)
    lab, p = xref.region_export(vals, order, 1.0 / M)
    if kind == "features":      # the head is evaluated in fp32 there and in double here: the sign is shared away from rounding level
        clear = (np.abs(vals) > 1e-4 * np.abs(vals).max()).all(axis=1).reshape(tgt)
        assert clear.mean() > 0.99 and np.array_equal(lab.reshape(tgt)[clear], own[clear])
    else:                       # ... and the float64 route agrees with the fp32 kernel: the sign of a sum is the sign of its quotient
        assert np.array_equal(lab.reshape(tgt), own)
    _, want_p = xref.paste_full(lab.reshape(tgt), p.reshape(R, *tgt), before, bbox, tb)
    err = np.abs(out["probabilities"].astype(np.float64) - want_p)
    assert (err <= xref.prob_bound(want_p, np.float16)).all()
    # the preprocessed geometry: no paste, no transpose
    flat = pinf.export_region_probabilities(acc, nsum, crop, None, None, None, M, order, prob_dtype=np.float32)
    assert np.array_equal(flat["segmentation"], own) and flat["probabilities"].shape == (R, *tgt)
    assert np.array_equal(flat["segmentation"], pinf.export_segmentation(acc, nsum, crop, None, None, None, order))
    assert (np.abs(flat["probabilities"].astype(np.float64) - p.reshape(R, *tgt)) <= xref.prob_bound(p, np.float32).reshape(R, *tgt)).all()
