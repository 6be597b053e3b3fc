"""GPU: the hole-filling kernels of csrc/components.hip (dgtta_holes_fill, dgtta_holes_member, dgtta_holes_apply,
dgtta_nonzero_mask), the post-processing built on them (fill_label_holes, the hook of run_tta) and the non-zero crop of the
preprocessing (crop_to_nonzero_gpu), against the numpy reference tests/holes_ref.py, which tests/test_holes_ref.py licenses
against scipy.ndimage.binary_fill_holes.  This file imports no scipy; the crop is compared with the host crop_to_nonzero.

Everything is boolean or integer valued, so every comparison is exact equality on every voxel; there is no tolerance and nothing
is left out.  Shapes: the complement is labelled by the tile kernels of the component filter (8 x 8 x 64), so the shapes are
components_ref.SHAPES; the boxes, shells and label maps are laid across tile borders."""
import numpy as np
import pytest
import torch

import holes_ref as HR

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)        # a copy: the shared inputs are read-only


def _check(name, mask, connectivity):
    from dg_tta_amd import ops
    m = _dev(mask)
    filled, n = ops.fill_holes(m, connectivity)
    filled2, n2, box = ops.fill_holes(m, connectivity, return_box=True)
    want, want_n = HR.reference(name, connectivity)
    where = f"{name} c{connectivity}"
    assert filled.dtype == torch.uint8 and filled.shape == mask.shape and n.dtype == torch.int64 and n.shape == ()
    assert torch.equal(filled, filled2) and int(n) == int(n2), f"{where}: two runs differ"
    bad = np.flatnonzero(filled.cpu().numpy().reshape(-1) != want.reshape(-1))
    assert bad.size == 0, f"{where}: filled differs at {bad.size} voxels, first {bad[:5]}"
    assert int(n) == want_n, where
    idx = np.nonzero(want)
    want_box = [int(i.min()) for i in idx] + [int(i.max()) for i in idx] if want.any() else None
    box = box.cpu().tolist()
    assert (box == want_box) if want_box else all(box[k] > box[3 + k] for k in range(3)), f"{where}: box {box} vs {want_box}"
    assert torch.equal(m, _dev(mask))                   # the input is left alone
    return int(n)


@pytest.mark.parametrize("connectivity", HR.CONNECTIVITIES)
@pytest.mark.parametrize("shape", HR.SHAPES, ids=str)
def test_fill_holes_vs_reference(shape, connectivity):
    """All False, all True, noise, the shell, and the serpentine cavity closed and ending on a face, wherever the shape holds them."""
    for kind in HR.GENERIC_KINDS:
        mask = HR.volume(kind, shape)
        if mask is not None:
            n = _check(HR.generic_name(kind, shape), mask, connectivity)
            if kind in ("empty", "full", "serpentine_open") or min(shape) < 3:
                assert n == 0
            if kind == "serpentine":
                assert n == int((mask == 0).sum())


@pytest.mark.parametrize("connectivity", HR.CONNECTIVITIES)
def test_boxes_tunnels_cup_and_shells(connectivity):
    """The hollow box closed and with a face, an edge-only and a corner-only tunnel, each also at the corner of four tiles; the cup
    open towards a face; the shell inside a shell.  Known counts for all of them."""
    k = HR.CONNECTIVITIES.index(connectivity)
    for name, mask in HR.special_inputs():
        n = _check(name, mask, connectivity)
        if name.startswith("box"):
            assert n == HR.BOX_COUNTS[name.split()[1]][k], name
    from dg_tta_amd import ops
    assert int(ops.fill_holes(_dev(HR.cup()), connectivity)[1]) == 0
    assert int(ops.fill_holes(_dev(HR.shells()), connectivity)[1]) == HR.SHELLS_COUNT


@pytest.mark.parametrize("connectivity", HR.CONNECTIVITIES)
@pytest.mark.parametrize("kind", HR.NOISE_KINDS)
def test_noise_around_the_percolation_threshold_of_the_complement(kind, connectivity):
    _check(HR.generic_name(kind, HR.NOISE_SHAPE), HR.volume(kind, HR.NOISE_SHAPE), connectivity)


def test_caller_buffers_and_bad_arguments():
    from dg_tta_amd import _lib, ops
    name, mask = "shells", HR.shells()
    m, n = _dev(mask), mask.size
    assert ops.holes_ws_bytes(*mask.shape) >= 5 * n and ops.holes_ws_bytes(0, 1, 1) == 0
    out_buf = torch.full((n + 100,), 7, dtype=torch.uint8, device=DEV)
    ws = torch.empty(ops.holes_ws_bytes(*mask.shape) + 64, dtype=torch.uint8, device=DEV)
    filled, cnt = ops.fill_holes(m, 18, out=out_buf, ws=ws)
    assert filled.data_ptr() == out_buf.data_ptr() and (out_buf[n:] == 7).all()
    assert np.array_equal(filled.cpu().numpy(), HR.reference(name, 18)[0]) and int(cnt) == HR.SHELLS_COUNT
    for c in (0, 4, 8, 27, True, "6", None):
        with pytest.raises(ValueError, match="connectivity"):
            ops.fill_holes(m, c)
    for bad in (m.bool(), m.long(), m.float(), m[0], m[None], m.permute(2, 1, 0)):
        with pytest.raises(ValueError, match="uint8 mask"):
            ops.fill_holes(bad)
    with pytest.raises(_lib.DgttaError):
        ops.fill_holes(m.cpu())
    for bad in (out_buf.int(), out_buf[:n - 1], out_buf.cpu()):
        with pytest.raises(ValueError, match="fill_holes: out"):
            ops.fill_holes(m, out=bad)
    for bad in (ws[:16], ws.cpu(), ws.view(torch.int32)):
        with pytest.raises(ValueError, match="fill_holes: ws"):
            ops.fill_holes(m, ws=bad)
    # 2^31 - 1 voxels and more are refused before anything is launched or read
    lib = _lib.load()
    assert lib.dgtta_holes_fill(m.data_ptr(), 2048, 1024, 1024, 6, filled.data_ptr(), cnt.data_ptr(), None, ws.data_ptr(), 2 ** 42, None) == -2
    assert b"2^31" in lib.dgtta_last_error()
    torch.cuda.synchronize()


def test_nonzero_mask_has_ieee_semantics():
    from dg_tta_amd import ops
    rng = np.random.default_rng(5)
    for shape in ((2, 6, 10, 12), (1, 3, 5, 7), (3, 1, 1, 1), (2, 4, 4, 5)):       # n a multiple of four and not
        data = rng.normal(0, 1, shape).astype(np.float32) * (rng.random(shape) < 0.3)
        flat = data.reshape(-1)
        flat[0::7], flat[1::11], flat[2::13] = np.nan, -0.0, np.float32(1e-45)   # NaN counts, -0.0 does not, a denormal does
        want = (data != 0).any(0)
        got = ops.nonzero_mask(_dev(data))
        assert got.dtype == torch.uint8 and got.shape == shape[1:] and np.array_equal(got.cpu().numpy(), want.astype(np.uint8))
        off = torch.zeros(data.size + 1, dtype=torch.float32, device=DEV)        # a pointer that is not 16-byte aligned
        off[1:] = _dev(data).reshape(-1)
        assert np.array_equal(ops.nonzero_mask(off[1:].view(shape)).cpu().numpy(), want.astype(np.uint8))
    for bad in (torch.zeros(2, 3, 4, 5, dtype=torch.float64, device=DEV), torch.zeros(5, device=DEV), torch.zeros(2, 3, 4, device=DEV)[:, ::2]):
        with pytest.raises(ValueError, match="float32 data"):
            ops.nonzero_mask(bad)


# ---------------------------------------------------------------------------------------------- labels
def _check_labels(seg, entries, connectivity=6, background=0):
    from dg_tta_amd.tta.postprocessing import fill_label_holes
    got, counts = fill_label_holes(seg.copy(), entries, connectivity=connectivity, background=background)    # (the shared one is read-only)
    want, want_counts = HR.fill_label_holes(seg, entries, connectivity, background)         # the whole-volume reference
    assert isinstance(got, np.ndarray) and got.dtype == seg.dtype and np.array_equal(got, want), entries
    assert counts == want_counts, entries
    return got, counts


@pytest.mark.parametrize("connectivity", HR.CONNECTIVITIES)
def test_fill_label_holes_vs_reference(connectivity):
    """The pocket is filled and the lesion kept; regions; the order of nested shells; labels of 1024 and more are no wall; noise.
    The product fills inside the bounding box of each entry, the reference in the whole volume."""
    organ, nested, wall = HR.organ_with_lesion(), HR.nested_label_shells(), HR.high_label_wall()
    for seg, entries in ((organ, None), (organ, [1, 2, 3, 4]), (organ, [(3, 2), 4]), (organ, [4, (2, 3)]), (organ, [7]), (nested, [1, 2]),
                         (nested, [2, 1]), (nested, [(2, 1)]), (nested, None), (wall, None), (wall, [2]), (wall, [(3, 2)]),
                         (HR.volume("noise0.69", HR.NOISE_SHAPE).astype(np.int64) * 3, [3])):
        _check_labels(seg, entries, connectivity)
    _check_labels(organ, [2], connectivity, background=3)


def test_fill_label_holes_known_results_and_containers():
    from dg_tta_amd.tta.postprocessing import fill_label_holes
    organ, nested = HR.organ_with_lesion(), HR.nested_label_shells()
    got, counts = _check_labels(organ, None)
    assert counts == {1: 0, 2: 96, 3: 0, 4: 8}
    assert (got[organ == 3] == 3).all() and (got[6:9, 6:10, 60:68] == 2).all() and (got[4:6, 4:6, 74:76] == 4).all()
    assert _check_labels(organ, [(3, 2)])[1] == {(3, 2): 96} and _check_labels(organ, [(3, 2)])[0][7, 7, 62] == 3
    assert _check_labels(nested, [1, 2])[0][6, 7, 37] == 1 and _check_labels(nested, [2, 1])[0][6, 7, 37] == 2
    assert _check_labels(HR.high_label_wall(), None)[1] == {1: 0, 2: 0, 3: 0}
    want = HR.fill_label_holes(organ, [2, 4], 6)[0]
    got, counts = fill_label_holes(organ.astype(np.int16), [2, 4])
    assert isinstance(got, np.ndarray) and got.dtype == np.int16 and np.array_equal(got, want) and counts == {2: 96, 4: 8}
    got, _ = fill_label_holes(torch.from_numpy(organ.copy()), [2, 4])
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and got.device.type == "cpu" and np.array_equal(got.numpy(), want)
    on_dev = _dev(organ)
    got, _ = fill_label_holes(on_dev, [2, 4])
    assert got.is_cuda and got.data_ptr() != on_dev.data_ptr() and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(on_dev, _dev(organ))             # an int64 map on the device is not filled in place
    got, _ = fill_label_holes(_dev(organ).to(torch.int32), [2, 4], connectivity=26)
    assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), HR.fill_label_holes(organ, [2, 4], 26)[0])
    got, counts = fill_label_holes(np.zeros((2, 3, 4), dtype=np.uint8))
    assert not got.any() and counts == {}
    with pytest.raises(ValueError, match="call twice"):
        fill_label_holes(organ.copy(), [2, (2, 3)])
    with pytest.raises(ValueError, match="connectivity"):
        fill_label_holes(organ.copy(), [2], connectivity=8)
    with pytest.raises(ValueError, match="integer label map"):
        fill_label_holes(organ.astype(np.float32))
    with pytest.raises(ValueError, match="foreground"):
        fill_label_holes(organ.copy(), "foreground")
    with pytest.raises(ValueError, match="1024"):
        fill_label_holes(organ.copy(), [1024])


def test_postprocess_prediction_follows_the_plan_keys(capsys):
    from dg_tta_amd.tta.tta import _postprocess_prediction
    organ = HR.organ_with_lesion()
    stray = organ.copy()
    assert not stray[0:2, 12:14, 50:54].any()
    stray[0, 13, 51:53] = 2             # an island of the organ for the component filter, which runs first
    seg = torch.from_numpy(stray)
    names = ["background", "blob", "organ", "lesion", "other"]
    assert _postprocess_prediction(seg, {"optimized_labels": names}, DEV) is seg
    assert _postprocess_prediction(seg, {"optimized_labels": names, "postprocessing_fill_holes": False,
                                         "postprocessing_fill_holes_connectivity": 26}, DEV) is seg
    got = _postprocess_prediction(seg, {"optimized_labels": names, "postprocessing_fill_holes": True}, DEV)
    assert got is not seg and got.dtype == seg.dtype and got.device == seg.device
    assert np.array_equal(got.numpy(), HR.fill_label_holes(stray, [1, 2, 3, 4], 6)[0])
    assert "filled voxels: blob=0, organ=96, lesion=0, other=8" in capsys.readouterr().out
    got = _postprocess_prediction(seg, {"optimized_labels": names, "postprocessing_fill_holes": [["lesion", "organ"]],
                                        "postprocessing_fill_holes_connectivity": 26,
                                        "postprocessing_keep_largest_component": ["organ"]}, DEV)
    assert np.array_equal(got.numpy(), HR.fill_label_holes(organ, [(3, 2)], 26)[0])         # the island is gone, then the pocket
    out = capsys.readouterr().out
    assert "removed voxels: organ=2" in out and "filled voxels: lesion+organ=96" in out
    assert torch.equal(seg, torch.from_numpy(stray))


# ---------------------------------------------------------------------------------------------- the non-zero crop
def _body(seed=0, shape=(22, 26, 30), channels=1):
    """test_preprocessing._case-style: a body of noise with interior zeros (a block and scattered voxels) in a zero volume."""
    rng = np.random.default_rng(seed)
    img = np.zeros((channels, *shape), np.float32)
    inner = (slice(3, shape[0] - 3), slice(4, shape[1] - 4), slice(5, shape[2] - 3))
    extent = tuple(s.stop - s.start for s in inner)
    img[(slice(None), *inner)] = rng.normal(-100, 400, (channels, *extent)) * (rng.random(extent) < 0.7)
    c = [(s.start + s.stop) // 2 for s in inner]
    img[:, c[0] - 1:c[0] + 1, c[1] - 2:c[1] + 2, c[2] - 2:c[2] + 2] = 0.0
    seg = np.zeros((1, *shape), np.int8)
    seg[:, 2:c[0] + 1, 6:13, 8:15] = 2
    seg[:, c[0]:, 12:19, 14:21] = 5
    return img, seg


def _check_crop(img, seg, **kw):
    from dg_tta_amd.tta import preprocessing as pp
    want = pp.crop_to_nonzero(img.copy(), None if seg is None else seg.copy(), **kw)
    got = pp.crop_to_nonzero_gpu(img.copy(), None if seg is None else seg.copy(), DEV, **kw)
    for g, w in zip(got[:2], want[:2]):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=g.dtype.kind == "f")
    assert got[2] == want[2] and all(type(v) is int for ab in got[2] for v in ab)
    return got


def test_crop_to_nonzero_gpu_equals_the_host_crop():
    img, seg = _body()
    _check_crop(img, seg)
    d, s, _ = _check_crop(img, None)
    assert ((s[0] == 0) & (d[0] == 0)).any() and ((s[0] == -1) & (d[0] == 0)).any()      # zeros inside the body and on its surface
    _check_crop(img, seg.astype(np.int16), nonzero_label=-7)
    img2, seg2 = _body(1, (9, 70, 33), channels=2)                      # C = 2: zero in one channel, not in the other
    img2[1, 4, 30:40, 10] = 0.0
    img2[:, 5, 30:40, 11] = 0.0
    _check_crop(img2, seg2)
    _check_crop(img2, None)
    odd = img.copy()                                                    # NaN counts as non-zero, -0.0 as zero
    odd[0, 0, 0, 0] = np.nan
    odd[0, 21, 25, 29] = -0.0
    odd[0, 10, 12, 14] = np.nan
    odd[0, 3:19, 4:22, 5] = -0.0
    _, _, bbox = _check_crop(odd, seg)
    assert bbox[0] == [0, 19] and bbox[2][0] == 0
    face = np.zeros((1, 12, 13, 66), np.float32)                        # a body that touches three faces, its cavity is closed
    face[0, 0:8, 5:13, 0:40] = 1.0
    face[0, 2:5, 7:10, 10:30] = 0.0
    d, s, bbox = _check_crop(face, None)
    assert bbox == [[0, 8], [5, 13], [0, 40]] and (s == 0).all()
    whole = np.ones((1, 3, 4, 5), np.float32)
    assert _check_crop(whole, None)[2] == [[0, 3], [0, 4], [0, 5]]


def test_crop_to_nonzero_gpu_refuses_what_the_host_refuses():
    from dg_tta_amd.tta import preprocessing as pp
    zero = np.zeros((1, 4, 5, 6), np.float32)
    with pytest.raises(ValueError):
        pp.crop_to_nonzero(zero, None)
    with pytest.raises(ValueError, match="zero"):
        pp.crop_to_nonzero_gpu(zero, None, DEV)
    with pytest.raises(ValueError, match="float32"):
        pp.crop_to_nonzero_gpu(zero.astype(np.float64), None, DEV)


def test_run_case_npy_crops_on_the_gpu(monkeypatch):
    import json
    from pathlib import Path

    from dg_tta_amd.tta import preprocessing as pp
    plans = json.loads((Path(pp.__file__).resolve().parents[1] / "__resources__" / "model_skeleton" / "plans.json").read_text())
    img, seg = _body(2)
    calls = []
    gpu_crop = pp.crop_to_nonzero_gpu
    monkeypatch.setattr(pp, "crop_to_nonzero_gpu", lambda *a, **k: calls.append(1) or gpu_crop(*a, **k))
    d, s, props = pp.run_case_npy(img.copy(), seg.copy(), (1.5, 1.5, 1.5), plans, "3d_fullres", "cuda:0")
    assert calls == [1]
    monkeypatch.setattr(pp, "crop_to_nonzero_gpu", lambda data, seg, device: pp.crop_to_nonzero(data, seg))
    d2, s2, props2 = pp.run_case_npy(img.copy(), seg.copy(), (1.5, 1.5, 1.5), plans, "3d_fullres", "cuda:0")
    assert np.array_equal(d, d2) and np.array_equal(s, s2) and s.dtype == s2.dtype
    assert props["bbox_used_for_cropping"] == props2["bbox_used_for_cropping"]
