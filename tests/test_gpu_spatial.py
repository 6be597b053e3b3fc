"""GPU: csrc/spatial_aug.hip (dgtta_bspline3_prefilter, dgtta_patch_sample_aug) against the float64 restatement
tests/spatial_ref.py - whose docstring derives the error bound asserted here - and the trainer paths of
`dgtta pretrain --augmentation spatial`.  The shapes are the smallest at which the kernels can still go wrong: lines shorter
and longer than a wave, extents that are no multiple of 4, three items of different volume shape in one launch, one of them
smaller than the patch.

Largest error / bound ratios measured on an MI355X (printed by the tests): prefilter 0.024 (5x6x7) and 0.034
(9x70x11); sampler order 3 0.0062, order 1 0.22; no label voxel differed, none was excluded for a tie and one image voxel for a face."""
import functools
import json

import numpy as np
import pytest
import torch

import spatial_ref as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _case(item):
    img, lab = sref.make_case(sref.SHAPES[item], 40 + item)
    return img, lab, sref.prefilter(img)


@pytest.mark.parametrize("shape", sref.PREFILTER_SHAPES)
def test_prefilter_against_float64(shape):
    from dg_tta_amd import ops
    vol = np.random.RandomState(sum(shape)).standard_normal(shape).astype(np.float32)
    ref = sref.prefilter(vol)
    x = torch.from_numpy(vol).to(DEV)
    got = ops.bspline3_prefilter(x)
    assert got.dtype == torch.float32 and got.shape == x.shape and torch.equal(x.cpu(), torch.from_numpy(vol))
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max()
    bound = sref.K_PRE * sref.U * float(np.abs(vol).max())
    print(f"\nprefilter {shape}: max err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.4f}")
    assert err <= bound
    # in place (dst = src) gives the same bits
    from dg_tta_amd import _lib
    y = x.clone()
    _lib.check(_lib.load().dgtta_bspline3_prefilter(y.data_ptr(), y.data_ptr(), *shape, _lib.stream_of(x.device)), "prefilter")
    assert torch.equal(y, got)


@pytest.mark.parametrize("order", [3, 1])
@pytest.mark.parametrize("row", range(len(sref.MAP_TABLE)))
def test_sampler_against_float64(row, order):
    from dg_tta_amd import ops
    name, _, _, exact = sref.MAP_TABLE[row]
    maps = [sref.table_map(row, shape, item) for item, shape in enumerate(sref.SHAPES)]
    vols = [torch.from_numpy(_case(i)[0]).to(DEV) for i in range(3)]
    labs = [torch.from_numpy(_case(i)[1]).to(DEV) for i in range(3)]
    srcs = [ops.bspline3_prefilter(v) for v in vols] if order == 3 else vols
    image, labels = ops.sample_patches_aug(srcs, labs, maps, sref.PATCH, order=order)       # ONE launch, three volume shapes
    assert image.shape == (3, 1, *sref.PATCH) and image.dtype == torch.float32
    assert labels.shape == (3, *sref.PATCH) and labels.dtype == torch.int64
    image, labels = image.cpu().numpy().astype(np.float64), labels.cpu().numpy()
    total = 3 * int(np.prod(sref.PATCH))
    worst = n_face = n_near = n_inside = 0
    for item in range(3):
        img, lab, coef = _case(item)
        ref, s, t, inside, face = sref.sample_image(coef if order == 3 else img, maps[item], sref.PATCH, order)
        ref_lab, near, _ = sref.sample_labels(lab, maps[item], sref.PATCH)
        bound = sref.error_bound(order, s, t, float(np.abs(img).max()))
        keep_img = np.ones(sref.PATCH, dtype=bool) if exact else face > 1e-4
        keep_lab = np.ones(sref.PATCH, dtype=bool) if exact else ~near
        n_face += int((~keep_img).sum())
        n_near += int((~keep_lab).sum())
        n_inside += int(inside.sum())
        err = np.abs(image[item, 0] - ref)
        assert np.all(image[item, 0][~inside & keep_img] == 0.0), f"{name}, item {item}: a voxel outside the volume is not 0"
        sel = inside & keep_img
        if sel.any():
            worst = max(worst, float((err[sel] / bound[sel]).max()))
        assert np.all(err[sel] <= bound[sel]), f"{name}, item {item}, order {order}: err / bound {(err[sel] / bound[sel]).max():.3f}"
        assert np.array_equal(labels[item][keep_lab], ref_lab[keep_lab]), \
            f"{name}, item {item}: {(labels[item] != ref_lab)[keep_lab].sum()} label voxels differ"
        if exact:
            assert np.array_equal(labels[item], sref.integer_crop(lab, maps[item], sref.PATCH).astype(np.int64))
            crop = sref.integer_crop(img.astype(np.float64), maps[item], sref.PATCH)
            assert np.all(np.abs(image[item, 0] - crop) <= np.where(inside, bound, 0.0))
    print(f"\nsampler {name}, order {order}: {n_inside} of {total} voxels inside, largest err / bound {worst:.4f}, excluded "
          f"{n_face} image / {n_near} label voxels")
    assert n_inside > total // 10
    if exact:
        assert n_face == 0 and n_near == 0
    else:
        assert n_near <= 0.005 * total and n_face <= 0.01 * total


def test_sampler_rejects_what_it_cannot_take():
    from dg_tta_amd import ops
    from dg_tta_amd._lib import DgttaError
    v = torch.zeros(4, 4, 4, device=DEV)
    eye = np.eye(3, 4)
    with pytest.raises(ValueError):
        ops.sample_patches_aug([v] * 17, [v] * 17, [eye] * 17, (2, 2, 2))
    with pytest.raises(ValueError):
        ops.sample_patches_aug([v], [v], [eye], (2, 2, 2), order=2)
    with pytest.raises(ValueError):
        ops.sample_patches_aug([v], [v], [eye * np.nan], (2, 2, 2))
    with pytest.raises(ValueError):
        ops.sample_patches_aug([v], [torch.zeros(4, 4, 5, device=DEV)], [eye], (2, 2, 2))
    with pytest.raises(DgttaError):
        ops.sample_patches_aug([v], [v], [eye], (2, 0, 2))
    img, lab = ops.sample_patches_aug([v] * 16, [v] * 16, [eye] * 16, (2, 3, 2))        # 16 items are taken
    assert img.shape == (16, 1, 2, 3, 2) and not img.any() and not lab.any()


# ------------------------------------------------------------------------------------------------ trainer
def _cases(n=3, size=(28, 26, 30)):
    from dg_tta_amd.pretraining.trainer import _Case
    out = []
    for i in range(n):
        img, lab = sref.make_case(size, 70 + i)
        out.append(_Case(f"c{i}", img[None], lab[None].astype(np.int16)))
    return out


def test_sample_without_events_is_get_batch_bit_for_bit():
    from dg_tta_amd.pretraining import trainer
    from dg_tta_amd.pretraining.spatial import SpatialAugmentation
    from dg_tta_amd.tta.torch_utils import get_batch, release_resident
    from dg_tta_amd.utils import numpy_rng
    cases, patch, off = _cases(), [16, 12, 20], SpatialAugmentation(0.0, 0.0)
    release_resident()
    try:
        state = numpy_rng().get_state()
        plan = trainer._plan_batch(cases, 6, patch, off, numpy_rng())
        numpy_rng().set_state(state)
        imgs, target, picks = trainer._sample(cases, 6, patch, DEV, None, spatial=off)
        assert imgs.shape == (6, 1, *patch) and target.shape == (6, *patch) and target.dtype == torch.int64
        assert [p.name for p in picks] == [p[0].name for p in plan] and all(p[2] is None for p in plan)
        for j, (case, center, _) in enumerate(plan):
            im, lb = get_batch([case.tensor], [0], patch, None, DEV, centers=[center])
            assert torch.equal(imgs[j], im[0][0]) and torch.equal(target[j], lb[0][0, 0]), j
    finally:
        release_resident()


def test_sample_with_events_reads_the_map_of_its_centre():
    """Probabilities forced to 1: every item leaves the one sample_patches_aug launch, and is the reference's sample of the
    case through sampling_map(A, patch_start(centre)) - the host chain from the draw to the kernel."""
    from dg_tta_amd.pretraining import trainer
    from dg_tta_amd.pretraining.spatial import SpatialAugmentation, patch_start, sampling_map
    from dg_tta_amd.tta import torch_utils
    from dg_tta_amd.utils import numpy_rng
    cases, patch, on = _cases(), [16, 12, 20], SpatialAugmentation(1.0, 1.0)
    torch_utils.release_resident()
    try:
        state = numpy_rng().get_state()
        plan = trainer._plan_batch(cases, 3, patch, on, numpy_rng())
        numpy_rng().set_state(state)
        imgs, target, _ = trainer._sample(cases, 3, patch, DEV, None, spatial=on)
        assert len(torch_utils._SPLINE_CACHE) == len({p[0].name for p in plan})
        for j, (case, center, a) in enumerate(plan):
            img, lab = case.tensor[0].numpy(), case.tensor[1].numpy()
            m = sampling_map(a, patch_start(center, img.shape, patch), patch)
            ref, s, t, inside, face = sref.sample_image(sref.prefilter(img), m, patch, 3)
            ref_lab, near, _ = sref.sample_labels(lab, m, patch)
            sel = face > 1e-4
            err = np.abs(imgs[j, 0].cpu().numpy().astype(np.float64) - ref)
            assert np.all(err[sel] <= sref.error_bound(3, s, t, float(np.abs(img).max()))[sel])
            assert np.array_equal(target[j].cpu().numpy()[~near], ref_lab[~near]) and near.mean() <= 0.005 and (~sel).mean() <= 0.01
        coef = torch_utils.resident_spline(cases[0].tensor, torch.device(DEV))
        assert torch_utils.resident_spline(cases[0].tensor, torch.device(DEV)) is coef      # cached
        torch_utils.release_resident([cases[0].tensor])
        assert all(k[0] != id(cases[0].tensor) for k in list(torch_utils._SPLINE_CACHE) + list(torch_utils._VOLUME_CACHE))
    finally:
        torch_utils.release_resident()
    assert not torch_utils._SPLINE_CACHE and not torch_utils._VOLUME_CACHE


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """The tiny source dataset of tests/test_gpu_pretrain.py: three 48^3 cases, 32^3 patches, batch 2."""
    from test_gpu_pretrain import _small_plans, _write_case
    tmp = tmp_path_factory.mktemp("spatial")
    raw, pre = tmp / "raw", tmp / "pre"
    src = raw / "Dataset802_Source"
    (src / "imagesTr").mkdir(parents=True)
    (src / "labelsTr").mkdir()
    for i in range(3):
        _write_case(src / "imagesTr", src / "labelsTr", f"ct{i:02d}", 48, 11 + i)
    json.dump({"labels": {"background": 0, "liver": 1, "spleen": 2, "kidney": 3}, "file_ending": ".nii.gz",
               "channel_names": {"0": "CT"}, "numTraining": 3}, open(src / "dataset.json", "w"))
    (pre / "Dataset802_Source").mkdir(parents=True)
    json.dump(_small_plans(), open(pre / "Dataset802_Source" / "nnUNetPlans.json", "w"))
    return tmp


def _train(dataset, monkeypatch, tag, augmentation):
    from dg_tta_amd.pretraining import trainer
    for k, v in {"nnUNet_raw": dataset / "raw", "nnUNet_results": dataset / f"res_{tag}", "nnUNet_preprocessed": dataset / "pre"}.items():
        monkeypatch.setenv(k, str(v))
    seen = []
    sample = getattr(trainer._sample, "wrapped", trainer._sample)

    def watched(*args, **kwargs):
        out = sample(*args, **kwargs)
        seen.append((int(out[1].min()), int(out[1].max()), kwargs.get("spatial", args[5] if len(args) > 5 else None)))
        return out
    watched.wrapped = sample
    monkeypatch.setattr(trainer, "_sample", watched)
    final = trainer.train_fold("802", "3d_fullres", 0, "nnUNetTrainer_GIN_MIND", num_epochs=2, iterations_per_epoch=2, val_iterations=1,
                               device=DEV, seed=3, augmentation=augmentation)
    ck = torch.load(final, map_location="cpu", weights_only=False)
    return final, ck["logging"], seen


def test_train_fold_with_spatial_augmentation(dataset, monkeypatch):
    from dg_tta_amd.pretraining.spatial import SpatialAugmentation
    from dg_tta_amd.tta import torch_utils
    torch_utils.release_resident()
    final, log_a, seen = _train(dataset, monkeypatch, "a", "spatial")
    assert final.name == "checkpoint_final.pth" and final.is_file()
    assert len(log_a["train_losses"]) == 2 and np.isfinite(log_a["train_losses"] + log_a["val_losses"]).all()
    assert not torch_utils._SPLINE_CACHE and not torch_utils._VOLUME_CACHE                # release_resident freed both
    assert len(seen) == 6 and [s[2] is not None for s in seen] == [True, True, False, True, True, False]   # validation: never
    _, log_b, _ = _train(dataset, monkeypatch, "b", "spatial")
    assert log_a["train_losses"] == log_b["train_losses"] and log_a["val_losses"] == log_b["val_losses"]
    _, log_c, seen = _train(dataset, monkeypatch, "c", SpatialAugmentation(1.0, 1.0))
    assert np.isfinite(log_c["train_losses"] + log_c["val_losses"]).all()
    assert all(0 <= lo and hi < 4 for lo, hi, _ in seen)                                     # num_classes = 4
    assert log_c["train_losses"] != log_a["train_losses"]
    assert not torch_utils._SPLINE_CACHE
