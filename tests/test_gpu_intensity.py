"""GPU: csrc/intensity_aug.hip (dgtta_intensity_stats, dgtta_intensity_map, dgtta_gauss_blur3) stage by stage against the
float64 restatement tests/intensity_ref.py - whose docstring derives the error bounds asserted here, on ALL voxels - the chain
of pretraining/intensity.py against its own stages bit for bit, and the trainer paths of `dgtta pretrain --augmentation
full`.  The shapes are the smallest at which the kernels can still go wrong: lines shorter and longer than a wave, extents that
are no multiple of 4 (scalar paths) and one that is (16-byte paths, more than one chunk), extents equal to and below the blur
radius; batches of 3 items with the middle one not named.

Largest error / bound ratios measured on an MI355X over all shapes and both named items (printed by the tests): noise 0.26,
brightness 0.95 (one rounding is the whole bound, and round-to-nearest reaches it), noise + brightness 0.46, contrast 0.64, gamma
power 0.41 (inverted 0.56), restore 0.49 (inverted 0.58), blur 0.095, mean 0.005, std 0.020; no voxel excluded."""
import functools
import json

import numpy as np
import pytest
import torch

import intensity_ref as iref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEL = list(iref.SELECTED)


@functools.lru_cache(maxsize=None)
def _batch(shape):
    x = iref.make_batch(shape)
    x.setflags(write=False)
    return x


def _gpu(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def _f64(t):
    return t.cpu().numpy().astype(np.float64)


def _check(name, shape, got, ref, bound, item):
    err = np.abs(_f64(got) - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"\n{name} {shape} item {item}: max err {err.max():.3e}, largest err / bound {ratio:.4f}")
    assert np.all(err <= bound), f"{name} {shape} item {item}: err / bound {ratio:.3f}"
    return ratio


def _untouched(y, x, shape):
    assert torch.equal(y[1], _gpu(x[1])), f"{shape}: the item that was not named changed"


@pytest.mark.parametrize("shape", iref.SHAPES)
def test_stats_against_float64(shape):
    from dg_tta_amd import ops
    x = _batch(shape)
    xg = _gpu(x)
    out = torch.full((3, 4), -7.0, dtype=torch.float64, device=DEV)
    assert ops.intensity_stats(xg, SEL, out=out) is out
    got = out.cpu().numpy()
    for item in SEL:
        mn, mx, mean, std = iref.stats(x[item])
        b_mean, b_std = iref.stats_bound(x[item])
        assert got[item, 0] == float(x[item].min()) == mn and got[item, 1] == float(x[item].max()) == mx      # bit-equal fp32 values
        print(f"\nstats {shape} item {item}: mean err / bound {abs(got[item, 2] - mean) / b_mean:.4f}, std err / bound "
              f"{abs(got[item, 3] - std) / b_std:.4f}")
        assert abs(got[item, 2] - mean) <= b_mean and abs(got[item, 3] - std) <= b_std
    assert np.all(got[1] == -7.0)                                          # the row of the item that was not named
    assert torch.equal(ops.intensity_stats(xg, SEL)[SEL], out[SEL])
    again = torch.full((3, 4), -7.0, dtype=torch.float64, device=DEV)
    ops.intensity_stats(xg, SEL, out=again)
    assert torch.equal(again, out) and torch.equal(xg, _gpu(x))            # the same bits on every run; the input is only read
    one = ops.intensity_stats(xg[2:3].clone(), [0])
    assert torch.equal(one[0, :2], out[2, :2]) and abs(float(one[0, 2] - out[2, 2])) <= 2 * iref.stats_bound(x[2])[0]


@pytest.mark.parametrize("shape", iref.SHAPES)
def test_linear_map_noise_and_brightness_against_float64(shape):
    from dg_tta_amd import ops
    x = _batch(shape)
    v = int(np.prod(shape))
    s, m = [float(p) for p in iref.PARAMS["s"]], [float(p) for p in iref.PARAMS["m"]]
    noise = [iref.noise_field(iref.KEYS[k], item, v) for k, item in enumerate(SEL)]
    y_noise = ops.intensity_map(_gpu(x), SEL, "linear", s=s, keys=iref.KEYS)
    y_bright = ops.intensity_map(_gpu(x), SEL, "linear", a=m)
    y_both = ops.intensity_map(_gpu(x), SEL, "linear", a=m, s=s, keys=iref.KEYS)
    for k, item in enumerate(SEL):
        xi = x[item, 0]
        _check("noise", shape, y_noise[item, 0], iref.linear(xi, 1.0, s[k], noise[k]), iref.linear_bound(xi, 1.0, s[k], noise[k]), item)
        _check("brightness", shape, y_bright[item, 0], iref.linear(xi, m[k]), iref.linear_bound(xi, m[k], 0.0, None), item)
        _check("noise + brightness", shape, y_both[item, 0], iref.linear(xi, m[k], s[k], noise[k]), iref.linear_bound(xi, m[k], s[k], noise[k]), item)
        assert torch.equal(y_bright[item, 0], _gpu(x[item, 0] * np.float32(m[k])))        # one fp32 product, no noise term
    for y in (y_noise, y_bright, y_both):
        _untouched(y, x, shape)
    # out of place: the same bits, and the item that is not named is not written
    out = torch.full((3, 1, *shape), -3.0, dtype=torch.float32, device=DEV)
    xg = _gpu(x)
    assert ops.intensity_map(xg, SEL, "linear", a=m, s=s, keys=iref.KEYS, out=out) is out and torch.equal(xg, _gpu(x))
    assert torch.equal(out[SEL], y_both[SEL]) and bool((out[1] == -3.0).all())


@pytest.mark.parametrize("shape", [iref.SHAPES[0], iref.SHAPES[4]])
def test_noise_depends_on_key_item_index_and_voxel_only(shape):
    from dg_tta_amd import ops
    x = _batch(shape)
    s = [0.1, 0.1]

    def run(keys, **kw):
        return ops.intensity_map(_gpu(x), SEL, "linear", s=s, keys=keys, **kw)
    a = run(iref.KEYS)
    assert torch.equal(a, run(iref.KEYS))                                                 # the same key: the same bits
    other_key, other_index, other_offset = run([iref.KEYS[0] ^ 1, iref.KEYS[1]]), run(iref.KEYS, noise_index=[1, 2]), run(iref.KEYS, offset=1)
    assert not torch.equal(a[0], other_key[0]) and torch.equal(a[2], other_key[2])
    assert not torch.equal(a[0], other_index[0]) and torch.equal(a[2], other_index[2])
    assert not torch.equal(a[0], other_offset[0]) and not torch.equal(a[2], other_offset[2])
    # item 2 of the 3-item launch = the same item launched alone with its index handed in ...
    alone = ops.intensity_map(_gpu(x[2:3]), [0], "linear", s=[0.1], keys=[iref.KEYS[1]], noise_index=[2])
    assert torch.equal(alone[0], a[2])
    # ... also from an address that is not 16-byte aligned (the scalar path where the batch took the 16-byte one)
    v = int(np.prod(shape))
    buf = torch.zeros(v + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(1, 1, *shape)
    view.copy_(_gpu(x[2:3]))
    assert view.data_ptr() % 16 != 0
    ops.intensity_map(view, [0], "linear", s=[0.1], keys=[iref.KEYS[1]], noise_index=[2])
    assert torch.equal(view[0], a[2])


@pytest.mark.parametrize("shape", iref.SHAPES)
def test_contrast_against_float64(shape):
    from dg_tta_amd import ops
    x = _batch(shape)
    f = [float(p) for p in iref.PARAMS["f"]]
    xg = _gpu(x)
    st = ops.intensity_stats(xg, SEL)
    y = ops.intensity_map(xg, SEL, "contrast", a=f, stats=st, out=torch.empty_like(xg).copy_(xg))
    in_place = ops.intensity_map(_gpu(x), SEL, "contrast", a=f, stats=st)
    assert torch.equal(in_place, y)                                                        # dst == src: the same bits
    clipped = 0
    for k, item in enumerate(SEL):
        xi = x[item, 0]
        bound = iref.contrast_bound(xi, f[k])
        _check("contrast", shape, y[item, 0], iref.contrast(xi, f[k]), bound, item)
        got, raw = y[item, 0].cpu().numpy(), iref.contrast(xi, f[k], clip=False)
        assert got.min() >= xi.min() and got.max() <= xi.max()
        assert np.all(got[raw > xi.max() + bound] == xi.max()) and np.all(got[raw < xi.min() - bound] == xi.min())   # exactly fp32 min / max
        clipped += int((raw > xi.max() + bound).sum() + (raw < xi.min() - bound).sum())
    assert clipped > 0 or f[1] <= 1.0
    _untouched(y, x, shape)


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("shape", iref.SHAPES)
def test_gamma_power_and_restore_against_float64(shape, negate):
    from dg_tta_amd import ops
    x = _batch(shape)
    g = [float(p) for p in iref.PARAMS["g"]]
    xg = _gpu(x)
    before = ops.intensity_stats(xg, SEL)
    y = ops.intensity_map(xg, SEL, "gamma", a=g, negate=negate, stats=before, out=torch.empty_like(xg).copy_(xg))
    assert torch.equal(ops.intensity_map(_gpu(x), SEL, "gamma", a=g, negate=negate, stats=before), y)          # in place
    after = ops.intensity_stats(y, SEL)
    z = ops.intensity_map(y, SEL, "restore", negate=negate, stats=before, stats2=after, out=torch.empty_like(y).copy_(y))
    assert torch.equal(ops.intensity_map(y.clone(), SEL, "restore", negate=negate, stats=before, stats2=after), z)
    for k, item in enumerate(SEL):
        xi = x[item, 0]
        _check(f"gamma power (negate {negate})", shape, y[item, 0], iref.gamma_power(xi, g[k], negate), iref.gamma_power_bound(xi, g[k], negate), item)
        # the restore step on ITS exact fp32 input: the power as the kernel wrote it
        y32 = y[item, 0].cpu().numpy()
        s0, s1 = iref.stats(xi), iref.stats(y32)
        _check(f"gamma restore (negate {negate})", shape, z[item, 0], iref.restore(y32, s0, s1, negate), iref.restore_bound(y32, s0, s1, negate), item)
    _untouched(y, x, shape)
    _untouched(z, x, shape)


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("shape", iref.SHAPES)
def test_gauss_blur_against_float64(shape, pair):
    from dg_tta_amd import ops
    x = _batch(shape)
    sigmas = iref.PARAMS["sigma"][2 * pair:2 * pair + 2]                                   # radii (2, 3) and (4, 4)
    xg = _gpu(x)
    out = torch.full((3, 1, *shape), -3.0, dtype=torch.float32, device=DEV)
    assert ops.gauss_blur3(xg, SEL, sigmas, out=out) is out and torch.equal(xg, _gpu(x))
    for k, item in enumerate(SEL):
        _check(f"blur sigma {sigmas[k]}", shape, out[item, 0], iref.blur(x[item, 0], sigmas[k]), iref.blur_bound(x[item, 0], sigmas[k]), item)
    assert bool((out[1] == -3.0).all())                                                     # not written
    in_place = ops.gauss_blur3(_gpu(x), SEL, sigmas)
    assert torch.equal(in_place[SEL], out[SEL])                                             # dst == src: the same bits
    _untouched(in_place, x, shape)
    scratch = torch.full_like(xg, 5.0)
    assert torch.equal(ops.gauss_blur3(_gpu(x), SEL, sigmas, scratch=scratch)[SEL], out[SEL]) and bool((scratch[1] == 5.0).all())


def test_a_constant_item_stays_finite_and_as_it_is():
    from dg_tta_amd import ops
    x = iref.make_batch((5, 6, 7))
    x[0] = np.float32(-1.75)
    xg = _gpu(x)
    st = ops.intensity_stats(xg, [0, 2])
    assert st[0].tolist() == [-1.75, -1.75, -1.75, 0.0]
    y = ops.intensity_map(xg.clone(), [0, 2], "contrast", a=[1.2, 1.2], stats=st)
    assert torch.isfinite(y).all() and torch.equal(y[0], xg[0])
    for negate in (False, True):
        p = ops.intensity_map(xg.clone(), [0, 2], "gamma", a=[0.8, 1.4], negate=negate, stats=st)
        z = ops.intensity_map(p.clone(), [0, 2], "restore", negate=negate, stats=st, stats2=ops.intensity_stats(p, [0, 2]))
        assert torch.isfinite(p).all() and torch.isfinite(z).all() and torch.equal(z[0], xg[0])
    blurred = ops.gauss_blur3(xg.clone(), [0], [0.7])[0]                  # the fp32 taps sum to 1 within their roundings only
    assert float((blurred - xg[0]).abs().max()) <= iref.blur_bound(x[0], 0.7)


def test_the_ops_reject_what_they_cannot_take():
    from dg_tta_amd import ops
    x = torch.zeros(3, 1, 4, 4, 4, device=DEV)
    many = torch.zeros(17, 1, 2, 2, 2, device=DEV)
    st = torch.zeros(3, 4, dtype=torch.float64, device=DEV)
    calls = [
        lambda: ops.intensity_stats(many, range(17)),
        lambda: ops.intensity_map(many, range(17), "linear"),
        lambda: ops.gauss_blur3(many, range(17), [0.7] * 17),
        lambda: ops.intensity_stats(x.cpu(), [0]),
        lambda: ops.intensity_map(x.cpu(), [0], "linear"),
        lambda: ops.gauss_blur3(x.cpu(), [0], [0.7]),
        lambda: ops.intensity_stats(x.double(), [0]),
        lambda: ops.intensity_map(x.transpose(3, 4), [0], "linear"),
        lambda: ops.gauss_blur3(x[:, :, ::2], [0], [0.7]),
        lambda: ops.intensity_stats(x, []),
        lambda: ops.intensity_stats(x, [0, 0]),
        lambda: ops.intensity_stats(x, [3]),
        lambda: ops.intensity_stats(x, [0], out=st.float()),
        lambda: ops.intensity_map(x, [0], "linear", a=[float("nan")]),
        lambda: ops.intensity_map(x, [0], "linear", s=[float("inf")]),
        lambda: ops.intensity_map(x, [0, 1], "linear", a=[1.0]),
        lambda: ops.intensity_map(x, [0], "sharpen"),
        lambda: ops.intensity_map(x, [0], "contrast", a=[1.1]),                              # no stats
        lambda: ops.intensity_map(x, [0], "gamma", a=[0.0], stats=st),
        lambda: ops.intensity_map(x, [0], "restore", stats=st),                              # no stats2
        lambda: ops.intensity_map(x, [0], "restore", stats=st, stats2=st[:2]),
        lambda: ops.intensity_map(x, [0], "linear", out=torch.zeros(3, 1, 4, 4, 5, device=DEV)),
        lambda: ops.gauss_blur3(x, [0], [0.0]),
        lambda: ops.gauss_blur3(x, [0], [1.5]),
        lambda: ops.gauss_blur3(x, [0], [float("nan")]),
        lambda: ops.gauss_blur3(x, [0, 1], [0.7]),
        lambda: ops.gauss_blur3(x, [0], [0.7], scratch=x),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was taken")
    sixteen = torch.ones(16, 1, 2, 3, 2, device=DEV)                                        # 16 items are taken
    assert torch.equal(ops.intensity_map(sixteen, range(16), "linear", a=[2.0] * 16), torch.full((16, 1, 2, 3, 2), 2.0, device=DEV))
    assert float((ops.gauss_blur3(sixteen, range(16), [1.0] * 16) - 2.0).abs().max()) <= iref.blur_bound(np.float32(2.0), 1.0)


# ------------------------------------------------------------------------------------------------ chain
def _by_hand(images, plan):
    """The stages of pretraining/intensity.py one ops call after the other, with the plan's parameters."""
    from dg_tta_amd import ops
    from dg_tta_amd.pretraining.intensity import simulate_low_resolution
    x = images.clone()
    idx = plan.fired("noise")
    if idx:
        ops.intensity_map(x, idx, "linear", s=[plan.noise[i][0] for i in idx], keys=[plan.noise[i][1] for i in idx])
    idx = plan.fired("blur")
    if idx:
        ops.gauss_blur3(x, idx, [plan.blur[i] for i in idx])
    idx = plan.fired("brightness")
    if idx:
        ops.intensity_map(x, idx, "linear", a=[plan.brightness[i] for i in idx])
    idx = plan.fired("contrast")
    if idx:
        ops.intensity_map(x, idx, "contrast", a=[plan.contrast[i] for i in idx], stats=ops.intensity_stats(x, idx))
    for i in plan.fired("lowres"):
        x[i, 0] = simulate_low_resolution(x[i, 0], plan.lowres[i], plan.thin)
    for stage, negate in (("gamma_inverted", True), ("gamma", False)):
        idx = plan.fired(stage)
        if idx:
            g = [getattr(plan, stage)[i] for i in idx]
            before = ops.intensity_stats(x, idx)
            ops.intensity_map(x, idx, "gamma", a=g, negate=negate, stats=before)
            ops.intensity_map(x, idx, "restore", negate=negate, stats=before, stats2=ops.intensity_stats(x, idx))
    return x


@pytest.mark.parametrize("shape", [(10, 12, 14), iref.SHAPES[4]])          # isotropic; thin axis 0 (stage 5 leaves it alone)
def test_chain_is_its_stages_bit_for_bit(shape):
    from dg_tta_amd.pretraining.intensity import STAGES, IntensityAugmentation
    from test_intensity_params import ALL_ON
    images = _gpu(np.concatenate([iref.make_batch(shape), iref.make_batch(shape, seed=1)]))  # 6 items
    kept = images.clone()
    on = IntensityAugmentation(**ALL_ON)
    plan = on.draw(6, shape, np.random.RandomState(5))
    assert all(plan.fired(s) == list(range(6)) for s in STAGES) and plan.thin == (0 if shape == iref.SHAPES[4] else None)
    out = on.apply(images, plan)
    assert out.shape == images.shape and out.dtype == torch.float32 and torch.equal(images, kept) and torch.isfinite(out).all()
    assert torch.equal(out, _by_hand(images, plan)) and not torch.equal(out, images)
    default = IntensityAugmentation()
    plan = default.draw(6, shape, np.random.RandomState(4))
    fired = [len(plan.fired(s)) for s in STAGES]
    assert 0 < sum(fired) < 6 * len(STAGES) and 0 in fired                                   # some stages fire, some do not
    out = default.apply(images, plan)
    assert torch.equal(out, _by_hand(images, plan)) and torch.equal(images, kept)
    touched = sorted({i for s in STAGES for i in plan.fired(s)})
    assert all(torch.equal(out[i], images[i]) for i in range(6) if i not in touched) and len(touched) < 6
    nothing = IntensityAugmentation(**{k: 0.0 for k in ALL_ON})
    out = nothing.apply(images, nothing.draw(6, shape, np.random.RandomState(1)))
    assert torch.equal(out, images) and out.data_ptr() != images.data_ptr()


# ------------------------------------------------------------------------------------------------ trainer
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """The tiny source dataset of tests/test_gpu_pretrain.py: three 48^3 cases, 32^3 patches, batch 2."""
    from test_gpu_pretrain import _small_plans, _write_case
    tmp = tmp_path_factory.mktemp("intensity")
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


def _train(dataset, monkeypatch, tag, augmentation, trainer_name="nnUNetTrainer_GIN_MIND"):
    from dg_tta_amd.pretraining import trainer
    for k, v in {"nnUNet_raw": dataset / "raw", "nnUNet_results": dataset / f"res_{tag}", "nnUNet_preprocessed": dataset / "pre"}.items():
        monkeypatch.setenv(k, str(v))
    seen = []
    sample = getattr(trainer._sample, "wrapped", trainer._sample)

    def watched(*args, **kwargs):
        out = sample(*args, **kwargs)
        seen.append((int(out[1].min()), int(out[1].max()), args[5] if len(args) > 5 else kwargs.get("spatial"), kwargs.get("intensity"),
                     bool(torch.isfinite(out[0]).all())))
        return out
    watched.wrapped = sample
    monkeypatch.setattr(trainer, "_sample", watched)
    final = trainer.train_fold("802", "3d_fullres", 0, trainer_name, num_epochs=2, iterations_per_epoch=2, val_iterations=1,
                               device=DEV, seed=3, augmentation=augmentation)
    ck = torch.load(final, map_location="cpu", weights_only=False)
    return final, ck["logging"], seen


_DEFAULT_RUN = {}          # the log of the default `full` run, shared by the tests below (trained again only when run alone)


def test_train_fold_with_full_augmentation(dataset, monkeypatch):
    from dg_tta_amd.tta import torch_utils
    torch_utils.release_resident()
    final, log_a, seen = _train(dataset, monkeypatch, "a", "full")
    assert final.name == "checkpoint_final.pth" and final.is_file()
    assert len(log_a["train_losses"]) == 2 and np.isfinite(log_a["train_losses"] + log_a["val_losses"]).all()
    assert not torch_utils._SPLINE_CACHE and not torch_utils._VOLUME_CACHE                # release_resident freed both
    train = [True, True, False, True, True, False]                                          # validation batches: never augmented
    assert len(seen) == 6 and [s[2] is not None for s in seen] == train and [s[3] is not None for s in seen] == train
    _, log_b, _ = _train(dataset, monkeypatch, "b", "full")
    assert log_a["train_losses"] == log_b["train_losses"] and log_a["val_losses"] == log_b["val_losses"]
    assert not torch_utils._SPLINE_CACHE and not torch_utils._VOLUME_CACHE
    _DEFAULT_RUN["log"] = log_a


def test_train_fold_with_every_intensity_stage_on(dataset, monkeypatch):
    from dg_tta_amd.pretraining.intensity import IntensityAugmentation
    from dg_tta_amd.tta import torch_utils
    from test_intensity_params import ALL_ON
    torch_utils.release_resident()
    log_a = _DEFAULT_RUN["log"] if _DEFAULT_RUN else _train(dataset, monkeypatch, "d", "full")[1]
    _, log_c, seen = _train(dataset, monkeypatch, "c", IntensityAugmentation(**ALL_ON))
    assert np.isfinite(log_c["train_losses"] + log_c["val_losses"]).all() and all(s[4] for s in seen)
    assert all(0 <= lo and hi < 4 for lo, hi, *_ in seen)                                    # num_classes = 4: labels untouched
    assert [s[2] is None for s in seen] == [True] * 6 and [s[3] is not None for s in seen] == [True, True, False, True, True, False]
    assert log_c["train_losses"] != log_a["train_losses"]
    assert not torch_utils._SPLINE_CACHE and not torch_utils._VOLUME_CACHE


def test_train_fold_multires_takes_the_discrete_transform_in_stage_5(dataset, monkeypatch):
    """Once more with a *_MultiRes trainer: stage 5 is the discrete transform, called from inside the chain."""
    from dg_tta_amd.pretraining import discrete_downsampling, trainer
    from dg_tta_amd.pretraining.intensity import IntensityAugmentation
    from dg_tta_amd.tta import torch_utils
    from test_intensity_params import ALL_ON
    torch_utils.release_resident()
    plans, calls = [], []
    draw, discrete = IntensityAugmentation.draw, discrete_downsampling.SimulateDiscreteLowResolutionTransform.__call__

    def watched_draw(self, *args, **kwargs):
        plans.append(draw(self, *args, **kwargs))
        return plans[-1]

    def watched_discrete(self, **data):
        calls.append(len(data["data"]))
        return discrete(self, **data)
    monkeypatch.setattr(IntensityAugmentation, "draw", watched_draw)
    monkeypatch.setattr(discrete_downsampling.SimulateDiscreteLowResolutionTransform, "__call__", watched_discrete)
    pair = (trainer.SpatialAugmentation(1.0, 1.0), IntensityAugmentation(**ALL_ON))
    final, log_m, seen = _train(dataset, monkeypatch, "m", pair, trainer_name="nnUNetTrainer_GIN_MIND_MultiRes")
    assert final.is_file() and np.isfinite(log_m["train_losses"] + log_m["val_losses"]).all() and all(s[4] for s in seen)
    assert len(plans) == 4 and all(isinstance(p.lowres, discrete_downsampling.SimulateDiscreteLowResolutionTransform) for p in plans)
    assert calls == [2, 2, 2, 2]                                                              # once per training batch, inside apply
    assert all(0 <= lo and hi < 4 for lo, hi, *_ in seen)
    assert not torch_utils._SPLINE_CACHE and not torch_utils._VOLUME_CACHE
