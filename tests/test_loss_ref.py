"""CPU: tests/loss_ref.py (the float64 restatements the GPU tests of csrc/softdice.hip and csrc/dice_ce.hip compare with)
against float64 torch autograd of the oracle (oracle.tta.consistency_loss, soft_dice_loss) and of plain torch restatements
written here.  Everything is float64: agreement to about 1e-12."""
import numpy as np
import pytest
import torch

import loss_ref
from oracle import tta as otta

TOL = dict(rtol=1e-11, atol=1e-13)


def _logits(rng, B, C, V, masked=True):
    """Logits with a positive class sum at most voxels, plus - when `masked` - voxels masked by either branch or both."""
    la, lb = rng.normal(size=(B, C, V)) * 2 + 3 / np.sqrt(C), rng.normal(size=(B, C, V)) * 2 + 3 / np.sqrt(C)
    if masked and V >= 8:
        la[:, :, 0] = lb[:, :, 0] = 0.0                    # exact zeros: the warp's border (sum > 0 is false)
        la[:, :, 1] -= np.abs(la[:, :, 1].sum(1, keepdims=True)) / C + 1       # negative sum in branch a only
        lb[:, :, 2] -= np.abs(lb[:, :, 2].sum(1, keepdims=True)) / C + 1       # ... in branch b only
    return la, lb


def _torch_softdice(la, lb, start_class, guard_items):
    """Plain torch float64 restatement with the start class and the guard groups of the kernel's ABI."""
    B, C, V = la.shape
    mask = ((la.sum(1, keepdim=True) > 0) & (lb.sum(1, keepdim=True) > 0)).double()
    a, b = la.softmax(1) * mask, lb.softmax(1) * mask
    nom, den = (2 * a * b).mean(2), 0.5 * ((a + b) ** 2).mean(2)
    rows = []
    for g0 in range(0, B, guard_items):
        n, d = nom[g0:g0 + guard_items], den[g0:g0 + guard_items]
        rows.append(n * 0 + 1 if float(d.sum().detach()) == 0.0 else n / d)
    dice = torch.cat(rows)
    return 1 - dice[:, start_class:].mean(), dice


@pytest.mark.parametrize("B,C,V", [(1, 2, 1), (2, 5, 37), (3, 16, 64), (1, 70, 9), (2, 128, 5)])
def test_softdice_matches_the_oracle(B, C, V):
    rng = np.random.RandomState(B * 1000 + C)
    la, lb = _logits(rng, B, C, V)
    ta, tb = (torch.tensor(x.reshape(B, C, V, 1, 1), requires_grad=True) for x in (la, lb))
    want = otta.consistency_loss(ta, tb)
    want.backward()
    assert otta.START_CLASS == 1
    loss, dice, ga, gb = loss_ref.softdice(la, lb, 1)
    np.testing.assert_allclose(loss, float(want.detach()), **TOL)
    np.testing.assert_allclose(ga, ta.grad.numpy().reshape(B, C, V), **TOL)
    np.testing.assert_allclose(gb, tb.grad.numpy().reshape(B, C, V), **TOL)
    mask = ((ta.sum(1, keepdim=True) > 0) & (tb.sum(1, keepdim=True) > 0)).double()
    d = otta.soft_dice_loss(ta.detach().softmax(1) * mask, tb.detach().softmax(1) * mask)
    np.testing.assert_allclose(dice, d.numpy(), **TOL)
    if V >= 8:
        assert 0 < float(mask.mean()) < 1 and not ga[:, :, :3].any() and not gb[:, :, :3].any()


@pytest.mark.parametrize("start_class", [0, 1, 4])
@pytest.mark.parametrize("guard_items", [1, 2, 4])
def test_softdice_start_class_and_guard_groups(start_class, guard_items):
    """B = 4, items 2 and 3 fully masked: with guard_items 1 or 2 their group's dice is 1 and its gradient 0 while the others
    are ordinary; with guard_items 4 (the oracle's whole-call guard) no group is all zero and their dice is 0 / 0."""
    rng = np.random.RandomState(7)
    B, C, V = 4, 5, 23
    la, lb = _logits(rng, B, C, V)
    la[2:] = -np.abs(la[2:])
    ta, tb = torch.tensor(la, requires_grad=True), torch.tensor(lb, requires_grad=True)
    want, wdice = _torch_softdice(ta, tb, start_class, guard_items)
    loss, dice, ga, gb = loss_ref.softdice(la, lb, start_class, guard_items)
    if guard_items == 4:
        assert np.isnan(dice[2:]).all() and np.isnan(loss) and np.isnan(float(want.detach()))
        np.testing.assert_allclose(dice[:2], wdice.detach().numpy()[:2], **TOL)
        return
    want.backward()
    np.testing.assert_allclose(loss, float(want.detach()), **TOL)
    np.testing.assert_allclose(dice, wdice.detach().numpy(), **TOL)
    np.testing.assert_allclose(ga, ta.grad.numpy(), **TOL)
    np.testing.assert_allclose(gb, tb.grad.numpy(), **TOL)
    assert (dice[2:] == 1).all() and not ga[2:].any() and not gb[2:].any() and ga[:2].any()
    if start_class:
        assert not np.allclose(ga, loss_ref.softdice(la, lb, 0, guard_items)[2])


def test_softdice_default_guard_is_the_whole_call_and_float32_is_close():
    rng = np.random.RandomState(9)
    la, lb = _logits(rng, 2, 6, 50)
    a, b = loss_ref.softdice(la, lb, 1), loss_ref.softdice(la, lb, 1, 2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    z = np.zeros((2, 3, 4))
    loss, dice, ga, gb = loss_ref.softdice(z, z, 1)
    assert loss == 0 and (dice == 1).all() and not ga.any() and not gb.any()
    la32, lb32 = la.astype(np.float32).astype(np.float64), lb.astype(np.float32).astype(np.float64)
    f = loss_ref.softdice(la32, lb32, 1, dtype=np.float32)
    d = loss_ref.softdice(la32, lb32, 1)
    assert all(x.dtype == np.float32 for x in f)
    assert abs(float(f[0]) - float(d[0])) < 1e-6 and np.abs(f[2] - d[2]).max() < 1e-5 * np.abs(d[2]).max()


@pytest.mark.parametrize("B,C,V", [(1, 1, 1), (2, 5, 33), (3, 7, 12)])
def test_softdice_probs_matches_the_oracle(B, C, V):
    rng = np.random.RandomState(B + C + V)
    a, b = rng.uniform(size=(B, C, V)), rng.uniform(size=(B, C, V))
    gd = rng.normal(size=(B, C))
    ta, tb = (torch.tensor(x.reshape(B, C, V, 1, 1), requires_grad=True) for x in (a, b))
    d = otta.soft_dice_loss(ta, tb)
    (d * torch.tensor(gd)).sum().backward()
    np.testing.assert_allclose(loss_ref.softdice_probs(a, b), d.detach().numpy(), **TOL)
    ga, gb = loss_ref.softdice_probs_grad(a, b, gd)
    np.testing.assert_allclose(ga, ta.grad.numpy().reshape(B, C, V), **TOL)
    np.testing.assert_allclose(gb, tb.grad.numpy().reshape(B, C, V), **TOL)
    z = np.zeros((B, C, V))
    assert (loss_ref.softdice_probs(z, z) == 1).all() and not loss_ref.softdice_probs_grad(z, z, gd)[0].any()
    assert (otta.soft_dice_loss(torch.zeros(B, C, V, 1, 1), torch.zeros(B, C, V, 1, 1)) == 1).all()


def _torch_dice_ce(logits, labels, smooth, do_bg):
    """test_pretraining.py::test_dice_ce_loss_matches_torch's restatement in float64, with N >= 1, the 1e-8 clamp of the
    denominator and the background switch."""
    c = logits.shape[1]
    labels = labels[:, None]
    valid = (labels >= 0) & (labels < c)
    safe = labels.clamp(0, c - 1)
    logp = torch.log_softmax(logits, 1)
    ce = -(logp.gather(1, safe) * valid).sum() / valid.sum().clamp_min(1)
    p = logits.softmax(1) * valid
    oh = torch.nn.functional.one_hot(safe[:, 0], c).movedim(-1, 1).double() * valid
    dims = tuple(range(2, logits.dim()))
    dice = (2 * (p * oh).sum(dims) + smooth) / (p.sum(dims) + oh.sum(dims) + smooth).clamp_min(1e-8)
    dl = -dice[:, (0 if do_bg else 1):].mean()
    return ce + dl, ce, dl, dice


def _labels(rng, B, C, shape):
    y = rng.randint(0, C, size=(B, *shape)).astype(np.int64)
    flat = y.reshape(B, -1)
    if flat.shape[1] >= 8:
        flat[0, :4] = [-1, C, 255 if C <= 255 else C + 1, -2 ** 40]          # ignored
    if C > 3:
        flat[flat == C - 2] = 0                                             # an absent class
    if B > 1:
        flat[1] = -1                                                        # one sample entirely ignored
    return y


@pytest.mark.parametrize("do_bg", [False, True])
@pytest.mark.parametrize("smooth", [1e-5, 0.0])
@pytest.mark.parametrize("B,C,V", [(1, 2, 1), (2, 3, 50), (3, 16, 31), (1, 128, 9)])
def test_dice_ce_matches_torch_float64(B, C, V, smooth, do_bg):
    rng = np.random.RandomState(C * 10 + V)
    z = rng.normal(size=(B, C, V)) * 3
    y = _labels(rng, B, C, (V,))
    tz = torch.tensor(z, requires_grad=True)
    loss, ce, dl, dice = _torch_dice_ce(tz, torch.tensor(y), smooth, do_bg)
    loss.backward()
    (rl, rce, rdl), rdice, rgrad = loss_ref.dice_ce(z, y, smooth, do_bg)
    np.testing.assert_allclose([rl, rce, rdl], [float(x.detach()) for x in (loss, ce, dl)], **TOL)
    np.testing.assert_allclose(rdice, dice.detach().numpy(), **TOL)
    np.testing.assert_allclose(rgrad, tz.grad.numpy(), **TOL)
    if B > 1:
        assert not rgrad[1].any() and (rdice[1] == (1.0 if smooth else 0.0)).all()
    if C > 3 and smooth == 0.0:
        assert (rdice[0, C - 2] == 0).all()                                  # the absent class under smooth = 0


def test_dice_ce_with_the_whole_batch_ignored():
    z = np.random.RandomState(0).normal(size=(2, 4, 10))
    (loss, ce, dl), dice, grad = loss_ref.dice_ce(z, np.full((2, 10), -1), 1e-5, False)
    assert ce == 0 and (dice == 1).all() and loss == -1 and dl == -1 and not grad.any()
    (_, _, dl0), dice0, _ = loss_ref.dice_ce(z, np.full((2, 10), 4), 0.0, True)
    assert (dice0 == 0).all() and dl0 == 0


@pytest.mark.parametrize("strides", [(1, 2, 4), (3, 3, 3), (2, 1, 2), (1, 1, 1)])
def test_dice_ce_strided_labels_are_plain_slicing(strides):
    rng = np.random.RandomState(sum(strides))
    d, h, w = 2, 3, 4
    sd, sh, sw = strides
    full = _labels(rng, 2, 5, (d * sd, h * sh, w * sw))
    low = full[:, sd // 2::sd, sh // 2::sh, sw // 2::sw]
    assert low.shape == (2, d, h, w) and np.array_equal(loss_ref.strided_labels(full, strides), low)
    z = rng.normal(size=(2, 5, d, h, w))
    a = loss_ref.dice_ce(z, full, 1e-5, False, strides)
    b = loss_ref.dice_ce(z.reshape(2, 5, -1), low.reshape(2, -1), 1e-5, False)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2].reshape(2, 5, -1), b[2])
    assert a[2].shape == z.shape
    if strides != (1, 1, 1):
        tz = torch.tensor(z, requires_grad=True)
        loss, _, _, _ = _torch_dice_ce(tz, torch.tensor(np.ascontiguousarray(low)), 1e-5, False)
        loss.backward()
        np.testing.assert_allclose(a[0][0], float(loss.detach()), **TOL)
        np.testing.assert_allclose(a[2], tz.grad.numpy(), **TOL)


def test_the_gpu_tests_judges_reject_nan_and_accept_the_fp32_evaluation():
    """The comparison helpers of tests/test_gpu_loss.py, run here on made-up kernel results: the float32 evaluation itself
    passes (ratio 1), one NaN anywhere - loss slot, dice, either gradient - or a gradient wrong in one element fails."""
    from test_gpu_loss import _judge, _probs_check
    rng = np.random.RandomState(3)
    la, lb = _logits(rng, 2, 5, 40)
    la, lb = la.astype(np.float32).astype(np.float64), lb.astype(np.float32).astype(np.float64)
    ref64, ref32 = loss_ref.softdice(la, lb, 1), loss_ref.softdice(la, lb, 1, dtype=np.float32)

    def got(**poison):
        g = dict(loss=np.float32(ref32[0]), dice=ref32[1].copy(), ga=ref32[2].copy(), gb=ref32[3].copy())
        for k, idx in poison.items():
            if g[k].ndim:
                g[k][idx] = np.nan
            else:
                g[k] = np.float32(np.nan)
        return g
    out = _judge("fp32 evaluation", got(), ref64, ref32)
    assert out["dice"] == 1.0 and out["grad"] == 1.0 and out["loss"] <= 1.0
    for poison in (dict(loss=()), dict(dice=(1, 2)), dict(ga=(0, 3, 7)), dict(gb=(1, 0, 39)), dict(gb=slice(None))):
        with pytest.raises(AssertionError, match="not finite"):
            _judge("poisoned", got(**poison), ref64, ref32)
    wrong = got()
    wrong["gb"][1, 2, 5] += 1e-4 * np.abs(ref64[3][1]).max()
    with pytest.raises(AssertionError, match="x the yardstick"):
        _judge("wrong", wrong, ref64, ref32)
    z = rng.normal(size=(2, 4, 30)).astype(np.float32).astype(np.float64)
    y = rng.randint(0, 4, size=(2, 30))
    r64, r32 = loss_ref.dice_ce(z, y), loss_ref.dice_ce(z, y, dtype=np.float32)
    flat = lambda r: (np.array(r[0], dtype=np.float64), r[1], r[2])
    for slot in range(3):
        loss = np.array(r32[0], dtype=np.float32)
        _judge("dice_ce", dict(loss=loss.copy(), dice=r32[1], g=r32[2]), flat(r64), flat(r32), grads=("g",))
        loss[slot] = np.nan
        with pytest.raises(AssertionError, match="not finite"):
            _judge("dice_ce", dict(loss=loss, dice=r32[1], g=r32[2]), flat(r64), flat(r32), grads=("g",))
    a, b = (rng.uniform(size=(2, 3, 50)).astype(np.float32).astype(np.float64) for _ in range(2))
    gd = rng.normal(size=(2, 3))
    d, (ga, gb) = loss_ref.softdice_probs(a, b, dtype=np.float32), loss_ref.softdice_probs_grad(a, b, gd, dtype=np.float32)
    _probs_check("probs", a, b, gd, d, ga, gb)
    for k in range(3):
        bad = [d.copy(), ga.copy(), gb.copy()]
        bad[k].flat[-1] = np.nan
        with pytest.raises(AssertionError, match="not finite"):
            _probs_check("probs", a, b, gd, *bad)
