"""CPU: licenses tests/region_ref.py (the float64 restatement the region-kernel GPU tests compare with) against float64 torch
autograd of binary_cross_entropy_with_logits plus the Dice formula written with tensor operations on an EXPLICITLY BUILT region
target [B, R, V] - the tensor nnU-Net materialises and the kernels never do - and against the literal loop over
regions_class_order for the label map."""
import numpy as np
import pytest
import torch

import region_ref

REGIONS = ((1, 2, 3), (2, 3), (3,))          # nested, KiTS-like
TABLE = np.array([0b000, 0b001, 0b011, 0b111], dtype=np.uint32)


def _table(regions):
    from dg_tta_amd.labels import membership_table
    return membership_table(regions)


def _explicit_target(y, regions, L):
    """[B][R][V] float64 built region by region with isin, and the valid mask - no table involved."""
    valid = (y >= 0) & (y < L)
    t = np.stack([np.isin(y, list(r)) & valid for r in regions], axis=1).astype(np.float64)
    return t, valid


def _torch_loss(z, t, valid, smooth, batch_dice):
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    tt, vm = torch.tensor(t), torch.tensor(valid.astype(np.float64))[:, None, :]
    B, R, V = z.shape
    n = max(int(valid.sum()), 1)
    bce = (torch.nn.functional.binary_cross_entropy_with_logits(zt, tt, reduction="none") * vm).sum() / (n * R)
    s = torch.sigmoid(zt) * vm
    axes = (0, 2) if batch_dice else (2,)
    I, P, Y = (s * tt).sum(axes), s.sum(axes), tt.sum(axes)
    dice = (2 * I + smooth) / torch.clip(P + Y + smooth, 1e-8)
    loss = bce - dice.mean()
    loss.backward()
    return float(loss.detach()), float(bce.detach()), dice.detach().numpy(), zt.grad.numpy()


def _case(B, R, V, seed, regions=None):
    rng = np.random.RandomState(seed)
    regions = regions or tuple(tuple(sorted(rng.choice(np.arange(1, 7), size=rng.randint(1, 4), replace=False).tolist())) for _ in range(R))
    table = _table(regions)
    z = rng.standard_normal((B, R, V)) * 3
    y = rng.randint(0, table.size, size=(B, V)).astype(np.int64)
    y[0, ::7] = -1
    y[B - 1, 1::11] = table.size
    y[B - 1, 2::13] = -2 ** 40
    return z, y, regions, table


@pytest.mark.parametrize("batch_dice", [False, True])
@pytest.mark.parametrize("smooth", [1e-5, 0.0])
@pytest.mark.parametrize("B,R,V", [(3, 1, 50), (2, 3, 129), (1, 5, 40), (4, 8, 33)])
def test_loss_and_gradient_against_torch_autograd(B, R, V, smooth, batch_dice):
    z, y, regions, table = _case(B, R, V, seed=B * 100 + R * 10 + V)
    t, valid = _explicit_target(y, regions, table.size)
    loss, bce, dice, grad = _torch_loss(z, t, valid, smooth, batch_dice)
    (l0, l1, l2), d, g = region_ref.region_loss(z, y, table, smooth, batch_dice)
    assert abs(l0 - loss) <= 1e-13 * max(1.0, abs(loss)) and abs(l1 - bce) <= 1e-13 * max(1.0, abs(bce))
    assert abs(l0 - (l1 + l2)) <= 1e-15 * (abs(l0) + abs(l1) + abs(l2))
    np.testing.assert_allclose(d, np.broadcast_to(dice, d.shape), rtol=1e-12, atol=0)
    np.testing.assert_allclose(g, grad, rtol=1e-10, atol=1e-16 + 1e-12 * np.abs(grad).max())
    assert not g[~np.broadcast_to(valid[:, None, :], g.shape)].any()


def test_nested_table_is_the_kits_example():
    assert np.array_equal(_table(REGIONS), TABLE)
    t, valid = region_ref.region_target(np.array([[0, 1, 2, 3, 4, -1]]), TABLE, 3)
    assert valid.tolist() == [[True, True, True, True, False, False]]
    assert t[0].astype(int).tolist() == [[0, 1, 1, 1, 0, 0], [0, 0, 1, 1, 0, 0], [0, 0, 0, 1, 0, 0]]


@pytest.mark.parametrize("strides", [(2, 2, 2), (1, 2, 2), (3, 1, 2)])
@pytest.mark.parametrize("batch_dice", [False, True])
def test_strided_labels_are_the_sliced_label_map(strides, batch_dice):
    B, R, dims = 2, 3, (4, 3, 5)
    rng = np.random.RandomState(sum(strides))
    z = rng.standard_normal((B, R, *dims)) * 2
    full = rng.randint(-1, 5, size=(B, *(d * s for d, s in zip(dims, strides)))).astype(np.int64)
    low = np.ascontiguousarray(full[:, strides[0] // 2::strides[0], strides[1] // 2::strides[1], strides[2] // 2::strides[2]])
    assert low.shape[1:] == dims
    a = region_ref.region_loss(z, full, TABLE, 1e-5, batch_dice, strides)
    b = region_ref.region_loss(z.reshape(B, R, -1), low.reshape(B, -1), TABLE, 1e-5, batch_dice)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2].reshape(B, R, -1), b[2])
    t, valid = _explicit_target(low.reshape(B, -1), REGIONS, TABLE.size)
    loss, _, _, grad = _torch_loss(z.reshape(B, R, -1), t, valid, 1e-5, batch_dice)
    assert abs(a[0][0] - loss) <= 1e-13 and np.abs(a[2].reshape(B, R, -1) - grad).max() <= 1e-13


def test_invalid_voxels_change_nothing():
    """Dropping the invalid voxels from the arrays gives the same loss, dice and gradient on the rest."""
    z, y, regions, table = _case(1, 3, 90, seed=5)
    keep = (y[0] >= 0) & (y[0] < table.size)
    assert 0 < keep.sum() < keep.size
    a = region_ref.region_loss(z, y, table)
    b = region_ref.region_loss(z[:, :, keep], y[:, keep], table)
    assert abs(a[0][0] - b[0][0]) <= 1e-14 and np.abs(a[1] - b[1]).max() <= 1e-14
    assert np.abs(a[2][:, :, keep] - b[2]).max() <= 1e-16 and not a[2][:, :, ~keep].any()
    # and the logits of invalid voxels do not matter
    z2 = z.copy()
    z2[:, :, ~keep] = 55.0
    c = region_ref.region_loss(z2, y, table)
    assert c[0] == a[0] and np.array_equal(c[2], a[2])
    # no valid voxel at all: bce 0, gradient 0, dice = smooth / smooth
    d = region_ref.region_loss(z, np.full_like(y, -1), table)
    assert d[0][1] == 0.0 and d[0][0] == -1.0 and np.all(d[1] == 1.0) and not d[2].any()
    d0 = region_ref.region_loss(z, np.full_like(y, -1), table, smooth=0.0)
    assert d0[0] == (0.0, 0.0, 0.0) and not d0[2].any()


def test_single_label_region_has_target_y_equals_k():
    rng = np.random.RandomState(3)
    y = rng.randint(0, 5, size=(2, 60))
    for k in (1, 4):
        t, valid = region_ref.region_target(y, _table(((k,),)), 1)
        assert np.array_equal(t[:, 0], (y == k) & valid) and np.array_equal(valid, y <= k)


def test_float32_mode_is_float32_and_close():
    z, y, regions, table = _case(2, 3, 129, seed=9)
    r64 = region_ref.region_loss(z.astype(np.float32), y, table)
    r32 = region_ref.region_loss(z.astype(np.float32), y, table, dtype=np.float32)
    assert r32[1].dtype == np.float32 and r32[2].dtype == np.float32 and isinstance(r32[0][0], np.float32)
    assert abs(float(r32[0][0]) - r64[0][0]) < 1e-5 and np.abs(r32[2] - r64[2]).max() < 1e-6 * np.abs(r64[2]).max() + 1e-9


def test_counts_against_explicit_masks():
    z, y, regions, table = _case(3, 4, 200, seed=11)
    z = np.round(z * 4) / 4                                    # exact zeros among the logits: "not predicted"
    assert (z == 0).any()
    t, valid = _explicit_target(y, regions, table.size)
    pred = (z > 0) & valid[:, None, :]
    want = np.stack([(pred & (t > 0)).sum((0, 2)), (pred & (t == 0)).sum((0, 2)), (~pred & (t > 0)).sum((0, 2))])
    got = region_ref.region_counts(z, y, table)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(got[0] + got[2], t.sum((0, 2)).astype(np.int64))


@pytest.mark.parametrize("order", [[1, 2, 3], [2, 7, 1], [4, 4, 9]])
def test_label_map_is_the_literal_loop(order):
    rng = np.random.RandomState(sum(order))
    lg = np.round(rng.standard_normal((6, 5, 4, 3)) * 2) / 2   # exact zeros included
    assert (lg == 0).any()
    want = np.zeros(lg.shape[:3], dtype=np.int64)
    for idx in np.ndindex(*lg.shape[:3]):
        seg = 0
        for i, c in enumerate(order):
            if lg[idx][i] > 0:
                seg = c
        want[idx] = seg
    assert np.array_equal(region_ref.region_label_map(lg, order), want)
    assert np.array_equal(region_ref.region_label_map(lg * 7.5, order), want)      # any positive multiple
