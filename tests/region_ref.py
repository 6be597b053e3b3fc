"""Numpy restatement of the region-based kernels (csrc/region_loss.hip, csrc/region_map.hip, the region label map of
csrc/window_features.hip), float64 by default:

  region_target      t[b][r][v] = bit r of table[y_bv] on valid voxels (0 <= y < L), and the valid mask
  region_loss        DC+BCE: loss, dice, gradient; batch Dice; strided labels (deep supervision)
  region_counts      TP / FP / FN per region of the hard prediction z > 0
  region_label_map   seg = 0; seg[l_i > 0] = order[i] for i = 0 .. R-1 in order

Arrays are region-major [B][R][V] here (the kernels' memory is voxel-major [B][V][ldc]: the tests transpose).  `dtype`:
np.float64 is the reference, np.float32 evaluates THE SAME formula in fp32 on the CPU - the error of that evaluation against
float64 is the yardstick tests/test_gpu_region_loss.py measures the kernels with.  tests/test_region_ref.py licenses the
float64 form against float64 torch autograd on an explicitly built region target."""
import numpy as np

from loss_ref import strided_labels


def region_target(labels, table, R):
    """labels integer [B][V] -> (t [B][R][V] of 0 / 1 (bool), valid [B][V]): a voxel is valid when 0 <= y < len(table)."""
    y = np.asarray(labels)
    table = np.asarray(table, dtype=np.uint32)
    valid = (y >= 0) & (y < table.size)
    bits = table[np.where(valid, y, 0)] * valid.astype(np.uint32)
    t = ((bits[:, None, :] >> np.arange(R, dtype=np.uint32)[None, :, None]) & np.uint32(1)).astype(bool)
    return t, valid


def region_loss(logits, labels, table, smooth=1e-5, batch_dice=False, strides=(1, 1, 1), dtype=np.float64):
    """The header of region_loss.hip.  logits [B][R][V] (or [B][R][d][h][w]); labels integer [B][V], or - with strides - the
    full-resolution map [B][d sd][h sh][w sw].  N = valid voxels of the batch (1 if none):
        bce = (1 / (N R)) sum_{valid v, r} [max(z, 0) - t z + log1p(exp(-|z|))]
        dice_br = (2 sum s t + smooth) / max(sum s + sum t + smooth, 1e-8)      (batch_dice: the sums pooled over b first)
        loss = bce - mean dice
        dL/dz = (s - t) / (N R) + s (1 - s) (alpha t + beta),  alpha = -2 w / D,  beta = w (2 I + smooth) / D^2 (0 where D was
        clamped),  w = 1 / (B R) or 1 / R
    Returns ((loss, bce, -mean dice), dice [B][R], grad_logits (shaped like logits))."""
    logits = np.asarray(logits, dtype=dtype)
    shape = logits.shape
    B, R = shape[:2]
    if tuple(strides) != (1, 1, 1):
        labels = strided_labels(labels, strides)
    z = logits.reshape(B, R, -1)
    y = np.asarray(labels).reshape(B, -1)
    assert y.shape[1] == z.shape[2]
    tb, valid = region_target(y, table, R)
    t, vm = tb.astype(dtype), valid.astype(dtype)[:, None, :]
    e = np.exp(-np.abs(z))
    inv = dtype(1) / (dtype(1) + e)
    s = np.where(z >= 0, inv, e * inv)
    ds = e * inv * inv
    n_r = dtype(max(int(valid.sum()), 1) * R)
    bce = ((np.maximum(z, dtype(0)) - t * z + np.log1p(e)) * vm).sum(dtype=dtype) / n_r
    sm = s * vm
    I, P, Y = (sm * t).sum(axis=2, dtype=dtype), sm.sum(axis=2, dtype=dtype), t.sum(axis=2, dtype=dtype)
    if batch_dice:
        I, P, Y = (np.broadcast_to(a.sum(axis=0, keepdims=True, dtype=dtype), (B, R)) for a in (I, P, Y))
    sc = dtype(smooth)
    num = dtype(2) * I + sc
    D0 = P + Y + sc
    D = np.maximum(D0, dtype(1e-8))
    dice = num / D
    w = dtype(1) / dtype((1 if batch_dice else B) * R)
    dl = -(dice[0] if batch_dice else dice).sum(dtype=dtype) * w
    alpha = (-dtype(2) * w / D).astype(dtype)[:, :, None]
    beta = np.where(D0 < dtype(1e-8), dtype(0), w * num / (D * D)).astype(dtype)[:, :, None]
    grad = vm * ((s - t) / n_r + ds * (alpha * t + beta))
    return (dtype(bce + dl), dtype(bce), dtype(dl)), dice.astype(dtype), grad.reshape(shape)


def region_counts(logits, labels, table):
    """int64 [3][R] = TP, FP, FN of (z > 0) against the region targets over valid voxels; logits [B][R][V], labels [B][V]."""
    z = np.asarray(logits)
    B, R = z.shape[:2]
    z = z.reshape(B, R, -1)
    t, valid = region_target(np.asarray(labels).reshape(B, -1), table, R)
    pred = (z > 0) & valid[:, None, :]
    return np.stack([(pred & t).sum(axis=(0, 2)), (pred & ~t).sum(axis=(0, 2)), (~pred & t).sum(axis=(0, 2))]).astype(np.int64)


def region_label_map(logits, order):
    """logits [..., R] (any positive multiple of the ensemble-mean logits) -> int64 [...]: 0, then order[i] where output i > 0,
    i ascending - the last positive region in the order wins; exactly 0 is not in the region."""
    lg = np.asarray(logits)
    seg = np.zeros(lg.shape[:-1], dtype=np.int64)
    for i, lab in enumerate(order):
        seg[lg[..., i] > 0] = int(lab)
    return seg
