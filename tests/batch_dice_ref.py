"""Numpy restatement of the batch mode of csrc/dice_ce.hip (dgtta_dice_ce_batch_fwd / dgtta_dice_ce_ds_batch_fwd with batch_dice = 1),
float64 by default; tests/loss_ref.py::dice_ce is the per-sample mode.  With p = softmax(z), y the one-hot label, s = smooth and the
sums over the valid voxels (label in [0, C)) of ALL samples:

    I_c = sum_b sum_v p y      P_c = sum_b sum_v p      Y_c = sum_b sum_v y
    dc_c = (2 I_c + s) / max(P_c + Y_c + s, 1e-8)
    loss = ce - mean_{c >= first} dc_c          (ce: mean over all valid voxels of the batch, as in the per-sample mode)

- nnU-Net's MemoryEfficientSoftDiceLoss(batch_dice=True, do_bg=False, smooth=1e-5) inside DC_and_CE_loss, restated from memory of
nnunetv2 2.2.1: UNPINNED.  Arrays are class-major [B][C][V], as in loss_ref.  `dtype`: np.float64 is the reference, np.float32
evaluates THE SAME formula in fp32 on the CPU - the yardstick tests/test_gpu_batch_dice.py measures the kernels with.
tests/test_batch_dice_ref.py pins the float64 form to float64 torch autograd."""
import numpy as np

import loss_ref


def dice_ce_batch(logits, labels, smooth=1e-5, do_bg=False, strides=(1, 1, 1), dtype=np.float64):
    """logits [B][C][V] (or [B][C][d][h][w]); labels integer [B][V], or - with strides - the full-resolution map
    [B][d sd][h sh][w sw] read through loss_ref.strided_labels.  The gradient is the closed form of the kernels, with
    w = 1 / (C - first):  alpha_c = -2 w / D_c,  beta_c = w N_c / D_c^2  (0 below first; the same pair for every b),
        dL/dp[b][c][v] = alpha_c [y_v == c] + beta_c,   dL/dz = valid ((p - y) / N + p (dL/dp - sum_c p dL/dp)).
    Returns ((loss, ce, -mean dice), dice [B][C] - every row the same -, grad_logits (shaped like logits))."""
    logits = np.asarray(logits, dtype=dtype)
    shape = logits.shape
    B, C = shape[:2]
    if tuple(strides) != (1, 1, 1):
        labels = loss_ref.strided_labels(labels, strides)
    z = logits.reshape(B, C, -1)
    y = np.asarray(labels).reshape(B, -1)
    assert y.shape[1] == z.shape[2]
    valid = (y >= 0) & (y < C)
    safe = np.where(valid, y, 0)
    zs = z - z.max(axis=1, keepdims=True)
    e = np.exp(zs)
    se = e.sum(axis=1, keepdims=True)
    p = e / se
    vm = valid.astype(dtype)[:, None, :]
    oh = (np.arange(C)[None, :, None] == safe[:, None, :]).astype(dtype) * vm
    n_valid = dtype(max(int(valid.sum()), 1))
    nlp = np.log(se) - (zs * oh).sum(axis=1, keepdims=True)               # -log p[y] on valid voxels
    ce = (nlp * vm).sum(dtype=dtype) / n_valid
    pm = p * vm
    I, P, Y = ((x.sum(axis=2, dtype=dtype)).sum(axis=0, dtype=dtype) for x in (pm * oh, pm, oh))          # [C]: over v, then over b
    s = dtype(smooth)
    num = dtype(2) * I + s
    D = np.maximum(P + Y + s, dtype(1e-8))
    dice = num / D
    first = 0 if do_bg else 1
    w = dtype(1) / dtype(C - first)
    dl = -dice[first:].sum(dtype=dtype) * w
    on = np.arange(C) >= first
    alpha = np.where(on, -dtype(2) * w / D, dtype(0)).astype(dtype)[None, :, None]
    beta = np.where(on, w * num / (D * D), dtype(0)).astype(dtype)[None, :, None]
    gp = alpha * oh + beta
    S = (p * gp).sum(axis=1, keepdims=True)
    grad = vm * ((p - oh) / n_valid + p * (gp - S))
    return (dtype(ce + dl), dtype(ce), dtype(dl)), np.repeat(dice[None], B, axis=0), grad.reshape(shape)
