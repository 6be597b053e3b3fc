"""Numpy restatements of the two loss kernels, float64 by default:

  softdice, softdice_probs(_grad)   csrc/softdice.hip (the masked-softmax soft-Dice consistency loss and the stand-alone
                                    soft_dice_loss on probability maps)
  dice_ce                           csrc/dice_ce.hip (nnU-Net's DC+CE pre-training loss, plain and deep-supervision form)

Arrays are class-major [B][C][V] here (the kernels' memory is voxel-major [B][V][ldc]: the tests transpose).  Every function
takes `dtype`: np.float64 is the reference, np.float32 evaluates THE SAME formula in fp32 on the CPU - the error of that
evaluation against float64 is the yardstick tests/test_gpu_loss.py measures the kernels with.
tests/test_loss_ref.py licenses the float64 form against float64 torch autograd of the oracle."""
import numpy as np


def _softmax(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def softdice(la, lb, start_class=1, guard_items=None, dtype=np.float64):
    """The header of softdice.hip:
        mask = (sum_c la > 0) * (sum_c lb > 0);  a = softmax_c(la) * mask;  b = softmax_c(lb) * mask
        nom = mean_v 2ab;  den = 0.5 mean_v (a + b)^2;  dice = nom / den
        per group of `guard_items` batch items (default: the whole batch): den sums to exactly 0 -> dice 1, gradient 0
        loss = 1 - mean_{b, c >= start_class} dice
    and the closed-form gradient of the loss with the per-class coefficients of the finalize kernel,
        P = -invN 2 / (V den),  Q = invN nom / (V den^2),  invN = 1 / (B (C - start_class))     (0 below start_class)
        dL/da = P b + Q (a + b),  dL/dla = mask pa (dL/da - sum_c dL/da pa)                     (pa: unmasked softmax)
    Returns (loss, dice [B][C], grad_la, grad_lb)."""
    la, lb = np.asarray(la, dtype=dtype), np.asarray(lb, dtype=dtype)
    B, C, V = la.shape
    guard_items = B if not guard_items else int(guard_items)
    assert B % guard_items == 0 and 0 <= start_class < C
    m = ((la.sum(axis=1) > 0) & (lb.sum(axis=1) > 0)).astype(dtype)[:, None, :]
    pa, pb = _softmax(la), _softmax(lb)
    a, b = pa * m, pb * m
    nom = (dtype(2) * a * b).mean(axis=2, dtype=dtype)
    den = dtype(0.5) * ((a + b) ** 2).mean(axis=2, dtype=dtype)
    flag = np.repeat(den.reshape(B // guard_items, -1).sum(axis=1) == 0, guard_items)[:, None]          # [B][1]
    on = ~flag & (np.arange(C) >= start_class)[None, :]
    inv_n = dtype(1) / dtype(B * (C - start_class))
    with np.errstate(divide="ignore", invalid="ignore"):
        dice = np.where(flag, dtype(1), nom / den)
        P = np.where(on, -inv_n * dtype(2) / (dtype(V) * den), dtype(0)).astype(dtype)[:, :, None]
        Q = np.where(on, inv_n * nom / (den * den * dtype(V)), dtype(0)).astype(dtype)[:, :, None]
    loss = dtype(1) - dice[:, start_class:].mean(dtype=dtype)
    with np.errstate(invalid="ignore"):                  # den = 0 outside a guarded group: 0 / 0, as in the oracle
        t = Q * (a + b)
        Ga, Gb = P * b + t, P * a + t
        ga = m * pa * (Ga - (Ga * pa).sum(axis=1, keepdims=True))
        gb = m * pb * (Gb - (Gb * pb).sum(axis=1, keepdims=True))
    return dtype(loss), dice.astype(dtype), ga, gb


def softdice_probs(a, b, dtype=np.float64):
    """soft_dice_loss(a, b) of the oracle on probability maps [B][C][V] -> dice [B][C]; the guard is over the whole call."""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    nom = (dtype(2) * a * b).mean(axis=2, dtype=dtype)
    den = dtype(0.5) * ((a + b) ** 2).mean(axis=2, dtype=dtype)
    if den.sum() == 0:
        return np.ones_like(nom)
    with np.errstate(divide="ignore", invalid="ignore"):
        return nom / den


def softdice_probs_grad(a, b, gdice, dtype=np.float64):
    """(grad_a, grad_b) of sum(dice * gdice): d dice / d a_v = 2 b_v / (V den) - nom (a_v + b_v) / (V den^2), a <-> b."""
    a, b, gdice = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype), np.asarray(gdice, dtype=dtype)
    V = a.shape[2]
    nom = (dtype(2) * a * b).mean(axis=2, dtype=dtype)
    den = dtype(0.5) * ((a + b) ** 2).mean(axis=2, dtype=dtype)
    if den.sum() == 0:
        return np.zeros_like(a), np.zeros_like(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        P = (gdice * dtype(2) / (dtype(V) * den))[:, :, None]
        Q = (-gdice * nom / (den * den * dtype(V)))[:, :, None]
    t = Q * (a + b)
    return P * b + t, P * a + t


def strided_labels(labels, strides):
    """labels [B][D][H][W] -> [B][D/sd][H/sh][W/sw]: low-resolution voxel (i, j, k) reads
    labels[i sd + sd // 2, j sh + sh // 2, k sw + sw // 2] (index arithmetic, as the kernel does it)."""
    labels = np.asarray(labels)
    sd, sh, sw = strides
    _, D, H, W = labels.shape
    assert D % sd == 0 and H % sh == 0 and W % sw == 0
    i = np.arange(D // sd) * sd + sd // 2
    j = np.arange(H // sh) * sh + sh // 2
    k = np.arange(W // sw) * sw + sw // 2
    return labels[:, i[:, None, None], j[None, :, None], k[None, None, :]]


def dice_ce(logits, labels, smooth=1e-5, do_bg=False, strides=(1, 1, 1), dtype=np.float64):
    """The header of dice_ce.hip.  logits [B][C][V] (or [B][C][d][h][w]); labels integer [B][V], or - with strides - the
    full-resolution map [B][d sd][h sh][w sw].  Labels outside [0, C) are ignored; N = valid voxels of the batch (1 if none):
        ce = -(1/N) sum_v log p[y_v];  dice_bc = (2 sum p y + smooth) / max(sum p + sum y + smooth, 1e-8)
        loss = ce - mean_{b, c >= first} dice,   first = 0 (do_bg) or 1
    Returns ((loss, ce, -mean dice), dice [B][C], grad_logits (shaped like logits))."""
    logits = np.asarray(logits, dtype=dtype)
    shape = logits.shape
    B, C = shape[:2]
    if tuple(strides) != (1, 1, 1):
        labels = strided_labels(labels, strides)
    z = logits.reshape(B, C, -1)
    y = np.asarray(labels).reshape(B, -1)
    V = z.shape[2]
    assert y.shape[1] == V
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
    I, P, Y = (pm * oh).sum(axis=2, dtype=dtype), pm.sum(axis=2, dtype=dtype), oh.sum(axis=2, dtype=dtype)
    s = dtype(smooth)
    num = dtype(2) * I + s
    D = np.maximum(P + Y + s, dtype(1e-8))
    dice = num / D
    first = 0 if do_bg else 1
    w = dtype(1) / dtype(B * (C - first))
    dl = -dice[:, first:].sum(dtype=dtype) * w
    on = (np.arange(C) >= first)[None, :]
    alpha = np.where(on, -dtype(2) * w / D, dtype(0)).astype(dtype)[:, :, None]
    beta = np.where(on, w * num / (D * D), dtype(0)).astype(dtype)[:, :, None]
    gp = alpha * oh + beta
    S = (p * gp).sum(axis=1, keepdims=True)
    grad = vm * ((p - oh) / n_valid + p * (gp - S))
    return (dtype(ce + dl), dtype(ce), dtype(dl)), dice, grad.reshape(shape)
