"""Tensor-level wrappers over the C ABI (include/dgtta.h).  PyTorch is used for device memory, streams and autograd
glue only; every number is produced by the HIP kernels in dg_tta_amd/csrc.  All functions require CUDA(HIP) tensors.

Channel-last convention: a logical [B,C,D,H,W] tensor whose memory is [B,D,H,W,C] is exactly PyTorch's
`torch.channels_last_3d`; kernels that work voxel-major return such tensors, so callers keep NCDHW semantics.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import check, ptr, require_cuda, stream_of

F32, BF16, F16 = 0, 1, 2
C_int = C.c_int      # (functions with a class count `C` of their own)


def dtype_code(torch_dtype):
    """DGTTA_F32 / DGTTA_BF16 / DGTTA_F16 of a torch storage dtype."""
    try:
        return {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}[torch_dtype]
    except KeyError:
        raise ValueError(f"unsupported activation dtype {torch_dtype}") from None
PAD_ZEROS, PAD_BORDER = 0, 1
LINEAR, NEAREST = 0, 1


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _f32c(t):
    return t.contiguous().float() if (t.dtype != torch.float32 or not t.is_contiguous()) else t


def is_cl3d(t):
    """True when a 5-D tensor's memory is dense [B,D,H,W,C]."""
    return t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d)


def empty_cl3d(b, c, d, h, w, dtype, device):
    return torch.empty((b, d, h, w, c), dtype=dtype, device=device).permute(0, 4, 1, 2, 3)


# ------------------------------------------------------------------------------------------------ MIND
def gauss_taps(sigma):
    """The smoothing kernel exactly as the reference evaluates it (mind.py:30-37, fp32 on the CPU)."""
    s = torch.tensor([float(sigma)])
    n = int(torch.ceil(s * 3.0 / 2.0).long().item()) * 2 + 1
    w = torch.exp(-torch.pow(torch.linspace(-(n // 2), n // 2, n), 2) / (2 * torch.pow(s, 2)))
    return (w / w.sum()).tolist()


def _u64(x):
    return int(x) & 0xFFFFFFFFFFFFFFFF


def mind3d_noise(b, d, h, w, seed, offset=0, b0=0, device="cuda"):
    """The seeded MIND noise field [b,12,d,h,w] (fp32) of include/dgtta.h: Philox4x32-10 on (voxel, sample b0 + i, channel
    group, offset) under the key `seed`, Box-Muller.  What mind3d(img, seed=...) generates inside its kernel."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.DgttaError("dg_tta_amd ops run on the MI355X only: mind3d_noise got a CPU device (there is no CPU fallback)")
    lib = _lib.load()
    out = torch.empty((b, 12, d, h, w), dtype=torch.float32, device=device)
    check(lib.dgtta_mind3d_noise_fill(ptr(out), _u64(seed), _u64(offset), int(b0), b, d, h, w, stream_of(out.device)),
          "dgtta_mind3d_noise_fill")
    return out


def mind3d(img, noise=None, randn_weighting=0.05, out_format="ncdhw", out_ldc=12, out_dtype=torch.float32, groups=1, delta=1,
           sigma=1.0, seed=None, offset=0, b0=0):
    """MIND3D descriptor of img [B,1,D,H,W] (reference: dg_tta/mind.py:142-164) with exactly one of
    `noise` [B,12,D,H,W], the randn draw of mind.py:150 as a tensor, or
    `seed` (with `offset`, `b0`): the counter-based noise of mind3d_noise(B, D, H, W, seed, offset, b0), generated inside the
    kernel - no noise tensor, no generator state.

    out_format 'ncdhw' -> contiguous [B,12,D,H,W] fp32; 'ndhwc' -> raw [B,D,H,W,out_ldc] buffer (fp32 or bf16).
    groups > 1: the batch is `groups` independent calls of B/groups samples (the variance clamp of mind.py:159-161
    uses the mean over the whole call's batch), written into one output buffer; group g of a seeded call starts at sample
    b0 + g B/groups, so the grouping does not change a sample's noise.
    """
    if (noise is None) == (seed is None):
        raise ValueError("mind3d takes exactly one of `noise` (a tensor) and `seed` (in-kernel noise)")
    require_cuda(img, noise)
    lib = _lib.load()
    b, c, d, h, w = img.shape
    assert c == 1 and (noise is None or tuple(noise.shape) == (b, 12, d, h, w))
    img = _f32c(img)
    if noise is not None:
        noise = _f32c(noise)
    ndhwc = out_format == "ndhwc"
    if ndhwc:
        out = torch.empty((b, d, h, w, out_ldc), dtype=out_dtype, device=img.device)
    else:
        out = torch.empty((b, 12, d, h, w), dtype=torch.float32, device=img.device)
    assert b % groups == 0
    bg = b // groups
    nbytes = lib.dgtta_mind3d_ws_bytes(bg, d, h, w)
    ws = _ws(nbytes, img.device)
    taps = gauss_taps(sigma)
    h_taps = (C.c_float * len(taps))(*taps)
    for g in range(groups):
        sl = slice(g * bg, (g + 1) * bg)
        tail = (float(randn_weighting), int(delta), h_taps, len(taps), ptr(out[sl]), int(ndhwc), int(out_ldc),
                dtype_code(out_dtype), ptr(ws), nbytes, bg, d, h, w, stream_of(img.device))
        if noise is not None:
            check(lib.dgtta_mind3d_fwd(ptr(img[sl]), ptr(noise[sl]), *tail), "dgtta_mind3d_fwd")
        else:
            check(lib.dgtta_mind3d_fwd_seeded(ptr(img[sl]), _u64(seed), _u64(offset), int(b0) + g * bg, *tail),
                  "dgtta_mind3d_fwd_seeded")
    return out


# ------------------------------------------------------------------------------------------------ GIN
def gin_chain(x, alpha, ks, kers, shifts):
    """GIN chain on x [B,1,D,H,W] with explicit draws (reference: dg_tta/gin.py:168-230)."""
    require_cuda(x, alpha, *kers, *shifts)
    lib = _lib.load()
    b, c, d, h, w = x.shape
    assert c == 1 and len(ks) == len(kers) == len(shifts) == 4
    x = _f32c(x)
    alpha = _f32c(alpha)
    kers = [_f32c(k) for k in kers]
    shifts = [_f32c(s) for s in shifts]
    out = torch.empty_like(x)
    nbytes = lib.dgtta_gin_ws_bytes(b, d, h, w)
    ws = _ws(nbytes, x.device)
    ksz = (C.c_int * 4)(*[int(k) for k in ks])
    kp = (C.c_void_p * 4)(*[k.data_ptr() for k in kers])
    sp = (C.c_void_p * 4)(*[s.data_ptr() for s in shifts])
    check(lib.dgtta_gin_chain_fwd(ptr(x), ptr(alpha), ksz, kp, sp, ptr(out), ptr(ws), nbytes, b, d, h, w,
                                  stream_of(x.device)), "dgtta_gin_chain_fwd")
    return out


# ------------------------------------------------------------------------------------------------ warp
def _warp_layout(t):
    """(tensor to pass, ndhwc flag, ldc)."""
    if is_cl3d(t) and t.shape[1] > 1:
        return t, 1, t.shape[1]
    t = t.contiguous()
    return t, 0, 0


def _warp_fwd_raw(src, theta, out_size, pad_mode, interp, algebra, sub_const):
    lib = _lib.load()
    b, c, ds, hs, wsz = src.shape
    dd, hd, wd = out_size
    src, ndhwc, ldc = _warp_layout(src)
    dst = empty_cl3d(b, c, dd, hd, wd, torch.float32, src.device) if ndhwc else \
        torch.empty((b, c, dd, hd, wd), dtype=torch.float32, device=src.device)
    check(lib.dgtta_affine_warp3d_fwd(ptr(src), ptr(theta), ptr(dst), b, c, ds, hs, wsz, dd, hd, wd, ndhwc, ldc, ldc,
                                      pad_mode, interp, int(algebra), ptr(sub_const), stream_of(src.device)),
          "dgtta_affine_warp3d_fwd")
    return dst


class _AffineWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, theta, out_size, pad_mode, algebra):
        ctx.save_for_backward(theta)
        ctx.meta = (tuple(src.shape), tuple(out_size), pad_mode, algebra, is_cl3d(src) and src.shape[1] > 1)
        return _warp_fwd_raw(src, theta, out_size, pad_mode, LINEAR, algebra, None)

    @staticmethod
    def backward(ctx, grad):
        (theta,) = ctx.saved_tensors
        shape, out_size, pad_mode, algebra, ndhwc = ctx.meta
        lib = _lib.load()
        b, c, ds, hs, wsz = shape
        dd, hd, wd = out_size
        if ndhwc:
            grad = grad.contiguous(memory_format=torch.channels_last_3d)
            gsrc = torch.empty((b, ds, hs, wsz, c), dtype=torch.float32, device=grad.device).permute(0, 4, 1, 2, 3)
        else:
            grad = grad.contiguous()
            gsrc = torch.empty(shape, dtype=torch.float32, device=grad.device)
        check(lib.dgtta_affine_warp3d_bwd(ptr(grad), ptr(theta), ptr(gsrc), b, c, ds, hs, wsz, dd, hd, wd, int(ndhwc), c,
                                          c, pad_mode, int(algebra), stream_of(grad.device)), "dgtta_affine_warp3d_bwd")
        return gsrc, None, None, None, None


def affine_warp(src, theta, out_size=None, padding_mode="zeros", tta_grid_algebra=False):
    """F.grid_sample(src, F.affine_grid(theta, ...), align_corners=False) (reference call sites tta.py:523-551,572-575).

    src [B,C,D,H,W] fp32 (contiguous or channels_last_3d; the layout is preserved), theta [B,3,4].
    Differentiable w.r.t. src (theta is a constant, as in the reference)."""
    require_cuda(src, theta)
    theta = _f32c(theta)
    src = src if src.dtype == torch.float32 else src.float()
    out_size = tuple(src.shape[2:]) if out_size is None else tuple(out_size)
    pad = PAD_BORDER if padding_mode == "border" else PAD_ZEROS
    return _AffineWarp.apply(src, theta, out_size, pad, bool(tta_grid_algebra))


def affine_sample(src, theta, out_size, padding_mode="zeros", mode="bilinear", sub_const=None):
    """Non-differentiable sampler with nearest mode and the (x - c) ... + c trick of get_batch (torch_utils.py:58-62)."""
    require_cuda(src, theta)
    pad = PAD_BORDER if padding_mode == "border" else PAD_ZEROS
    interp = NEAREST if mode == "nearest" else LINEAR
    return _warp_fwd_raw(src.float(), _f32c(theta), tuple(out_size), pad, interp, False, sub_const)


# ------------------------------------------------------------------------------------------------ deformable augmentation
def rf_field(draw, size_3d, box=5):
    """get_rf_field (augmentation_utils.py:8-43) from its torch.randn draw [B,F,D//k,H//k,W//k]: three `box`^3 mean filters,
    trilinear upsampling to size_3d, per (sample, field) zero mean and unit (1e-3 + std).  Returns [B,F,D,H,W] fp32."""
    require_cuda(draw)
    lib = _lib.load()
    b, f, dl, hl, wl = draw.shape
    d, h, w = (int(v) for v in size_3d)
    draw = _f32c(draw)
    field = torch.empty((b, f, d, h, w), dtype=torch.float32, device=draw.device)
    nbytes = lib.dgtta_rf_field_ws_bytes(b * f, dl, hl, wl)
    ws = _ws(nbytes, draw.device)
    check(lib.dgtta_rf_field_fwd(ptr(draw), ptr(field), ptr(ws), nbytes, b * f, int(box), dl, hl, wl, d, h, w,
                                 stream_of(draw.device)), "dgtta_rf_field_fwd")
    return field


def diffeo_fields(field, factor=1.0, time_steps=5):
    """calc_consistent_diffeomorphic_field(field * factor, zeros, time_steps, ensure_inverse_consistency=True)
    (augmentation_utils.py:46-135) of field [B,3,D,H,W].  Returns (disp, inverse) as contiguous [B,D,H,W,3]."""
    require_cuda(field)
    lib = _lib.load()
    b, c, d, h, w = field.shape
    assert c == 3
    field = _f32c(field)
    disp = torch.empty((b, d, h, w, 3), dtype=torch.float32, device=field.device)
    inverse = torch.empty_like(disp)
    nbytes = lib.dgtta_diffeo_fields_ws_bytes(b, d, h, w)
    ws = _ws(nbytes, field.device)
    check(lib.dgtta_diffeo_fields(ptr(field), float(factor), ptr(disp), ptr(inverse), ptr(ws), nbytes, b, d, h, w,
                                  int(time_steps), stream_of(field.device)), "dgtta_diffeo_fields")
    return disp, inverse


class _DenseWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, disp, pad_mode):
        lib = _lib.load()
        b, c, d, h, w = src.shape
        src, ndhwc, ldc = _warp_layout(src)
        dst = empty_cl3d(b, c, d, h, w, torch.float32, src.device) if ndhwc else torch.empty_like(src)
        check(lib.dgtta_dense_warp3d_fwd(ptr(src), ptr(disp), ptr(dst), b, c, d, h, w, ndhwc, ldc, ldc, pad_mode,
                                         stream_of(src.device)), "dgtta_dense_warp3d_fwd")
        ctx.save_for_backward(disp)
        ctx.meta = (tuple(src.shape), pad_mode, bool(ndhwc))
        return dst

    @staticmethod
    def backward(ctx, grad):
        (disp,) = ctx.saved_tensors
        (b, c, d, h, w), pad_mode, ndhwc = ctx.meta
        lib = _lib.load()
        if ndhwc:
            grad = grad.contiguous(memory_format=torch.channels_last_3d)
            gsrc = empty_cl3d(b, c, d, h, w, torch.float32, grad.device)
        else:
            grad = grad.contiguous()
            gsrc = torch.empty((b, c, d, h, w), dtype=torch.float32, device=grad.device)
        check(lib.dgtta_dense_warp3d_bwd(ptr(grad), ptr(disp), ptr(gsrc), b, c, d, h, w, int(ndhwc), c, c, pad_mode,
                                         stream_of(grad.device)), "dgtta_dense_warp3d_bwd")
        return gsrc, None, None


def dense_warp(src, disp, padding_mode="zeros"):
    """F.grid_sample(src, (0 * identity + disp) + identity, align_corners=False) with identity = F.affine_grid(eye): the
    deformable call sites of calc_branch (tta.py:534-551 image, border; :572-575 logits, zeros).

    src [B,C,D,H,W] fp32 (contiguous or channels_last_3d; the layout is preserved), disp [B,D,H,W,3] in (x, y, z) order.
    Differentiable w.r.t. src only (the fields are constants, as in the reference); that gradient is summed with fp32
    atomics, so its last bits vary from run to run."""
    require_cuda(src, disp)
    if tuple(disp.shape) != (src.shape[0], *src.shape[2:], 3):
        raise ValueError(f"dense_warp: disp {tuple(disp.shape)} does not belong to src {tuple(src.shape)}")
    src = src if src.dtype == torch.float32 else src.float()
    pad = PAD_BORDER if padding_mode == "border" else PAD_ZEROS
    return _DenseWarp.apply(src, _f32c(disp.detach()), pad)


# ------------------------------------------------------------------------------------------------ loss
class _ConsistencyLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, la, lb, start_class, guard_items=0):
        lib = _lib.load()
        b, c = la.shape[:2]
        v = la.shape[2] * la.shape[3] * la.shape[4]
        la = la.contiguous(memory_format=torch.channels_last_3d)
        lb = lb.contiguous(memory_format=torch.channels_last_3d)
        dice = torch.empty((b, c), dtype=torch.float32, device=la.device)
        loss = torch.empty((), dtype=torch.float32, device=la.device)
        nbytes = lib.dgtta_softdice_ws_bytes(b, c, v)
        ws = _ws(nbytes, la.device)
        check(lib.dgtta_softdice_fwd(ptr(la), ptr(lb), ptr(dice), ptr(loss), ptr(ws), nbytes, b, c, v, c, start_class,
                                     guard_items if guard_items else b, stream_of(la.device)), "dgtta_softdice_fwd")
        ctx.save_for_backward(la, lb, ws)
        ctx.meta = (b, c, v, start_class)
        ctx.mark_non_differentiable(dice)
        return loss, dice

    @staticmethod
    def backward(ctx, gloss, _gdice):
        la, lb, ws = ctx.saved_tensors
        b, c, v, start_class = ctx.meta
        lib = _lib.load()
        ga = torch.empty_like(la, memory_format=torch.preserve_format)
        gb = torch.empty_like(lb, memory_format=torch.preserve_format)
        # the upstream gradient (e.g. 1/patches_to_be_accumulated) is read on the device: no host sync, no torch math
        gs = gloss.reshape(1).float().contiguous()
        check(lib.dgtta_softdice_bwd(ptr(la), ptr(lb), ptr(ga), ptr(gb), ptr(ws), 1.0, ptr(gs), b, c, v, c, start_class,
                                     stream_of(la.device)), "dgtta_softdice_bwd")
        return ga, gb, None, None


class _ConsistencyLossPair(torch.autograd.Function):
    """Same loss on the two halves of ONE batched tensor [2B,C,D,H,W] (branch a = first half): the gradient comes back
    as one buffer, so autograd needs no slice-backward zero fills and adds."""

    @staticmethod
    def forward(ctx, both, start_class, guard_items):
        lib = _lib.load()
        # the producer's offer to take the gradient in its 16-bit storage type (unet.Grad16Sink; 16-class rows only)
        sink = getattr(both, "_dgtta_grad16", None)
        ctx.sink = sink if (sink is not None and both.shape[1] == 16 and sink.claim()) else None
        both = both.contiguous(memory_format=torch.channels_last_3d)
        b2, c = both.shape[:2]
        b = b2 // 2
        v = both.shape[2] * both.shape[3] * both.shape[4]
        la, lb = both[:b], both[b:]
        dice = torch.empty((b, c), dtype=torch.float32, device=both.device)
        loss = torch.empty((), dtype=torch.float32, device=both.device)
        nbytes = lib.dgtta_softdice_ws_bytes(b, c, v)
        ws = _ws(nbytes, both.device)
        check(lib.dgtta_softdice_fwd(ptr(la), ptr(lb), ptr(dice), ptr(loss), ptr(ws), nbytes, b, c, v, c, start_class,
                                     guard_items if guard_items else b, stream_of(both.device)), "dgtta_softdice_fwd")
        ctx.save_for_backward(both, ws)
        ctx.meta = (b, c, v, start_class)
        ctx.mark_non_differentiable(dice)
        return loss, dice

    @staticmethod
    def backward(ctx, gloss, _gdice):
        both, ws = ctx.saved_tensors
        b, c, v, start_class = ctx.meta
        lib = _lib.load()
        gs = gloss.reshape(1).float().contiguous()
        if ctx.sink is not None:
            # the gradient goes to the producer in ITS storage type through the sink; autograd gets a stride-0 placeholder
            g16 = torch.empty((2 * b, *both.shape[2:], c), dtype=ctx.sink.dtype, device=both.device)
            check(lib.dgtta_softdice_bwd_t(ptr(both[:b]), ptr(both[b:]), ptr(g16[:b]), ptr(g16[b:]), ptr(ws), 1.0, ptr(gs), b, c, v,
                                           c, start_class, dtype_code(ctx.sink.dtype), stream_of(both.device)), "dgtta_softdice_bwd_t")
            ctx.sink.put(g16)
            return torch.zeros((), dtype=both.dtype, device=both.device).expand(both.shape), None, None
        g = torch.empty_like(both, memory_format=torch.preserve_format)
        check(lib.dgtta_softdice_bwd(ptr(both[:b]), ptr(both[b:]), ptr(g[:b]), ptr(g[b:]), ptr(ws), 1.0, ptr(gs), b, c, v, c,
                                     start_class, stream_of(both.device)), "dgtta_softdice_bwd")
        return g, None, None


def consistency_loss(target_a, target_b, start_class=1):
    """tta.py:263-269: masked softmax of both branches + `1 - soft_dice[:, start_class:].mean()`. Returns (loss, dice[B,C]).
    Targets produced by tta.calc_both_branches carry their common batched tensor (`_dgtta_pair`): the loss is then taken
    on that tensor directly."""
    require_cuda(target_a, target_b)
    pair = getattr(target_a, "_dgtta_pair", None)
    if pair is not None and pair is getattr(target_b, "_dgtta_pair", None) and pair.dtype == torch.float32:
        return _ConsistencyLossPair.apply(pair, int(start_class), int(getattr(target_a, "_dgtta_guard_items", 0)))
    return _ConsistencyLoss.apply(target_a.float(), target_b.float(), int(start_class),
                                  int(getattr(target_a, "_dgtta_guard_items", 0)))


class _DiceCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, smooth, do_bg, batch_dice=False):
        lib = _lib.load()
        b, c = logits.shape[:2]
        v = logits[0, 0].numel()
        logits = logits.contiguous(memory_format=torch.channels_last_3d)
        labels = labels.reshape(b, v).contiguous()
        loss3 = torch.empty(3, dtype=torch.float32, device=logits.device)
        dice = torch.empty((b, c), dtype=torch.float32, device=logits.device)
        nbytes = lib.dgtta_dice_ce_ws_bytes(b, c, v)
        ws = _ws(nbytes, logits.device)
        if batch_dice:
            check(lib.dgtta_dice_ce_batch_fwd(ptr(logits), c, ptr(labels), ptr(loss3), ptr(dice), ptr(ws), nbytes, b, c, v, float(smooth),
                                              int(do_bg), 1, stream_of(logits.device)), "dgtta_dice_ce_batch_fwd")
        else:
            check(lib.dgtta_dice_ce_fwd(ptr(logits), c, ptr(labels), ptr(loss3), ptr(dice), ptr(ws), nbytes, b, c, v, float(smooth),
                                        int(do_bg), stream_of(logits.device)), "dgtta_dice_ce_fwd")
        ctx.save_for_backward(logits, labels, ws)
        ctx.meta = (b, c, v)
        ctx.mark_non_differentiable(dice)
        return loss3[0], dice, loss3[1:].detach()

    @staticmethod
    def backward(ctx, gloss, _gdice, _gparts):
        logits, labels, ws = ctx.saved_tensors
        b, c, v = ctx.meta
        lib = _lib.load()
        g = torch.empty_like(logits, memory_format=torch.preserve_format)
        gs = gloss.reshape(1).float().contiguous()
        check(lib.dgtta_dice_ce_bwd(ptr(logits), c, ptr(labels), ptr(ws), 1.0, ptr(gs), ptr(g), c, b, c, v,
                                    stream_of(logits.device)), "dgtta_dice_ce_bwd")
        return g, None, None, None, None


def dice_ce_loss(logits, labels, smooth=1e-5, do_bg=False, batch_dice=False):
    """nnU-Net's pre-training loss DC_and_CE_loss [3P] (soft Dice per sample without background + cross-entropy) of logits
    [B,C,D,H,W] (fp32) against an integer label map [B,1,D,H,W] / [B,D,H,W] (labels outside [0, C) are ignored).
    batch_dice: the plans' switch of that name - the Dice sums are pooled over the batch before the ratio (csrc/dice_ce.hip, from
    memory of nnU-Net's MemoryEfficientSoftDiceLoss, unpinned); every row of the returned dice then holds the class's one value.
    Returns (loss, dice [B,C], (ce, -mean dice)); differentiable w.r.t. the logits."""
    require_cuda(logits, labels)
    if labels.dtype != torch.int64:
        labels = labels.long()
    return _DiceCE.apply(logits.float(), labels, smooth, do_bg, bool(batch_dice))


class _DiceCEStrided(torch.autograd.Function):
    """DC+CE of low-resolution logits against a strided view of the full-resolution label map (csrc/dice_ce.hip, _ds)."""

    @staticmethod
    def forward(ctx, logits, labels, strides, smooth, do_bg, batch_dice=False):
        lib = _lib.load()
        b, c, d, h, w = logits.shape
        logits = logits.contiguous(memory_format=torch.channels_last_3d)
        labels = labels.contiguous()
        loss3 = torch.empty(3, dtype=torch.float32, device=logits.device)
        dice = torch.empty((b, c), dtype=torch.float32, device=logits.device)
        nbytes = lib.dgtta_dice_ce_ds_ws_bytes(b, c, d, h, w)
        ws = _ws(nbytes, logits.device)
        if batch_dice:
            check(lib.dgtta_dice_ce_ds_batch_fwd(ptr(logits), c, ptr(labels), ptr(loss3), ptr(dice), ptr(ws), nbytes, b, c, d, h, w,
                                                 *strides, float(smooth), int(do_bg), 1, stream_of(logits.device)),
                  "dgtta_dice_ce_ds_batch_fwd")
        else:
            check(lib.dgtta_dice_ce_ds_fwd(ptr(logits), c, ptr(labels), ptr(loss3), ptr(dice), ptr(ws), nbytes, b, c, d, h, w, *strides,
                                           float(smooth), int(do_bg), stream_of(logits.device)), "dgtta_dice_ce_ds_fwd")
        ctx.save_for_backward(logits, labels, ws)
        ctx.meta = (b, c, d, h, w, strides)
        ctx.mark_non_differentiable(dice)
        return loss3[0], dice, loss3[1:].detach()

    @staticmethod
    def backward(ctx, gloss, _gdice, _gparts):
        logits, labels, ws = ctx.saved_tensors
        b, c, d, h, w, strides = ctx.meta
        lib = _lib.load()
        g = torch.empty_like(logits, memory_format=torch.preserve_format)
        gs = gloss.reshape(1).float().contiguous()      # (carries the scale's weight of the multi-scale sum)
        check(lib.dgtta_dice_ce_ds_bwd(ptr(logits), c, ptr(labels), ptr(ws), 1.0, ptr(gs), ptr(g), c, b, c, d, h, w, *strides,
                                       stream_of(logits.device)), "dgtta_dice_ce_ds_bwd")
        return g, None, None, None, None, None


def deep_supervision_weights(n):
    """nnU-Net's weights of the multi-scale loss for n outputs (highest resolution first): 2^-i, the lowest resolution set to 0,
    normalised to sum 1 (5 outputs: [8/15, 4/15, 2/15, 1/15, 0]; one output: [1])."""
    w = [2.0 ** -i for i in range(n)]
    if n > 1:
        w[-1] = 0.0
    tot = sum(w)
    return [x / tot for x in w]


def _label_strides(out_shape, label_shape):
    strides = []
    for o, full in zip(out_shape, label_shape):
        if o <= 0 or full % o:
            raise ValueError(f"deep_supervision_loss: output {tuple(out_shape)} does not divide the label map {tuple(label_shape)}")
        strides.append(full // o)
    return tuple(strides)


def deep_supervision_loss(outputs, labels, smooth=1e-5, do_bg=False, weights=None, batch_dice=False):
    """nnU-Net's multi-scale loss (DeepSupervisionWrapper [3P] around DC_and_CE_loss): sum_i w_i * dice_ce(outputs[i], labels at
    the resolution of outputs[i]).  outputs: logits [B,C,d_i,h_i,w_i], highest resolution first (what HipPlainConvUNet returns
    with deep_supervision on); labels: the FULL-resolution integer map [B,1,D,H,W] / [B,D,H,W] - every output is compared
    with the strided view labels[i sd + sd/2, j sh + sh/2, k sw + sw/2] of it (csrc/dice_ce.hip; a restatement from memory of
    nnU-Net's DownsampleSegForDSTransform2, unpinned), no downsampled label map is built.  The strides follow from the shapes
    and must divide exactly (ValueError).  weights: default deep_supervision_weights(len(outputs)); a zero-weight scale is
    skipped in both directions.  batch_dice: every scale's Dice term pools its sums over the batch (dice_ce_loss).
    Returns (loss, [per-scale loss or None where skipped]); differentiable w.r.t. every output."""
    outputs = list(outputs)
    if labels.dim() == 5:
        labels = labels[:, 0]
    if weights is None:
        weights = deep_supervision_weights(len(outputs))
    if len(weights) != len(outputs):
        raise ValueError(f"deep_supervision_loss: {len(weights)} weights for {len(outputs)} outputs")
    strides = [_label_strides(o.shape[2:], labels.shape[1:]) for o in outputs]
    for o in outputs:
        if o.shape[0] != labels.shape[0]:
            raise ValueError("deep_supervision_loss: batch sizes of outputs and labels differ")
    require_cuda(labels, *outputs)
    if labels.dtype != torch.int64:
        labels = labels.long()
    total, per_scale = None, []
    for o, st, wgt in zip(outputs, strides, weights):
        if wgt == 0:
            per_scale.append(None)
            continue
        li, _, _ = _DiceCEStrided.apply(o.float(), labels, st, smooth, do_bg, bool(batch_dice))
        per_scale.append(li.detach())
        total = li * wgt if total is None else total + li * wgt
    if total is None:
        raise ValueError("deep_supervision_loss: every weight is zero")
    return total, per_scale


# ------------------------------------------------------------------------------------------------ region-based datasets
MAX_REGIONS, MAX_REGION_TABLE = 32, 1024


def region_table(table, device):
    """The membership table of dg_tta_amd.labels (uint32 [L]: bit r of entry y = label y belongs to region r) as an int32 device
    tensor holding the same bits (what the region kernels read)."""
    if isinstance(table, torch.Tensor):
        if table.dtype != torch.int32 or table.dim() != 1:
            raise ValueError("region table: a uint32 numpy array or a 1-D int32 tensor (the same bits) expected")
        t = table.to(device).contiguous()
    else:
        import numpy as np
        a = np.ascontiguousarray(np.asarray(table))
        if a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (a.min() < 0 or a.max() > 0xffffffff)):
            raise ValueError("region table: a 1-D array of 32-bit masks expected")
        t = torch.from_numpy(a.astype(np.uint32).view(np.int32)).to(device)
    if not 1 <= t.numel() <= MAX_REGION_TABLE:
        raise ValueError(f"region table: 1..{MAX_REGION_TABLE} label values expected, got {t.numel()}")
    return t


class _RegionLoss(torch.autograd.Function):
    """DC+BCE of region logits against an integer label map and the membership table (csrc/region_loss.hip); strides None: dense
    labels [B, V], else the full-resolution map read through the deep-supervision index map."""

    @staticmethod
    def forward(ctx, logits, labels, table, strides, smooth, batch_dice):
        lib = _lib.load()
        b, r, d, h, w = logits.shape
        logits = logits.contiguous(memory_format=torch.channels_last_3d)
        labels = labels.contiguous()
        dev, L = logits.device, table.numel()
        loss3 = torch.empty(3, dtype=torch.float32, device=dev)
        dice = torch.empty((b, r), dtype=torch.float32, device=dev)
        if strides is None:
            v = d * h * w
            nbytes = lib.dgtta_region_loss_ws_bytes(b, r, v)
            ws = _ws(nbytes, dev)
            check(lib.dgtta_region_loss_batch_fwd(ptr(logits), r, ptr(labels), ptr(table), L, ptr(loss3), ptr(dice), ptr(ws), nbytes, b, r, v,
                                                  float(smooth), int(batch_dice), stream_of(dev)), "dgtta_region_loss_batch_fwd")
        else:
            nbytes = lib.dgtta_region_loss_ds_ws_bytes(b, r, d, h, w)
            ws = _ws(nbytes, dev)
            check(lib.dgtta_region_loss_ds_batch_fwd(ptr(logits), r, ptr(labels), ptr(table), L, ptr(loss3), ptr(dice), ptr(ws), nbytes, b, r,
                                                     d, h, w, *strides, float(smooth), int(batch_dice), stream_of(dev)),
                  "dgtta_region_loss_ds_batch_fwd")
        ctx.save_for_backward(logits, labels, table, ws)
        ctx.meta = (b, r, d, h, w, strides)
        ctx.mark_non_differentiable(dice)
        return loss3[0], dice, loss3[1:].detach()

    @staticmethod
    def backward(ctx, gloss, _gdice, _gparts):
        logits, labels, table, ws = ctx.saved_tensors
        b, r, d, h, w, strides = ctx.meta
        lib = _lib.load()
        g = torch.empty_like(logits, memory_format=torch.preserve_format)
        gs = gloss.reshape(1).float().contiguous()      # (carries the scale's weight of the multi-scale sum)
        st = stream_of(logits.device)
        if strides is None:
            check(lib.dgtta_region_loss_bwd(ptr(logits), r, ptr(labels), ptr(table), table.numel(), ptr(ws), 1.0, ptr(gs), ptr(g), r, b, r,
                                            d * h * w, st), "dgtta_region_loss_bwd")
        else:
            check(lib.dgtta_region_loss_ds_bwd(ptr(logits), r, ptr(labels), ptr(table), table.numel(), ptr(ws), 1.0, ptr(gs), ptr(g), r, b, r,
                                               d, h, w, *strides, st), "dgtta_region_loss_ds_bwd")
        return g, None, None, None, None, None


def _region_logits(logits, name):
    if logits.dim() != 5 or not 1 <= logits.shape[1] <= MAX_REGIONS:
        raise ValueError(f"{name}: logits [B,R,D,H,W] with 1 <= R <= {MAX_REGIONS} expected, got {tuple(logits.shape)}")


def region_loss(logits, labels, table, smooth=1e-5, batch_dice=False):
    """nnU-Net's loss of region-based training, DC_and_BCE_loss [3P] (soft Dice per sample over all R regions + binary
    cross-entropy, csrc/region_loss.hip; from memory, unpinned): logits [B,R,D,H,W] (fp32, one sigmoid output per region) against
    an integer label map [B,1,D,H,W] / [B,D,H,W] and the membership `table` (dg_tta_amd.labels: uint32 [L], bit r of entry y = label
    y belongs to region r).  Labels outside [0, L) are ignored.  No region target tensor is built.  batch_dice: the Dice sums are
    pooled over the batch before the ratio.  Returns (loss, dice [B,R], (bce, -mean dice)); differentiable w.r.t. the logits."""
    require_cuda(logits, labels)
    _region_logits(logits, "region_loss")
    if labels.dtype != torch.int64:
        labels = labels.long()
    labels = labels.reshape(logits.shape[0], -1)
    if labels.shape[1] != logits[0, 0].numel():
        raise ValueError("region_loss: the label map does not have the logits' voxels")
    return _RegionLoss.apply(logits.float(), labels, region_table(table, logits.device), None, smooth, bool(batch_dice))


def deep_supervision_region_loss(outputs, labels, table, weights=None, batch_dice=False, smooth=1e-5):
    """deep_supervision_loss for a region head: sum_i w_i * region_loss(outputs[i], labels at the resolution of outputs[i]), every
    output compared with the strided view of the FULL-resolution label map (no downsampled map, no region target tensor).
    Returns (loss, [per-scale loss or None where skipped]); differentiable w.r.t. every output."""
    outputs = list(outputs)
    if labels.dim() == 5:
        labels = labels[:, 0]
    if weights is None:
        weights = deep_supervision_weights(len(outputs))
    if len(weights) != len(outputs):
        raise ValueError(f"deep_supervision_region_loss: {len(weights)} weights for {len(outputs)} outputs")
    strides = [_label_strides(o.shape[2:], labels.shape[1:]) for o in outputs]
    for o in outputs:
        _region_logits(o, "deep_supervision_region_loss")
        if o.shape[0] != labels.shape[0]:
            raise ValueError("deep_supervision_region_loss: batch sizes of outputs and labels differ")
    require_cuda(labels, *outputs)
    if labels.dtype != torch.int64:
        labels = labels.long()
    table = region_table(table, labels.device)
    total, per_scale = None, []
    for o, st, wgt in zip(outputs, strides, weights):
        if wgt == 0:
            per_scale.append(None)
            continue
        li, _, _ = _RegionLoss.apply(o.float(), labels, table, st, smooth, bool(batch_dice))
        per_scale.append(li.detach())
        total = li * wgt if total is None else total + li * wgt
    if total is None:
        raise ValueError("deep_supervision_region_loss: every weight is zero")
    return total, per_scale


def region_counts(logits, labels, table):
    """Per-region counts of the hard prediction logits > 0 (sigmoid > 0.5; exactly 0 is "not predicted") against the regions of
    an integer label map, over the voxels whose label lies inside the table: int64 [3, R] = TP, FP, FN - the online pseudo-Dice
    2 TP / (2 TP + FP + FN) of a region trainer (csrc/region_map.hip), what argmax_dice's counts are for the softmax case."""
    require_cuda(logits, labels)
    _region_logits(logits, "region_counts")
    lib = _lib.load()
    b, r = logits.shape[:2]
    lg = logits.float().contiguous(memory_format=torch.channels_last_3d)
    lb = labels.reshape(-1).to(torch.int64).contiguous()
    if lb.numel() != b * lg[0, 0].numel():
        raise ValueError("region_counts: the label map does not have the logits' voxels")
    table = region_table(table, lg.device)
    counts = torch.empty((3, r), dtype=torch.int64, device=lg.device)
    check(lib.dgtta_region_counts(ptr(lg), r, r, ptr(lb), ptr(table), table.numel(), ptr(counts), lb.numel(), stream_of(lg.device)),
          "dgtta_region_counts")
    return counts


def check_regions_class_order(order, num_regions):
    """`regions_class_order` as plain ints: one positive label per region.  ValueError otherwise (before anything touches the GPU)."""
    order = [int(x) for x in order]
    if len(order) != num_regions or not 1 <= num_regions <= MAX_REGIONS or min(order) <= 0:
        raise ValueError(f"regions_class_order: {num_regions} positive labels expected (1..{MAX_REGIONS} regions), got {order}")
    return order


def logits_regions(acc, order):
    """Label map of a voxel-major accumulator of region logits [..., R] (fp32 or fp16, contiguous): 0, then order[i] wherever
    output i is > 0, for i = 0 .. R-1 in order - the last positive region wins (csrc/region_map.hip; nnU-Net's
    convert_probabilities_to_segmentation for regions, from memory, unpinned).  int64."""
    require_cuda(acc)
    if acc.dtype not in (torch.float32, torch.float16) or not acc.is_contiguous():
        raise ValueError("logits_regions: contiguous fp32 / fp16 rows expected")
    order = check_regions_class_order(order, acc.shape[-1])
    lib = _lib.load()
    out = torch.empty(acc.shape[:-1], dtype=torch.int64, device=acc.device)
    check(lib.dgtta_logits_regions(ptr(acc), F32 if acc.dtype == torch.float32 else F16, len(order), out.numel(), (C_int * len(order))(*order),
                                   ptr(out), stream_of(acc.device)), "dgtta_logits_regions")
    return out


def feature_head_regions_supported(M, R):
    """dgtta_feature_head_regions takes R <= 32 regions and a weight image of M members that fits the LDS."""
    return 1 <= R <= MAX_REGIONS and (M * 32 * 36 + 32) * 4 + 128 <= 160 * 1024


def feature_head_regions(facc, nsum, w, bsum, order):
    """Region label map of feature-space window accumulators (csrc/window_features.hip): the inputs of feature_head_argmax with a
    head of R region outputs, plus `order` = regions_class_order -> int64 [X,Y,Z]: 0, then order[i] wherever
    sum_m w[m,i] . facc[m,v] + nsum[v] bsum[i] > 0, i = 0 .. R-1 in order (the sign of the accumulated sum is the sign of the
    ensemble-mean logit)."""
    if facc.dim() == 4:
        facc, w = facc[None], (w[None] if w.dim() == 2 else w)
    if not (facc.is_cuda and facc.dtype == torch.float32 and facc[0].is_contiguous() and facc.shape[-1] == 32):
        raise ValueError("feature_head_regions: fp32 GPU accumulators [M,X,Y,Z,32] expected")
    M, R = facc.shape[0], w.shape[1]
    if tuple(w.shape) != (M, R, 32) or tuple(bsum.shape) != (R,) or tuple(nsum.shape) != tuple(facc.shape[1:4]):
        raise ValueError("feature_head_regions: w [M,R,32], bsum [R], nsum [X,Y,Z] expected")
    order = check_regions_class_order(order, R)
    lib = _lib.load()
    w, bsum, nsum = w.float().contiguous(), bsum.float().contiguous(), nsum.float().contiguous()
    out = torch.empty(facc.shape[1:4], dtype=torch.int64, device=facc.device)
    check(lib.dgtta_feature_head_regions(ptr(facc), facc.stride(0) if M > 1 else 0, ptr(nsum), ptr(w), ptr(bsum), M, 32, R, out.numel(),
                                         (C_int * R)(*order), ptr(out), stream_of(facc.device)), "dgtta_feature_head_regions")
    return out


class _SoftDice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        lib = _lib.load()
        bsz, c = a.shape[:2]
        v = a[0, 0].numel()
        dense = [t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last_3d) for t in (a, b)]
        if not (all(dense) and a.stride() == b.stride()):
            a, b = a.contiguous(), b.contiguous()
        cl = a.dim() == 5 and not a.is_contiguous()             # dense channels-last
        strides = (v * c, 1, c) if cl else (v * c, v, 1)
        dice = torch.empty((bsz, c), dtype=torch.float32, device=a.device)
        nbytes = lib.dgtta_softdice_ws_bytes(bsz, c, v)
        ws = _ws(nbytes, a.device)
        check(lib.dgtta_softdice_probs_fwd(ptr(a), ptr(b), ptr(dice), ptr(ws), nbytes, bsz, c, v, *strides,
                                           stream_of(a.device)), "dgtta_softdice_probs_fwd")
        ctx.save_for_backward(a, b, ws)
        ctx.meta = (bsz, c, v, strides)
        return dice

    @staticmethod
    def backward(ctx, gdice):
        a, b, ws = ctx.saved_tensors
        bsz, c, v, strides = ctx.meta
        lib = _lib.load()
        ga, gb = torch.empty_like(a, memory_format=torch.preserve_format), torch.empty_like(b, memory_format=torch.preserve_format)
        check(lib.dgtta_softdice_probs_bwd(ptr(a), ptr(b), ptr(gdice.float().contiguous()), ptr(ga), ptr(gb), ptr(ws), bsz,
                                           c, v, *strides, stream_of(a.device)), "dgtta_softdice_probs_bwd")
        return ga, gb


def soft_dice(smp_a, smp_b):
    """soft_dice_loss(smp_a, smp_b) -> [B,C] of the reference (torch_utils.py:90-104) on probability maps [B,C,D,H,W]
    (fp32, contiguous or channels_last_3d); differentiable w.r.t. both inputs."""
    require_cuda(smp_a, smp_b)
    assert smp_a.shape == smp_b.shape and smp_a.dim() >= 3
    return _SoftDice.apply(smp_a.float(), smp_b.float())


# ------------------------------------------------------------------------------------------------ AdamW
def adamw_step(params, grads, exp_avgs, exp_avg_sqs, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
               grad_scale=1.0, skip_flag=None):
    """One multi-tensor AdamW step; skipped on the device when skip_flag (int32 device scalar) is non-zero."""
    lib = _lib.load()
    n = len(params)
    if n == 0:
        return
    require_cuda(*params)
    P = C.c_void_p * n
    hp = P(*[p.data_ptr() for p in params])
    hg = P(*[(g.data_ptr() if g is not None else None) for g in grads])
    hm = P(*[m.data_ptr() for m in exp_avgs])
    hv = P(*[v.data_ptr() for v in exp_avg_sqs])
    hn = (C.c_int64 * n)(*[p.numel() for p in params])
    check(lib.dgtta_adamw_step(hp, hg, hm, hv, hn, n, float(lr), float(betas[0]), float(betas[1]), float(eps),
                               float(weight_decay), int(step), float(grad_scale), ptr(skip_flag),
                               stream_of(params[0].device)), "dgtta_adamw_step")


def grads_nonfinite(grads, flag):
    """Sets flag (int32 device scalar, zeroed by the caller) when any element of `grads` is inf / NaN."""
    lib = _lib.load()
    grads = [g for g in grads if g is not None]
    if not grads:
        return
    require_cuda(*grads)
    n = len(grads)
    hg = (C.c_void_p * n)(*[g.data_ptr() for g in grads])
    hn = (C.c_int64 * n)(*[g.numel() for g in grads])
    check(lib.dgtta_grads_nonfinite(hg, hn, n, ptr(flag), stream_of(grads[0].device)), "dgtta_grads_nonfinite")


# ------------------------------------------------------------------------------------------------ clipped SGD
def grad_sumsq_ws_bytes(total_elements, ntensors):
    return int(_lib.load().dgtta_grad_sumsq_ws_bytes(int(total_elements), int(ntensors)))


def grad_sumsq(grads, out=None, ws=None):
    """Sum of squares of every element of `grads` (fp32 GPU tensors, None entries skipped) -> fp32 device scalar `out`;
    bit-reproducible (csrc/sgd.hip).  ws: uint8 workspace of grad_sumsq_ws_bytes(total elements, len) bytes, allocated
    when not given."""
    lib = _lib.load()
    grads = [g for g in grads if g is not None]
    require_cuda(*grads)
    require_cuda(out, ws)
    if not grads and out is None:
        raise ValueError("grad_sumsq: no gradient and no `out` to tell the device from")
    for g in grads:
        if g.dtype != torch.float32 or not g.is_contiguous():
            raise ValueError("grad_sumsq: contiguous fp32 gradients expected")
    device = grads[0].device if grads else out.device
    n = len(grads)
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=device)
    elif out.dtype != torch.float32 or out.numel() != 1:
        raise ValueError("grad_sumsq: `out` is one fp32 element")
    need = grad_sumsq_ws_bytes(sum(g.numel() for g in grads), n)
    if ws is None:
        ws = _ws(need, device)
    elif ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need:
        raise ValueError(f"grad_sumsq: `ws` is a contiguous uint8 tensor of at least {need} bytes")
    hg = (C.c_void_p * max(n, 1))(*[g.data_ptr() for g in grads])
    hn = (C.c_int64 * max(n, 1))(*[g.numel() for g in grads])
    check(lib.dgtta_grad_sumsq(hg, hn, n, ptr(out), ptr(ws), ws.numel(), stream_of(device)), "dgtta_grad_sumsq")
    return out


def sgd_step(params, grads, bufs, lr, momentum=0.99, weight_decay=3e-5, nesterov=True, first_step=False, grad_scale=1.0,
             sumsq=None, max_norm=12.0, skip_flag=None):
    """One multi-tensor clipped SGD step (csrc/sgd.hip; formula in include/dgtta.h).  sumsq: the device scalar of
    grad_sumsq over ALL gradients of the step (None: no clipping); first_step: `bufs` are written, not read; skipped on
    the device when skip_flag (int32 device scalar) is non-zero."""
    lib = _lib.load()
    n = len(params)
    if n == 0:
        return
    require_cuda(*params)
    require_cuda(*grads)
    require_cuda(*bufs)
    require_cuda(sumsq, skip_flag)
    for p, g, b in zip(params, grads, bufs):
        for t in (p, g, b):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError("sgd_step: contiguous fp32 tensors expected")
        if (g is not None and g.numel() != p.numel()) or b.numel() != p.numel():
            raise ValueError("sgd_step: a gradient or momentum buffer does not have its parameter's element count")
    P = C.c_void_p * n
    hp = P(*[p.data_ptr() for p in params])
    hg = P(*[(g.data_ptr() if g is not None else None) for g in grads])
    hb = P(*[b.data_ptr() for b in bufs])
    hn = (C.c_int64 * n)(*[p.numel() for p in params])
    check(lib.dgtta_sgd_step(hp, hg, hb, hn, n, float(lr), float(momentum), float(weight_decay), int(bool(nesterov)),
                             int(bool(first_step)), float(grad_scale), ptr(sumsq), float(max_norm), ptr(skip_flag),
                             stream_of(params[0].device)), "dgtta_sgd_step")


# ------------------------------------------------------------------------------------------------ eval helpers
def argmax_dice(logits, labels=None):
    """argmax over channels (+ per-label counts for hard Dice, tta.py:321, torch_utils.py:107-117).

    Returns (argmax [B,D,H,W] int64, counts [3,C] int64 or None)."""
    require_cuda(logits)
    lib = _lib.load()
    b, c, d, h, w = logits.shape
    lg = logits.float().contiguous(memory_format=torch.channels_last_3d)
    am = torch.empty((b, d, h, w), dtype=torch.int64, device=lg.device)
    counts = None
    lp = None
    if labels is not None:
        labels = labels.reshape(b, d, h, w).to(torch.int64).contiguous()
        counts = torch.zeros((3, c), dtype=torch.int64, device=lg.device)
        lp = labels.data_ptr()
    check(lib.dgtta_argmax_dice(ptr(lg), c, c, lp, ptr(am), ptr(counts), b, d * h * w, stream_of(lg.device)),
          "dgtta_argmax_dice")
    return am, counts


def feature_head_argmax(facc, nsum, w, bsum):
    """Label map of feature-space window accumulators (csrc/window_features.hip): facc [M,X,Y,Z,32] fp32, nsum [X,Y,Z], w [M,C,32],
    bsum [C] = sum of the members' head biases -> int64 [X,Y,Z] = argmax_c sum_m (w[m,c] . facc[m,v]) + nsum[v] bsum[c]."""
    if facc.dim() == 4:
        facc, w = facc[None], (w[None] if w.dim() == 2 else w)
    if not (facc.is_cuda and facc.dtype == torch.float32 and facc[0].is_contiguous() and facc.shape[-1] == 32):
        raise ValueError("feature_head_argmax: fp32 GPU accumulators [M,X,Y,Z,32] expected")
    M, C = facc.shape[0], w.shape[1]
    if tuple(w.shape) != (M, C, 32) or tuple(bsum.shape) != (C,) or tuple(nsum.shape) != tuple(facc.shape[1:4]):
        raise ValueError("feature_head_argmax: w [M,C,32], bsum [C], nsum [X,Y,Z] expected")
    lib = _lib.load()
    w, bsum, nsum = w.float().contiguous(), bsum.float().contiguous(), nsum.float().contiguous()
    out = torch.empty(facc.shape[1:4], dtype=torch.int64, device=facc.device)
    check(lib.dgtta_feature_head_argmax(ptr(facc), facc.stride(0) if M > 1 else 0, ptr(nsum), ptr(w), ptr(bsum), M, 32, C, out.numel(),
                                        ptr(out), stream_of(facc.device)), "dgtta_feature_head_argmax")
    return out


MAX_SELECTED_CLASSES = 32


def check_selected_classes(classes, num_classes):
    """The `sel` list of the softmax entry points as plain ints: 1..32 DISTINCT class indices in [0, num_classes), any order.
    ValueError otherwise (checked before anything touches the GPU)."""
    sel = [int(c) for c in classes]
    if not 1 <= len(sel) <= MAX_SELECTED_CLASSES:
        raise ValueError(f"classes: 1..{MAX_SELECTED_CLASSES} selected classes expected, got {len(sel)}")
    if len(set(sel)) != len(sel):
        raise ValueError(f"classes: duplicate class index in {sel}")
    if min(sel) < 0 or max(sel) >= num_classes:
        raise ValueError(f"classes: index outside [0, {num_classes}) in {sel}")
    return sel


def prob_dtype_code(prob_dtype):
    if prob_dtype not in (torch.float32, torch.float16):
        raise ValueError(f"probabilities are stored as float32 or float16, not {prob_dtype}")
    return F32 if prob_dtype == torch.float32 else F16


def feature_head_softmax_supported(M, C):
    """dgtta_feature_head_softmax takes C <= 128 and a weight image of M members that fits the LDS (the limits of
    dgtta_feature_head_argmax's matrix-core path); anything wider belongs to the class-group path."""
    ncb = (C + 31) // 32
    return ncb <= 4 and (M * 32 * ncb * 36 + 32 * ncb) * 4 + 128 <= 160 * 1024


def feature_head_softmax(facc, nsum, w, bsum, classes, prob_dtype=torch.float32):
    """Softmax end of feature-space window accumulators (csrc/window_features.hip; definitions in include/dgtta.h, nnU-Net's from
    memory, UNPINNED): the inputs of feature_head_argmax plus `classes` (see check_selected_classes) ->
    (label int64 [X,Y,Z] - the integers feature_head_argmax returns -, confidence fp32 [X,Y,Z] = p[label], entropy fp32 [X,Y,Z] in
    nats, probs prob_dtype [K,X,Y,Z] = p[classes[k]]) of p = softmax over ALL C classes of the ensemble-mean logits
    (sum_m w[m,c] . facc[m,v] + nsum[v] bsum[c]) / (M nsum[v]).  The K maps sum to at most 1: the rest is mass on other classes."""
    sel = check_selected_classes(classes, w.shape[-2])
    code = prob_dtype_code(prob_dtype)
    if facc.dim() == 4:
        facc, w = facc[None], (w[None] if w.dim() == 2 else w)
    if not (facc.is_cuda and facc.dtype == torch.float32 and facc[0].is_contiguous() and facc.shape[-1] == 32):
        raise ValueError("feature_head_softmax: fp32 GPU accumulators [M,X,Y,Z,32] expected")
    M, C = facc.shape[0], w.shape[1]
    if tuple(w.shape) != (M, C, 32) or tuple(bsum.shape) != (C,) or tuple(nsum.shape) != tuple(facc.shape[1:4]):
        raise ValueError("feature_head_softmax: w [M,C,32], bsum [C], nsum [X,Y,Z] expected")
    lib = _lib.load()
    w, bsum, nsum = w.float().contiguous(), bsum.float().contiguous(), nsum.float().contiguous()
    shp, dev, K = facc.shape[1:4], facc.device, len(sel)
    label = torch.empty(shp, dtype=torch.int64, device=dev)
    conf = torch.empty(shp, dtype=torch.float32, device=dev)
    ent = torch.empty(shp, dtype=torch.float32, device=dev)
    probs = torch.empty((K, *shp), dtype=prob_dtype, device=dev)
    check(lib.dgtta_feature_head_softmax(ptr(facc), facc.stride(0) if M > 1 else 0, ptr(nsum), ptr(w), ptr(bsum), M, 32, C, label.numel(),
                                         (C_int * K)(*sel), K, code, ptr(label), ptr(conf), ptr(ent), ptr(probs), stream_of(dev)),
          "dgtta_feature_head_softmax")
    return label, conf, ent, probs


def argmax_rows(acc):
    """Label map of a voxel-major accumulator [..., C] (fp32 or fp16, contiguous): argmax over the last axis, int64."""
    require_cuda(acc)
    if acc.dtype not in (torch.float32, torch.float16) or not acc.is_contiguous():
        raise ValueError("argmax_rows: contiguous fp32 / fp16 rows expected")
    lib = _lib.load()
    out = torch.empty(acc.shape[:-1], dtype=torch.int64, device=acc.device)
    check(lib.dgtta_argmax_rows(ptr(acc), F32 if acc.dtype == torch.float32 else F16, acc.shape[-1], out.numel(), ptr(out),
                                stream_of(acc.device)), "dgtta_argmax_rows")
    return out


def argmax_dice_from_labels(pred, labels, num_classes):
    """Per-label counts for two integer label maps (dice_coeff, torch_utils.py:107-117): counts [3,C] int64."""
    require_cuda(pred, labels)
    lib = _lib.load()
    pr = pred.reshape(-1).to(torch.int64).contiguous()
    lb = labels.reshape(-1).to(torch.int64).contiguous()
    assert pr.numel() == lb.numel()
    counts = torch.zeros((3, num_classes), dtype=torch.int64, device=pr.device)
    check(lib.dgtta_argmax_dice(None, 0, num_classes, ptr(lb), ptr(pr), ptr(counts), 1, pr.numel(),
                                stream_of(pr.device)), "dgtta_argmax_dice")
    return pr, counts


# ------------------------------------------------------------------------------------------------ surface distances
def _label_map3(t, name):
    require_cuda(t)
    if t.dim() != 3 or t.dtype != torch.int64 or not t.is_contiguous():
        raise ValueError(f"{name}: contiguous int64 label map [D,H,W] expected")
    return t


def label_bboxes(a, b, nlab):
    """Inclusive bounding boxes of every label < nlab in the union of two int64 label maps [D,H,W] of equal shape: int32
    [nlab,6] = (lo d, lo h, lo w, hi d, hi h, hi w); a label in neither map has lo > hi."""
    _label_map3(a, "label_bboxes"), _label_map3(b, "label_bboxes")
    if a.shape != b.shape:
        raise ValueError(f"label_bboxes: shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
    lib = _lib.load()
    boxes = torch.empty((int(nlab), 6), dtype=torch.int32, device=a.device)
    d, h, w = a.shape
    check(lib.dgtta_label_bboxes(ptr(a), ptr(b), d, h, w, int(nlab), ptr(boxes), stream_of(a.device)), "dgtta_label_bboxes")
    return boxes


def label_surface(label_map, label, box=None, out=None):
    """Surface voxels of (label_map == label) inside the crop box (d0, h0, w0, cd, ch, cw) (default: the whole volume): uint8
    [cd,ch,cw], 1 where the voxel carries the label and one of its six face neighbours (read from the full map; outside the volume
    counts) does not.  `out`: a uint8 buffer of at least cd*ch*cw elements to write into."""
    _label_map3(label_map, "label_surface")
    lib = _lib.load()
    d, h, w = label_map.shape
    d0, h0, w0, cd, ch, cw = (0, 0, 0, d, h, w) if box is None else (int(v) for v in box)
    n = cd * ch * cw
    if out is None:
        surf = torch.empty((cd, ch, cw), dtype=torch.uint8, device=label_map.device)
    else:
        if out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < n or out.device != label_map.device:
            raise ValueError("label_surface: out must be a contiguous uint8 buffer of at least cd*ch*cw elements on the map's device")
        surf = out.reshape(-1)[:n].view(cd, ch, cw)
    check(lib.dgtta_label_surface(ptr(label_map), d, h, w, int(label), d0, h0, w0, cd, ch, cw, ptr(surf), stream_of(label_map.device)),
          "dgtta_label_surface")
    return surf


def edt_ws_bytes(d, h, w):
    return int(_lib.load().dgtta_edt_ws_bytes(int(d), int(h), int(w)))


def edt_sq(site, spacing=(1.0, 1.0, 1.0), out=None, ws=None):
    """Exact squared Euclidean distance transform (csrc/surface.hip): site uint8 [D,H,W] -> fp32 [D,H,W], the squared physical
    distance to the nearest nonzero voxel of `site` at the per-axis `spacing` (d, h, w); +inf everywhere without a site.  `out`
    (fp32, at least D*H*W elements) and `ws` (uint8, at least edt_ws_bytes(D,H,W)) let a caller reuse its buffers."""
    require_cuda(site)
    if site.dim() != 3 or site.dtype != torch.uint8 or not site.is_contiguous():
        raise ValueError("edt_sq: contiguous uint8 site mask [D,H,W] expected")
    lib = _lib.load()
    d, h, w = site.shape
    n = d * h * w
    if out is None:
        dist2 = torch.empty((d, h, w), dtype=torch.float32, device=site.device)
    else:
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < n or out.device != site.device:
            raise ValueError("edt_sq: out must be a contiguous fp32 buffer of at least D*H*W elements on the mask's device")
        dist2 = out.reshape(-1)[:n].view(d, h, w)
    nbytes = lib.dgtta_edt_ws_bytes(d, h, w)
    if ws is None:
        ws = _ws(nbytes, site.device)
    elif ws.dtype != torch.uint8 or ws.numel() < nbytes or ws.device != site.device:
        raise ValueError("edt_sq: ws must be a uint8 buffer of at least edt_ws_bytes(D,H,W) bytes on the mask's device")
    sd, sh, sw = (float(s) for s in spacing)
    check(lib.dgtta_edt_sq(ptr(site), ptr(dist2), ptr(ws), ws.numel(), d, h, w, sd, sh, sw, stream_of(site.device)), "dgtta_edt_sq")
    return dist2


# ------------------------------------------------------------------------------------------------ connected components
CC_MAX_TABLE = 1024


def _group_table(group, label_map, name):
    if (group.dim() != 1 or group.dtype != torch.int32 or not group.is_contiguous() or group.device != label_map.device
            or not 0 < group.numel() <= CC_MAX_TABLE):
        raise ValueError(f"{name}: group must be a contiguous int32 table of 1 to {CC_MAX_TABLE} entries on the map's device")
    return group


def _cc_buffer(out, n, dtype, device, name, what):
    if out.dtype != dtype or not out.is_contiguous() or out.numel() < n or out.device != device:
        raise ValueError(f"{name}: {what} must be a contiguous {str(dtype).replace('torch.', '')} buffer of at least D*H*W elements "
                         f"on the map's device")
    return out.reshape(-1)[:n]


def _cc_ws(ws, nbytes, device, name):
    if ws is None:
        return _ws(nbytes, device)
    if ws.dtype != torch.uint8 or ws.numel() < nbytes or ws.device != device:
        raise ValueError(f"{name}: ws must be a uint8 buffer of at least cc_ws_bytes(D,H,W) bytes on the map's device")
    return ws


def cc_ws_bytes(d, h, w):
    return int(_lib.load().dgtta_cc_ws_bytes(int(d), int(h), int(w)))


def cc_label(label_map, group, connectivity=26, out=None, ws=None):
    """Canonical connected components (csrc/components.hip) of an int64 label map [D,H,W]: int32 [D,H,W], 0 where
    g = group[label] is 0 (labels outside the int32 table `group` included), elsewhere 1 + the smallest linear index of the voxel's
    component.  Voxels are connected iff they are neighbours under `connectivity` (6, 18, 26) and have equal, non-zero g.  `out`
    (int32, at least D*H*W elements) and `ws` (uint8, at least cc_ws_bytes(D,H,W)) let a caller reuse its buffers."""
    _label_map3(label_map, "cc_label")
    _group_table(group, label_map, "cc_label")
    lib = _lib.load()
    d, h, w = label_map.shape
    n = d * h * w
    cc = (torch.empty(n, dtype=torch.int32, device=label_map.device) if out is None
          else _cc_buffer(out, n, torch.int32, label_map.device, "cc_label", "out")).view(d, h, w)
    ws = _cc_ws(ws, lib.dgtta_cc_ws_bytes(d, h, w), label_map.device, "cc_label")
    check(lib.dgtta_cc_label(ptr(label_map), ptr(group), group.numel(), d, h, w, int(connectivity), ptr(cc), ptr(ws), ws.numel(),
                             stream_of(label_map.device)), "dgtta_cc_label")
    return cc


def cc_sizes(cc, out=None):
    """size int32 [D*H*W] of a cc_label result: size[r] = the number of voxels with cc == r + 1 (0 where r is not a component's
    first voxel).  `out`: an int32 buffer of at least D*H*W elements."""
    require_cuda(cc)
    if cc.dtype != torch.int32 or not cc.is_contiguous() or cc.numel() == 0:
        raise ValueError("cc_sizes: contiguous int32 component map expected")
    n = cc.numel()
    size = torch.empty(n, dtype=torch.int32, device=cc.device) if out is None else _cc_buffer(out, n, torch.int32, cc.device, "cc_sizes",
                                                                                                "out")
    check(_lib.load().dgtta_cc_sizes(ptr(cc), n, ptr(size), stream_of(cc.device)), "dgtta_cc_sizes")
    return size


def cc_filter(label_map, group, cc, size, keep_largest=True, min_voxels=0, background=0, out=None, ws=None):
    """(filtered map int64 [D,H,W], removed int64 [len(group)]): a voxel with g != 0 keeps its label iff (not keep_largest or its
    component is the largest of its group, ties to the smaller cc) and its component has at least min_voxels voxels, otherwise it
    becomes `background`; g == 0 passes through.  removed[c] = voxels removed from group c.  `cc`, `size`: cc_label / cc_sizes of the
    same map and table.  `out` (int64, at least D*H*W elements) and `ws` as in cc_label."""
    _label_map3(label_map, "cc_filter")
    _group_table(group, label_map, "cc_filter")
    lib = _lib.load()
    d, h, w = label_map.shape
    n = d * h * w
    cc = _cc_buffer(cc, n, torch.int32, label_map.device, "cc_filter", "cc")
    size = _cc_buffer(size, n, torch.int32, label_map.device, "cc_filter", "size")
    if not 0 <= int(min_voxels) < 2 ** 31:
        raise ValueError("cc_filter: min_voxels must be in [0, 2^31)")
    res = (torch.empty(n, dtype=torch.int64, device=label_map.device) if out is None
           else _cc_buffer(out, n, torch.int64, label_map.device, "cc_filter", "out")).view(d, h, w)
    ws = _cc_ws(ws, lib.dgtta_cc_ws_bytes(d, h, w), label_map.device, "cc_filter")
    removed = torch.empty(group.numel(), dtype=torch.int64, device=label_map.device)
    check(lib.dgtta_cc_filter(ptr(label_map), ptr(group), group.numel(), ptr(cc), ptr(size), n, int(bool(keep_largest)), int(min_voxels),
                              int(background), ptr(res), ptr(removed), ptr(ws), ws.numel(), stream_of(label_map.device)),
          "dgtta_cc_filter")
    return res, removed


# ------------------------------------------------------------------------------------------------ hole filling
def _mask3(t, name, what="mask"):
    require_cuda(t)
    if t.dim() != 3 or t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() == 0:
        raise ValueError(f"{name}: contiguous uint8 {what} [D,H,W] expected")
    return t


def holes_ws_bytes(d, h, w):
    return int(_lib.load().dgtta_holes_ws_bytes(int(d), int(h), int(w)))


def fill_holes(mask, connectivity=6, out=None, ws=None, return_box=False):
    """(filled uint8 [D,H,W], n_filled) of a uint8 membership mask (non-zero = member): the mask plus its enclosed voxels, those
    whose component of the complement under `connectivity` (6, 18, 26) touches none of the six faces of the volume
    (csrc/components.hip).  Connectivity 6 is scipy.ndimage.binary_fill_holes.  n_filled: the number of enclosed voxels, a 0-dim
    int64 tensor on the device (reading it synchronises).  `out` (uint8, at least D*H*W elements) and `ws` (uint8, at least
    holes_ws_bytes(D,H,W)) let a caller reuse its buffers.  return_box: a third result, int32 [6] on the device = the inclusive
    bounding box of `filled` (lo d, h, w, hi d, h, w; lo > hi when it is empty)."""
    _mask3(mask, "fill_holes")
    if isinstance(connectivity, bool) or connectivity not in (6, 18, 26):
        raise ValueError(f"fill_holes: connectivity {connectivity!r} (6, 18 or 26)")
    lib = _lib.load()
    d, h, w = mask.shape
    n = d * h * w
    filled = (torch.empty(n, dtype=torch.uint8, device=mask.device) if out is None
              else _cc_buffer(out, n, torch.uint8, mask.device, "fill_holes", "out")).view(d, h, w)
    nbytes = lib.dgtta_holes_ws_bytes(d, h, w)
    if ws is None:
        ws = _ws(nbytes, mask.device)
    elif ws.dtype != torch.uint8 or ws.numel() < nbytes or ws.device != mask.device:
        raise ValueError("fill_holes: ws must be a uint8 buffer of at least holes_ws_bytes(D,H,W) bytes on the mask's device")
    n_filled = torch.empty((), dtype=torch.int64, device=mask.device)
    box = torch.empty(6, dtype=torch.int32, device=mask.device) if return_box else None
    check(lib.dgtta_holes_fill(ptr(mask), d, h, w, int(connectivity), ptr(filled), ptr(n_filled), ptr(box), ptr(ws), ws.numel(),
                               stream_of(mask.device)), "dgtta_holes_fill")
    return (filled, n_filled, box) if return_box else (filled, n_filled)


def holes_member(label_map, group, box):
    """uint8 [cd,ch,cw]: 1 where group[label] != 0 (the table rule of cc_label) inside the crop box (d0, h0, w0, cd, ch, cw) of an
    int64 label map."""
    _label_map3(label_map, "holes_member")
    _group_table(group, label_map, "holes_member")
    d, h, w = label_map.shape
    d0, h0, w0, cd, ch, cw = (int(v) for v in box)
    mask = torch.empty((cd, ch, cw), dtype=torch.uint8, device=label_map.device)
    check(_lib.load().dgtta_holes_member(ptr(label_map), d, h, w, ptr(group), group.numel(), d0, h0, w0, cd, ch, cw, ptr(mask),
                                         stream_of(label_map.device)), "dgtta_holes_member")
    return mask


def holes_apply(label_map, mask, filled, box, background, label):
    """IN PLACE on the int64 label map: inside the crop box (d0, h0, w0, cd, ch, cw) a voxel that `filled` has and `mask` has not
    (both uint8 [cd,ch,cw]) and whose value is `background` becomes `label`.  Returns the number of voxels changed, a 0-dim
    int64 tensor on the device."""
    _label_map3(label_map, "holes_apply")
    d, h, w = label_map.shape
    d0, h0, w0, cd, ch, cw = (int(v) for v in box)
    for t, what in ((mask, "mask"), (filled, "filled")):
        _mask3(t, "holes_apply", what)
        if tuple(t.shape) != (cd, ch, cw) or t.device != label_map.device:
            raise ValueError(f"holes_apply: {what} must have the box's shape {(cd, ch, cw)} on the map's device")
    count = torch.empty((), dtype=torch.int64, device=label_map.device)
    check(_lib.load().dgtta_holes_apply(ptr(label_map), d, h, w, ptr(mask), ptr(filled), d0, h0, w0, cd, ch, cw, int(background),
                                        int(label), ptr(count), stream_of(label_map.device)), "dgtta_holes_apply")
    return count


def nonzero_mask(data):
    """uint8 [*spatial] = OR over the channels of (data[c] != 0) for float32 data [C, *spatial]: IEEE comparison, so NaN counts as
    non-zero and -0.0 as zero, as numpy's `!=` does."""
    require_cuda(data)
    if data.dim() < 2 or data.dtype != torch.float32 or not data.is_contiguous() or data.numel() == 0:
        raise ValueError("nonzero_mask: contiguous float32 data [C, ...] expected")
    mask = torch.empty(data.shape[1:], dtype=torch.uint8, device=data.device)
    check(_lib.load().dgtta_nonzero_mask(ptr(data), data.shape[0], mask.numel(), ptr(mask), stream_of(data.device)), "dgtta_nonzero_mask")
    return mask


# ------------------------------------------------------------------------------------------------ spatial augmentation
def _volume3(t, name, what):
    t = t.reshape(t.shape[-3:]) if t.dim() > 3 and t.numel() == t.shape[-3] * t.shape[-2] * t.shape[-1] else t
    if t.dim() != 3 or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() == 0:
        raise ValueError(f"{name}: {what} must be a contiguous float32 volume [D, H, W] (leading axes of extent 1 allowed)")
    return t


def bspline3_prefilter(volume):
    """scipy.ndimage.spline_filter(volume, order=3, mode="mirror") in fp32 (csrc/spatial_aug.hip): the cubic B-spline
    coefficients sample_patches_aug(order=3) reads.  volume: float32 [D, H, W] on the GPU -> a new tensor of that shape."""
    require_cuda(volume)
    src = _volume3(volume, "bspline3_prefilter", "volume")
    dst = torch.empty_like(src)
    d, h, w = src.shape
    check(_lib.load().dgtta_bspline3_prefilter(ptr(src), ptr(dst), d, h, w, stream_of(src.device)), "dgtta_bspline3_prefilter")
    return dst.reshape(volume.shape)


def sample_patches_aug(coefs, label_maps, maps, patch_size, order=3):
    """One launch that samples len(coefs) <= 16 patches through affine voxel maps (csrc/spatial_aug.hip, include/dgtta.h).
    coefs: per item the float32 volume the image is read from - B-spline coefficients (bspline3_prefilter) for order 3, the
    raw volume for order 1; label_maps: per item the label map as float32 values, same shape; maps: per item a 3 x 4 [A | t]
    (anything numpy converts; rounded to fp32): output voxel v reads source position A v + t, (D, H, W) order, voxel units.
    Items may differ in volume shape.  Returns (image float32 [B, 1, *patch_size], labels int64 [B, *patch_size])."""
    import numpy as np
    n = len(coefs)
    if not (1 <= n <= _lib.PATCH_MAX_ITEMS and len(label_maps) == n and len(maps) == n):
        raise ValueError(f"sample_patches_aug: 1..{_lib.PATCH_MAX_ITEMS} items with one label map and one map each (got {n}, "
                         f"{len(label_maps)}, {len(maps)})")
    if order not in (1, 3):
        raise ValueError(f"sample_patches_aug: order {order} not in (1, 3)")
    pd, ph, pw = (int(p) for p in patch_size)
    items = (_lib.PatchItem * n)()
    keep = []
    for b in range(n):
        require_cuda(coefs[b], label_maps[b])
        img, lab = _volume3(coefs[b], "sample_patches_aug", "an image"), _volume3(label_maps[b], "sample_patches_aug", "a label map")
        if img.shape != lab.shape or img.device != lab.device or img.device != coefs[0].device:
            raise ValueError(f"sample_patches_aug: item {b}: image {tuple(img.shape)} and label map {tuple(lab.shape)} must agree "
                             f"in shape and lie on one device")
        m = np.asarray(maps[b], dtype=np.float64)
        if m.shape != (3, 4) or not np.isfinite(m).all():
            raise ValueError(f"sample_patches_aug: item {b}: a finite 3 x 4 map expected")
        keep += [img, lab]
        items[b].image, items[b].label = img.data_ptr(), lab.data_ptr()
        items[b].D, items[b].H, items[b].W = (int(s) for s in img.shape)
        items[b].map[:] = m.astype(np.float32).reshape(-1).tolist()
    device = coefs[0].device
    image = torch.empty((n, 1, pd, ph, pw), dtype=torch.float32, device=device)
    labels = torch.empty((n, pd, ph, pw), dtype=torch.int64, device=device)
    check(_lib.load().dgtta_patch_sample_aug(items, n, pd, ph, pw, int(order), ptr(image), ptr(labels), stream_of(device)),
          "dgtta_patch_sample_aug")
    return image, labels


# ------------------------------------------------------------------------------------------------ mirroring
MIRROR_SUBSET_ORDER = ((), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2))


def check_mirror_axes(axes):
    """None, or the sorted tuple of a subset of (0, 1, 2) (an empty subset is None: nothing to mirror)."""
    if axes is None:
        return None
    axes = tuple(sorted(int(a) for a in axes))
    if len(set(axes)) != len(axes) or any(a not in (0, 1, 2) for a in axes):
        raise ValueError(f"mirror axes {axes}: None or a subset of (0, 1, 2) expected")
    return axes or None


def mirror_masks(axes):
    """The mirror masks (bit a = axis a flipped) of every subset of the allowed axes, in the order nnU-Net's predictor runs its
    passes: (), (0), (1), (2), (0,1), (0,2), (1,2), (0,1,2) restricted to `axes`.  None -> [0]."""
    axes = check_mirror_axes(axes)
    if axes is None:
        return [0]
    return [sum(1 << a for a in s) for s in MIRROR_SUBSET_ORDER if all(a in axes for a in s)]


def mirror_batch(images, labels, masks):
    """nnU-Net's MirrorTransform on a batch in one launch (csrc/mirror.hip): images float32 [B, C, D, H, W] and labels int64
    [B, D, H, W] on the GPU, masks: B host integers 0..7 (bit 0 = D, bit 1 = H, bit 2 = W flipped; 0 = copied).  Returns new
    (images, labels)."""
    import ctypes
    require_cuda(images, labels)
    B = images.shape[0] if images.dim() == 5 else -1
    if (images.dim() != 5 or images.dtype != torch.float32 or labels.dtype != torch.int64 or
            tuple(labels.shape) != (B, *images.shape[2:]) or labels.device != images.device):
        raise ValueError(f"mirror_batch: float32 images [B, C, D, H, W] and int64 labels [B, D, H, W] on one device expected "
                         f"(got {tuple(images.shape)} {images.dtype}, {tuple(labels.shape)} {labels.dtype})")
    masks = [int(m) for m in masks]
    if len(masks) != B or any(not 0 <= m <= 7 for m in masks):
        raise ValueError(f"mirror_batch: {B} masks in 0..7 expected (got {masks})")
    images, labels = images.contiguous(), labels.contiguous()
    out_i, out_l = torch.empty_like(images), torch.empty_like(labels)
    check(_lib.load().dgtta_mirror_batch(ptr(images), ptr(labels), ptr(out_i), ptr(out_l), (ctypes.c_int * B)(*masks), B,
                                         *(int(s) for s in images.shape[1:]), stream_of(images.device)), "dgtta_mirror_batch")
    return out_i, out_l


def window_gather(volume, origins, masks, patch_size):
    """The window batch [n, C, *patch_size] (float32) of sliding-window inference with mirroring, in one launch per 16 windows
    (csrc/mirror.hip): window k is the block of `volume` [C, X, Y, Z] (float32, GPU) at origins[k], flipped along the axes of
    masks[k]."""
    import ctypes
    require_cuda(volume)
    n = len(origins)
    if volume.dim() != 4 or volume.dtype != torch.float32 or len(masks) != n or n < 1:
        raise ValueError("window_gather: a float32 volume [C, X, Y, Z], n >= 1 origins and n masks expected")
    volume = volume.contiguous()
    flat = [int(v) for o in origins for v in o]
    out = torch.empty((n, volume.shape[0], *(int(p) for p in patch_size)), dtype=torch.float32, device=volume.device)
    check(_lib.load().dgtta_window_gather(ptr(volume), ptr(out), (ctypes.c_int * (3 * n))(*flat), (ctypes.c_int * n)(*[int(m) for m in masks]),
                                          n, volume.shape[0], *(int(p) for p in patch_size), *(int(s) for s in volume.shape[1:]),
                                          stream_of(volume.device)), "dgtta_window_gather")
    return out


# ------------------------------------------------------------------------------------------------ intensity augmentation
IMAP_MODES = {"linear": _lib.IMAP_LINEAR, "contrast": _lib.IMAP_CONTRAST, "gamma": _lib.IMAP_GAMMA, "restore": _lib.IMAP_RESTORE}


def _intensity_batch(x, name, what="x"):
    """(B, D, H, W) of a batch [B, (1,) D, H, W] the intensity kernels take; ValueError for anything else."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f"{name}: `{what}` must be a CUDA tensor (there is no CPU fallback)")
    if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"{name}: `{what}` must be a non-empty contiguous float32 tensor")
    if not (x.dim() == 4 or (x.dim() == 5 and x.shape[1] == 1)):
        raise ValueError(f"{name}: `{what}` must be [B, 1, D, H, W] or [B, D, H, W] (got {tuple(x.shape)})")
    return (int(x.shape[0]), *(int(s) for s in x.shape[-3:]))


def _intensity_items(items, b, name):
    items = [int(i) for i in items]
    if not 1 <= len(items) <= _lib.INTENSITY_MAX_ITEMS:
        raise ValueError(f"{name}: 1..{_lib.INTENSITY_MAX_ITEMS} items per launch (got {len(items)})")
    if len(set(items)) != len(items) or min(items) < 0 or max(items) >= b:
        raise ValueError(f"{name}: items {items} must be distinct indices into a batch of {b}")
    return items


def _intensity_params(values, n, name, what):
    import math
    values = [float(v) for v in values]
    if len(values) != n or not all(math.isfinite(v) for v in values):
        raise ValueError(f"{name}: {n} finite `{what}` expected (got {values})")
    return values


def _intensity_stats_arg(t, b, like, name, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != like.device or t.dtype != torch.float64 or \
            not t.is_contiguous() or tuple(t.shape) != (b, 4):
        raise ValueError(f"{name}: `{what}` must be a contiguous float64 CUDA tensor [{b}, 4] on the batch's device")
    return t


def _intensity_out(x, out, name):
    if out is None:
        return x
    _intensity_batch(out, name, "out")
    if out.shape != x.shape or out.device != x.device:
        raise ValueError(f"{name}: `out` must have the shape and device of `x`")
    return out


def intensity_stats_ws_bytes(n_items, voxels):
    return int(_lib.load().dgtta_intensity_stats_ws_bytes(int(n_items), int(voxels)))


def intensity_stats(x, items, out=None, ws=None):
    """Per item of `items` (indices into the batch x [B, 1, D, H, W], float32) its min, max, mean and population standard
    deviation -> out[item] of a float64 tensor [B, 4] on the device; rows of other items are left as they are (csrc/
    intensity_aug.hip; bit-reproducible, no read-back).  ws: uint8 workspace of intensity_stats_ws_bytes(len(items), voxels)."""
    b, d, h, w = _intensity_batch(x, "intensity_stats")
    items = _intensity_items(items, b, "intensity_stats")
    v = d * h * w
    out = torch.empty((b, 4), dtype=torch.float64, device=x.device) if out is None else _intensity_stats_arg(out, b, x, "intensity_stats", "out")
    need = intensity_stats_ws_bytes(len(items), v)
    if ws is None:
        ws = _ws(need, x.device)
    elif not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need:
        raise ValueError(f"intensity_stats: `ws` is a contiguous uint8 CUDA tensor of at least {need} bytes")
    h_items = (C.c_int * len(items))(*items)
    check(_lib.load().dgtta_intensity_stats(ptr(x), b, v, h_items, len(items), ptr(out), ptr(ws), ws.numel(), stream_of(x.device)),
          "dgtta_intensity_stats")
    return out


def intensity_map(x, items, mode, a=None, s=None, keys=None, offset=0, noise_index=None, negate=False, stats=None, stats2=None,
                  out=None):
    """One elementwise pass over the items `items` of the batch x [B, 1, D, H, W] (float32), formulas in include/dgtta.h:
      mode "linear"    x * a + s * n(v): a (default 1) and s (default 0: no noise) per item; keys: per item the 64-bit Philox
                       key of its noise, offset: counter words 2 and 3, noise_index: per item counter word 1 (default: the
                       item's index in the batch);
      mode "contrast"  clip((x - mean) * a + mean, min, max) with the item's row of `stats`;
      mode "gamma"     ((x - lo) / (r + 1e-7))^a * r + lo from `stats`; negate: of the negated item (not negated back);
      mode "restore"   (x - mean2) / (std2 + 1e-8) * std + mean with `stats` (before the power) and `stats2` (after); negate:
                       the mean of the negated item, and the result negated back.
    stats / stats2: float64 [B, 4] as intensity_stats writes them, read on the device.  Writes `out` (default: x itself, in
    place); items that are not named are neither read nor written.  Returns out."""
    name = "intensity_map"
    b, d, h, w = _intensity_batch(x, name)
    items = _intensity_items(items, b, name)
    n = len(items)
    if mode not in IMAP_MODES:
        raise ValueError(f"{name}: mode {mode!r} not in {sorted(IMAP_MODES)}")
    out = _intensity_out(x, out, name)
    a = _intensity_params([1.0] * n if a is None else a, n, name, "a")
    s = _intensity_params([0.0] * n if s is None else s, n, name, "s")
    if mode != "linear":
        stats = _intensity_stats_arg(stats, b, x, name, "stats")
        if any(v != 0.0 for v in s):
            raise ValueError(f"{name}: noise belongs to mode 'linear'")
    if mode == "restore":
        stats2 = _intensity_stats_arg(stats2, b, x, name, "stats2")
    if mode == "gamma" and not all(v > 0.0 for v in a):
        raise ValueError(f"{name}: gamma exponents must be positive (got {a})")
    keys = [0] * n if keys is None else [_u64(k) for k in keys]
    noise_index = items if noise_index is None else [int(i) for i in noise_index]
    if len(keys) != n or len(noise_index) != n or any(not 0 <= i < 2 ** 31 for i in noise_index):
        raise ValueError(f"{name}: one key and one noise index in [0, 2^31) per item expected")
    off = _u64(offset)
    desc = (_lib.IntensityItem * n)()
    for k in range(n):
        desc[k].item, desc[k].mode, desc[k].negate, desc[k].noise_b = items[k], IMAP_MODES[mode], int(bool(negate)), noise_index[k]
        desc[k].a, desc[k].s = a[k], s[k]
        desc[k].seed_lo, desc[k].seed_hi = keys[k] & 0xFFFFFFFF, keys[k] >> 32
        desc[k].off_lo, desc[k].off_hi = off & 0xFFFFFFFF, off >> 32
    check(_lib.load().dgtta_intensity_map(ptr(x), ptr(out), b, d * h * w, desc, n, ptr(stats) if mode != "linear" else None,
                                          ptr(stats2) if mode == "restore" else None, stream_of(x.device)), "dgtta_intensity_map")
    return out


def gauss_blur_taps(sigma):
    """(radius, taps) of scipy.ndimage.gaussian_filter(sigma, truncate=4) for 0 < sigma <= 1: radius = int(4 sigma + 0.5) in
    1 .. 4 (sigma < 0.125 keeps the one-voxel radius the kernel needs; its outer taps are then below 1e-13),
    taps = exp(-x^2 / (2 sigma^2)) / sum in float64, rounded to float32."""
    import numpy as np
    sigma = float(sigma)
    if not 0.0 < sigma <= 1.0:        # false for NaN
        raise ValueError(f"gauss_blur3: sigma {sigma} outside (0, 1]")
    radius = max(int(4.0 * sigma + 0.5), 1)
    xs = np.arange(-radius, radius + 1, dtype=np.float64)
    t = np.exp(-0.5 / (sigma * sigma) * xs ** 2)
    return radius, (t / t.sum()).astype(np.float32)


def gauss_blur3(x, items, sigmas, out=None, scratch=None):
    """scipy.ndimage.gaussian_filter(x[item, 0], sigma, mode="reflect", truncate=4) for the items `items` of the batch x
    [B, 1, D, H, W] (float32) with one sigma in (0, 1] each, separable in fp32 (csrc/intensity_aug.hip; three launches).
    Writes `out` (default: x itself, in place); `scratch`: a float32 tensor of x's shape that is neither x nor out (allocated
    when not given).  Items that are not named are neither read nor written.  Returns out."""
    name = "gauss_blur3"
    b, d, h, w = _intensity_batch(x, name)
    items = _intensity_items(items, b, name)
    sigmas = list(sigmas)
    if len(sigmas) != len(items):
        raise ValueError(f"{name}: one sigma per item expected")
    out = _intensity_out(x, out, name)
    if scratch is None:
        scratch = torch.empty_like(x)
    else:
        _intensity_batch(scratch, name, "scratch")
        if scratch.shape != x.shape or scratch.device != x.device or scratch.data_ptr() in (x.data_ptr(), out.data_ptr()):
            raise ValueError(f"{name}: `scratch` must have x's shape and device and be a buffer of its own")
    desc = (_lib.BlurItem * len(items))()
    for k, (item, sigma) in enumerate(zip(items, sigmas)):
        radius, taps = gauss_blur_taps(sigma)
        desc[k].item, desc[k].radius = item, radius
        desc[k].taps[:len(taps)] = taps.tolist()
    check(_lib.load().dgtta_gauss_blur3(ptr(x), ptr(out), ptr(scratch), b, d, h, w, desc, len(items), stream_of(x.device)),
          "dgtta_gauss_blur3")
    return out


# ------------------------------------------------------------------------------------------------ dataset fingerprint
FP_BINS, FP_MAX_PREFIXES = _lib.FP_BINS, _lib.FP_MAX_PREFIXES
_FP_SEG = {torch.uint8: _lib.SEG_U8, torch.int16: _lib.SEG_I16, torch.int32: _lib.SEG_I32}


def fingerprint_state(device):
    """The initial running state of the moment sweeps: an int64 tensor [7] holding DgttaFingerprintState of include/dgtta.h
    (count, nonfinite, first_nonfinite_case as integers; min, max, sum, sumsq_centred as the bits of doubles)."""
    s = torch.zeros(7, dtype=torch.float64)
    s[3], s[4] = float("inf"), float("-inf")
    s = s.view(torch.int64)
    s[2] = -1
    return s.to(device)


def fingerprint_read_state(state):
    """The state as a dict of Python numbers (one copy from the device)."""
    i = state.cpu()
    f = i.view(torch.float64)
    return {"count": int(i[0]), "nonfinite": int(i[1]), "first_nonfinite_case": int(i[2]), "min": float(f[3]), "max": float(f[4]),
            "sum": float(f[5]), "sumsq_centred": float(f[6])}


def fingerprint_counters(device, n_prefixes=1):
    """Zeroed running histogram of a sweep: int64 [n_prefixes, FP_BINS] (the kernels count in unsigned 64 bits)."""
    return torch.zeros((int(n_prefixes), FP_BINS), dtype=torch.int64, device=device)


def fingerprint_ws_bytes(voxels, n_prefixes):
    return int(_lib.load().dgtta_fingerprint_ws_bytes(int(voxels), int(n_prefixes)))


def fingerprint_sweep(x, seg, counters, prefix_bits=0, digit_bits=11, prefixes=None, moment=0, state=None, mean=0.0, case_index=0,
                      ws=None):
    """One case of one fingerprint sweep (csrc/fingerprint.hip).  x: float32 CUDA tensor, seg: uint8 / int16 / int32 labels of the
    same number of voxels; foreground is seg > 0.  counters [len(prefixes), FP_BINS] (int64, the caller's running histogram)
    grows by the digit histogram - the `digit_bits` key bits after the leading `prefix_bits` - of the finite foreground values
    whose key starts with one of `prefixes` (prefix_bits = 0: of all of them).  moment 1 / 2 adds the case to `state`
    (fingerprint_state): count, min, max, sum and non-finite count / the sum of (x - mean)^2.  Nothing is read back."""
    name = "fingerprint_sweep"
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"{name}: `x` must be a non-empty contiguous float32 CUDA tensor (there is no CPU fallback)")
    if not isinstance(seg, torch.Tensor) or seg.device != x.device or seg.dtype not in _FP_SEG or not seg.is_contiguous() or \
            seg.numel() != x.numel():
        raise ValueError(f"{name}: `seg` must be a contiguous uint8 / int16 / int32 tensor of x's size on x's device")
    prefix_bits, digit_bits, moment = int(prefix_bits), int(digit_bits), int(moment)
    if prefix_bits != 0 and prefixes is None:
        raise ValueError(f"{name}: a prefix of {prefix_bits} bits needs `prefixes`")
    prefixes = [0] if prefix_bits == 0 else [int(p) for p in prefixes]
    n = len(prefixes)
    if not 1 <= n <= FP_MAX_PREFIXES or len(set(prefixes)) != n or any(not 0 <= p < 2 ** 32 for p in prefixes):
        raise ValueError(f"{name}: 1..{FP_MAX_PREFIXES} distinct 32-bit prefixes expected (got {prefixes})")
    if not isinstance(counters, torch.Tensor) or counters.device != x.device or counters.dtype != torch.int64 or \
            not counters.is_contiguous() or tuple(counters.shape) != (n, FP_BINS):
        raise ValueError(f"{name}: `counters` must be a contiguous int64 tensor [{n}, {FP_BINS}] on x's device")
    if moment not in (0, 1, 2):
        raise ValueError(f"{name}: moment {moment} not in (0, 1, 2)")
    if moment and (not isinstance(state, torch.Tensor) or state.device != x.device or state.dtype != torch.int64 or
                   not state.is_contiguous() or state.numel() != 7):
        raise ValueError(f"{name}: `state` must be the int64 tensor [7] of fingerprint_state on x's device")
    need = fingerprint_ws_bytes(x.numel(), n)
    if ws is None:
        ws = _ws(need, x.device)
    elif not ws.is_cuda or ws.device != x.device or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need:
        raise ValueError(f"{name}: `ws` is a contiguous uint8 CUDA tensor of at least {need} bytes")
    h_pre = (C.c_uint32 * n)(*prefixes)
    check(_lib.load().dgtta_fingerprint_sweep(ptr(x), ptr(seg), _FP_SEG[seg.dtype], x.numel(), moment, float(mean), int(case_index),
                                              prefix_bits, digit_bits, h_pre, n, ptr(counters), ptr(state) if moment else None, ptr(ws),
                                              ws.numel(), stream_of(x.device)), "dgtta_fingerprint_sweep")
    return counters


# ------------------------------------------------------------------------------------------------ resampling
def resize_volume(x, new_shape, order, axes=None):
    """skimage.transform.resize(x[c], new_shape, order, mode='edge', anti_aliasing=False, clip=False) for every leading
    index c, on the GPU: x [..., X, Y, Z] (any float dtype, CUDA) -> double [..., *new_shape].  `axes`: subset of the
    three trailing axes to resample (others must keep their size).  One separable pass per axis (csrc/resample.hip)."""
    require_cuda(x)
    lib = _lib.load()
    cur = x.double().contiguous()
    lead = cur.shape[:-3]
    outer0 = 1
    for s in lead:
        outer0 *= int(s)
    for ax in (range(3) if axes is None else axes):
        shp = list(cur.shape[-3:])
        n, m = shp[ax], int(new_shape[ax])
        if n == m:
            continue
        inner = 1
        for s in shp[ax + 1:]:
            inner *= s
        outer = outer0
        for s in shp[:ax]:
            outer *= s
        out_shape = shp[:ax] + [m] + shp[ax + 1:]
        dst = torch.empty((*lead, *out_shape), dtype=torch.float64, device=cur.device)
        nbytes = lib.dgtta_resample_axis_ws_bytes(outer, n, inner, int(order))
        ws = _ws(nbytes, cur.device)
        check(lib.dgtta_resample_axis(ptr(cur), ptr(dst), ptr(ws), nbytes, outer, n, m, inner, int(order),
                                      stream_of(cur.device)), "dgtta_resample_axis")
        cur = dst
    return cur
