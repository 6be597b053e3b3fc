"""CPU restatement of the deformable spatial augmentation (steps 1-3 of the feature: random field, inverse-consistent
integration, the two dense-grid warps of a branch) in plain torch, at the precision of its inputs.  In fp32 it reproduces
tests/golden/deformable*.npz bit for bit (tests/test_deformable_fields.py); in fp64 it is the yardstick against which both
the fp32 restatement and the HIP kernels are measured (tests/test_gpu_deformable.py)."""
import numpy as np
import torch
import torch.nn.functional as F

BOX = 5             # calc_branch: interpolation_factor=5
FACTOR = 0.5        # calc_branch: factor=0.5
TIME_STEPS = 5      # get_disp_field: STEPS = 5


def hash_noise(shape, salt):
    """Deterministic pseudo-noise with zero mean and unit variance, from integer arithmetic only (the same bits on every
    machine and torch version, so inputs need not be stored in the fixtures).  Returned as float64."""
    n = int(np.prod(shape))
    h = (np.arange(n, dtype=np.uint64) + np.uint64(salt) * np.uint64(1000003)) * np.uint64(2654435761)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    u = (h & np.uint64(0xFFFFFF)).astype(np.float64) / float(1 << 24)          # [0, 1), 24 bits: exact in fp32 too
    return torch.from_numpy((u - 0.5) * np.sqrt(12.0)).reshape(shape)


def rf_field(draw, size_3d):
    """Low-resolution noise [B,F,d,h,w] -> smooth fields [B,F,D,H,W] of zero mean and unit (1e-3 + std)."""
    x = draw
    for _ in range(3):
        x = F.avg_pool3d(x, BOX, stride=1, padding=BOX // 2)
    x = F.interpolate(x, size=tuple(size_3d), mode="trilinear")
    x = x - x.mean((-3, -2, -1), keepdim=True)
    b, f = x.shape[:2]
    return x / (1e-3 + x.reshape(b * f, -1).std(1).reshape(b, f, 1, 1, 1))


def diffeo_fields(field, factor=FACTOR, time_steps=TIME_STEPS):
    """Smooth fields [B,3,D,H,W] -> (disp, inverse), both [B,D,H,W,3].  Channel c is divided by the c-th of (D, H, W) although
    it displaces the c-th of (x, y, z): kept as the reference has it."""
    b, _, d, h, w = field.shape
    dims = torch.tensor([d, h, w]).reshape(1, 3, 1, 1, 1)
    ident = F.affine_grid(torch.eye(3, 4)[None], (1, 1, d, h, w), align_corners=True).permute(0, 4, 1, 2, 3).to(field)
    fwd = (field * factor) / dims / (2 ** time_steps) * (1.0 / time_steps)
    inv = torch.zeros_like(fwd)

    def pull(src, by):
        return F.grid_sample(src, (ident + by).permute(0, 2, 3, 4, 1), padding_mode="border", align_corners=True)

    for _ in range(time_steps):
        fwd, inv = 0.5 * fwd - 0.5 * pull(inv, fwd), 0.5 * inv - 0.5 * pull(fwd, inv)
    fwd = fwd * 2 ** time_steps * dims
    inv = inv * 2 ** time_steps * dims
    return fwd.permute(0, 2, 3, 4, 1).contiguous(), inv.permute(0, 2, 3, 4, 1).contiguous()


def disp_fields(draw, size_3d):
    return diffeo_fields(rf_field(draw, size_3d))


def dense_warp(src, disp, padding_mode):
    """A branch's grid algebra: grid = (0 * identity + disp) + identity, sampled with align_corners=False."""
    b = src.shape[0]
    ident = F.affine_grid(torch.eye(3, 4)[None].repeat(b, 1, 1), [b, 1] + list(src.shape[2:]), align_corners=False).to(src)
    return F.grid_sample(src, (0.0 * ident + disp.to(src)) + ident, padding_mode=padding_mode, align_corners=False)


def warp_and_grad(logits, inverse, weight):
    """Zero-padded warp of the logits through the inverse field and d sum(weight * warped) / d logits."""
    logits = logits.clone().requires_grad_(True)
    out = dense_warp(logits, inverse, "zeros")
    (out * weight).sum().backward()
    return out.detach(), logits.grad
