"""Spatial augmentation parameters - mirrors dg_tta/tta/augmentation_utils.py: get_rand_affine (:156-170) and the
deformable path get_rf_field (:8-43) -> calc_consistent_diffeomorphic_field (:46-135) as get_disp_field (:138-153)
composes them.  The reference's get_disp_field raises TypeError because it hands get_rf_field a keyword
(`alternating_fields`) that function does not take; everything it calls is intact, so the composition is reproduced here as
written with that one keyword dropped.  The arithmetic runs in csrc/deform.hip; only the draws are made here (on the
device generator, where the reference draws them)."""
import torch

from .. import ops
from ..utils import cpu_generator, device_generator


def get_rand_affine(batch_size, strength=0.05, flip=False):
    """theta = I(3x4) + strength*randn (CPU generator, like the reference) and its inverse; both [B,3,4] on the CPU."""
    top = torch.randn(batch_size, 3, 4, generator=cpu_generator()) * strength + torch.eye(3, 4).unsqueeze(0)
    bottom = torch.tensor([0, 0, 0, 1]).view(1, 1, 4).repeat(batch_size, 1, 1)
    affine = torch.cat((top, bottom), 1)
    if flip:
        signs = torch.cat([(2 * (torch.rand(3, generator=cpu_generator()) > 0.5).float() - 1), torch.tensor([1.0])])
        affine = affine @ torch.diag(signs)
    return affine[:, :3], affine.inverse()[:, :3]


def low_res_size(size_3d, interpolation_factor):
    """Shape of get_rf_field's draw.  avg_pool3d refuses an input smaller than its kernel, so every patch axis must be at
    least interpolation_factor^2 voxels (25 for the factor 5 that calc_branch uses): checked here, before any launch."""
    k = int(interpolation_factor)
    if k < 1 or k % 2 == 0:
        raise NotImplementedError(f"deformable augmentation: interpolation_factor must be odd (got {interpolation_factor}); "
                                  "an even box filter changes the size of the low-resolution field")
    size_3d = [int(v) for v in size_3d]
    if len(size_3d) != 3 or min(size_3d) // k < k:
        raise ValueError(f"deformable augmentation needs every patch axis >= {k * k} voxels (size // {k} >= {k}, the box "
                         f"filter of the random field); got patch size {size_3d}")
    return tuple(v // k for v in size_3d)


def draw_field_noise_(slot):
    """get_rf_field's torch.randn draw, written in place (device generator, as the reference).  A function of its own so that
    parity tests can route it through the CPU generator, like mind.draw_noise_."""
    return slot.normal_(generator=device_generator())


def get_rf_field(num_batch, size_3d, interpolation_factor=4, num_fields=4, device="cpu", draw=None):
    """Smooth random fields [num_batch, num_fields, D, H, W] with zero mean and unit (1e-3 + std) each.
    draw: the pre-drawn low-resolution noise [num_batch, num_fields, D//k, H//k, W//k] (else drawn on `device`)."""
    low = low_res_size(size_3d, interpolation_factor)
    if draw is None:
        draw = draw_field_noise_(torch.empty((num_batch, num_fields) + low, dtype=torch.float32, device=device))
    elif tuple(draw.shape) != (num_batch, num_fields) + low:
        raise ValueError(f"get_rf_field: draw has shape {tuple(draw.shape)}, expected {(num_batch, num_fields) + low}")
    return ops.rf_field(draw, size_3d, box=interpolation_factor)


def calc_consistent_diffeomorphic_field(disp_field, inverse_disp_field=None, time_steps=1, ensure_inverse_consistency=True,
                                        iter_steps_override=None):
    """The inverse-consistent fixed-point iteration on disp_field [B,3,D,H,W] with the inverse starting at zero (the only
    use the reference makes of it).  Returns (disp, inverse) as [B,3,D,H,W] views of channel-last memory."""
    if not ensure_inverse_consistency or iter_steps_override:
        raise NotImplementedError("only ensure_inverse_consistency=True without iter_steps_override is provided")
    if inverse_disp_field is not None and bool((inverse_disp_field != 0).any()):
        raise NotImplementedError("the inverse field must start at zero (as get_disp_field passes it)")
    disp, inverse = ops.diffeo_fields(disp_field, 1.0, time_steps)
    return disp.permute(0, 4, 1, 2, 3), inverse.permute(0, 4, 1, 2, 3)


def get_disp_field(batch_num, size_3d, factor=0.1, interpolation_factor=5, device="cpu", draw=None):
    """(grid_deformable, grid_deformable_inverse), both [B,D,H,W,3] in normalised grid units: a smooth random displacement
    (unit-variance fields scaled by `factor`, five inverse-consistent integration steps) and its approximate inverse.
    draw: the pre-drawn low-resolution noise [B,3,D//k,H//k,W//k] (tests feed a recorded one)."""
    field = get_rf_field(batch_num, size_3d, interpolation_factor=interpolation_factor, num_fields=3, device=device, draw=draw)
    return ops.diffeo_fields(field, factor, time_steps=5)
