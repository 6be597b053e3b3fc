"""Writes tests/golden/deformable.npz and deformable_logits.npz from the reference implementation (development machine
only: needs the reference checkout, path in DG_TTA_REFERENCE or the first argument).

The reference's get_disp_field cannot be called (it passes get_rf_field a keyword that function does not take), so its two
intact functions are composed here exactly as it composes them.  Arrays only.  The inputs that are not random draws (image,
logits, loss weights) come from tests/deformable_ref.hash_noise and are not stored; two files keep each under 1 MiB."""
import os
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, os.environ.get("DG_TTA_REFERENCE") or sys.argv[1])

from deformable_ref import hash_noise  # noqa: E402
from dg_tta.tta import augmentation_utils as ref  # noqa: E402

SIZE = [25, 27, 30]
CLASSES = 5


def main():
    torch.manual_seed(20261016)
    state = torch.get_rng_state()
    draw = torch.randn(1, 3, *[s // 5 for s in SIZE])
    torch.set_rng_state(state)          # get_rf_field draws for itself: hand it the same stream
    field = ref.get_rf_field(1, SIZE, num_fields=3, interpolation_factor=5)
    disp, inv = ref.calc_consistent_diffeomorphic_field(field * 0.5, torch.zeros_like(field), 5,
                                                        ensure_inverse_consistency=True)
    disp, inv = disp.permute(0, 2, 3, 4, 1), inv.permute(0, 2, 3, 4, 1)
    # the two grid_sample calls of calc_branch (tta.py:520-575) with their grid algebra
    identity = F.affine_grid(torch.eye(3, 4)[None], [1, 1] + SIZE, align_corners=False)
    zero = 0.0 * identity
    image = hash_noise([1, 1] + SIZE, 1).float()
    image_warped = F.grid_sample(image, (zero + disp) + identity, padding_mode="border", align_corners=False)
    logits = hash_noise([1, CLASSES] + SIZE, 2).float().requires_grad_(True)
    weight = hash_noise([1, CLASSES] + SIZE, 3).float()
    logits_warped = F.grid_sample(logits, (zero + inv) + identity, align_corners=False)
    (logits_warped * weight).sum().backward()
    np.savez(HERE / "deformable.npz", size=np.array(SIZE), draw=draw.numpy(), field=field.numpy(),
             disp=disp.contiguous().numpy(), inverse=inv.contiguous().numpy(), image_warped=image_warped.numpy())
    np.savez(HERE / "deformable_logits.npz", logits_warped=logits_warped.detach().numpy(), logits_grad=logits.grad.numpy())
    for f in ("deformable.npz", "deformable_logits.npz"):
        print(f, (HERE / f).stat().st_size, "bytes")
    print("zero-padding share of the logits warp:", float((logits_warped == 0).float().mean()))


if __name__ == "__main__":
    main()
