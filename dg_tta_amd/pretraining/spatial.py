"""nnU-Net's rotation / scaling augmentation for `dgtta pretrain --augmentation spatial`: the host side - what is drawn per
batch item and the voxel map the sampler (ops.sample_patches_aug, csrc/spatial_aug.hip) is given.  Restated from memory of
nnunetv2 2.2's training transforms / batchgenerators' SpatialTransform (UNPINNED, like the trainer around it):

  * per batch item, independently: rotation with probability 0.2, scaling with probability 0.2; no elastic deformation, no
    mirroring (the DG trainers switch mirroring off);
  * rotation: three angles, each U(-30 deg, 30 deg), matrix Rx @ Ry @ Rz about the patch centre, axes in (D, H, W) order.
    For an anisotropic patch (max(patch) / min(patch) > 3, nnU-Net's "dummy 2D" rule) ONE angle U(-180 deg, 180 deg) about the
    thin axis (the shortest patch axis), and scaling acts in the plane only: the thin axis' row and column of the matrix
    stay (1, 0, 0);
  * scaling: one factor for all axes from (0.7, 1.4): with probability 0.5 from [0.7, 1], else from [1, 1.4].  The factor
    multiplies the patch grid: > 1 makes the patch cover more of the volume (the content appears smaller).

Random stream: every draw comes from utils.numpy_rng() (or the generator handed in), per item in this fixed order -
  1. u ~ U(0, 1): rotation happens iff u < p_rotation;
  2. if it does: the three angles in the order x (D axis), y (H), z (W) - or the one in-plane angle;
  3. u ~ U(0, 1): scaling happens iff u < p_scaling;
  4. if it does: u ~ U(0, 1) picks the side (u < 0.5: [0.7, 1]), then the factor ~ U(side);
so `--seed` reproduces a run.  Host arithmetic only, float64."""
import math

import numpy as np

from ..utils import numpy_rng

ANISOTROPY_THRESHOLD = 3.0


def rotation_matrix(ax, ay, az):
    """Rx(ax) @ Ry(ay) @ Rz(az), angles in radians, x = the first array axis (D)."""
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return rx @ ry @ rz


def thin_axis(patch):
    """The axis nnU-Net's dummy-2D rule leaves alone: the shortest one when max(patch) / min(patch) > 3, else None."""
    patch = [int(p) for p in patch]
    if max(patch) / min(patch) > ANISOTROPY_THRESHOLD:
        return int(np.argmin(patch))
    return None


class SpatialAugmentation:
    """The draw.  draw(patch) -> None when neither event fired (the item is then cropped, as nnU-Net crops it), else the
    3 x 3 matrix A in voxel units, (D, H, W) order, float64.  last = (angles in radians | None, factor | None) of the latest
    draw, for tests and logs."""

    def __init__(self, p_rotation=0.2, p_scaling=0.2, rotation=(-30.0, 30.0), rotation_in_plane=(-180.0, 180.0),
                 scaling=(0.7, 1.4)):
        if not (scaling[0] <= 1.0 <= scaling[1] and scaling[0] > 0):
            raise ValueError(f"scaling range {scaling}: 0 < low <= 1 <= high expected")
        self.p_rotation, self.p_scaling = float(p_rotation), float(p_scaling)
        self.rotation, self.rotation_in_plane, self.scaling = tuple(rotation), tuple(rotation_in_plane), tuple(scaling)
        self.last = (None, None)

    def draw(self, patch, rng=None):
        rng = numpy_rng() if rng is None else rng
        thin = thin_axis(patch)
        angles = factor = None
        if rng.uniform() < self.p_rotation:
            if thin is None:
                angles = tuple(math.radians(rng.uniform(*self.rotation)) for _ in range(3))
            else:
                angles = (math.radians(rng.uniform(*self.rotation_in_plane)),)
        if rng.uniform() < self.p_scaling:
            lo, hi = (self.scaling[0], 1.0) if rng.uniform() < 0.5 else (1.0, self.scaling[1])
            factor = float(rng.uniform(lo, hi))
        self.last = (angles, factor)
        if angles is None and factor is None:
            return None
        if thin is None:
            rot = rotation_matrix(*angles) if angles is not None else np.eye(3)
            return rot * (1.0 if factor is None else factor)
        a = np.eye(3)
        plane = [i for i in range(3) if i != thin]
        c, s = (math.cos(angles[0]), math.sin(angles[0])) if angles is not None else (1.0, 0.0)
        f = 1.0 if factor is None else factor
        a[np.ix_(plane, plane)] = f * np.array([[c, -s], [s, c]])
        return a


def patch_start(center, shape, patch):
    """Integer start of the patch centred on voxel `center`: clamp(center - p // 2, 0, shape - p), the start
    torch_utils.center_to_offset encodes; on an axis where the volume is smaller than the patch the centred integer start
    -((p - shape) // 2)."""
    out = []
    for c, s, p in zip(center, shape, patch):
        c, s, p = int(c), int(s), int(p)
        out.append(-((p - s) // 2) if s < p else min(max(c - p // 2, 0), s - p))
    return out


def sampling_map(a, start, patch):
    """The 3 x 4 [A | t] of x(v) = s + (P - 1) / 2 + A (v - (P - 1) / 2), computed in float64 and rounded to fp32 (returned as
    float32).  With A = I, t = s exactly; with a signed permutation and patch extents of one parity every entry is an integer."""
    a = np.asarray(a, dtype=np.float64).reshape(3, 3)
    c = (np.asarray(patch, dtype=np.float64) - 1.0) / 2.0
    t = np.asarray(start, dtype=np.float64) + c - a @ c
    return np.concatenate([a, t[:, None]], axis=1).astype(np.float32)
