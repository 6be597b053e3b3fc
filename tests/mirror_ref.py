"""float64 / torch restatement of nnU-Net's mirroring (test infrastructure; nnunetv2 2.2.1 / batchgenerators from memory, UNPINNED):
the subset order of the predictor's mirrored passes, the mean over mirrors, the window gather and the mirrored Gaussian
accumulation.  Masks: bit a set = axis a of a [D][H][W] block flipped."""
import torch

SUBSET_ORDER = ((), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2))


def subsets(axes):
    """The subsets of the allowed axes in the order the predictor runs them."""
    axes = () if axes is None else tuple(axes)
    return [s for s in SUBSET_ORDER if all(a in axes for a in s)]


def mask_of(subset):
    return sum(1 << a for a in subset)


def axes_of(mask):
    return tuple(a for a in range(3) if mask >> a & 1)


def flip(t, mask, first=-3):
    """t flipped along the spatial axes of `mask`; `first` is the index of spatial axis 0 (default: the last three dims)."""
    dims = [first + a for a in axes_of(mask)]
    return t.flip(dims) if dims else t


def mirrored(model, axes):
    """x [1, C, D, H, W] -> the mean over the subsets S of flip_S(model(flip_S(x))), in double."""
    def f(x):
        total = None
        for s in subsets(axes):
            m = mask_of(s)
            out = flip(model(flip(x, m)), m).double()
            total = out if total is None else total + out
        return total / len(subsets(axes))
    return f


def gather(volume, origins, masks, patch):
    """[n, C, *patch]: window k = flip(volume[:, origin_k : origin_k + patch])."""
    return torch.stack([flip(volume[:, x:x + patch[0], y:y + patch[1], z:z + patch[2]], m)
                        for (x, y, z), m in zip(origins, masks)])


def accumulate(acc, nsum, absacc, counts, g, z, origin, mask):
    """acc[o + p][c] += g[p] * z[flip(p)][c] in double (z [PD, PH, PW, C], channels last); nsum[o + p] += g[p]; absacc the same
    with absolute values (the error bound's sum of |g z|) and counts the number of contributions per voxel."""
    sl = tuple(slice(o, o + p) for o, p in zip(origin, g.shape))
    zz = flip(z.double(), mask, first=0)
    gd = g.double()
    acc[sl] += gd[..., None] * zz
    absacc[sl] += (gd[..., None] * zz).abs()
    nsum[sl] += gd
    counts[sl] += 1
