"""Float64 numpy restatement of the region end of the export loop (csrc/resample.hip dgtta_regions_merge_f64,
inference._RunningRegions / export_region_probabilities / _paste_label_map):

  merge_groups     the label map over class groups merged in ascending c0: label = 0, then order[c0 + j] where vals[v][j] > 0
  stable_sigmoid   1 / (1 + exp(-x)) for x >= 0, e / (1 + e) with e = exp(x) otherwise - the branch that never overflows
  region_export    both ends of one [V, R] array of SUMMED logits: labels of the sum, sigmoid of scale * sum
  paste_full       outside the crop box label 0 and probability 0; then transpose_backward on the spatial axes
  prob_bound       the derived bound of a stored probability: one unit in the last place of the output type at the float64 value

tests/test_region_export_ref.py licenses it against an explicit voxel loop of nnU-Net's rule and against tests/region_ref.py."""
import numpy as np


def merge_groups(vals, order, group):
    """vals [V, R] float64 (any positive multiple of the mean logits), merged in groups of `group` outputs as the export loop does:
    int32 [V].  0, -0.0 and NaN are not positive."""
    vals = np.asarray(vals, dtype=np.float64)
    V, R = vals.shape
    label = np.zeros(V, dtype=np.int32)
    for c0 in range(0, R, group):
        for j in range(min(group, R - c0)):
            label[vals[:, c0 + j] > 0] = int(order[c0 + j])
    return label


def stable_sigmoid(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(under="ignore"):      # (exp(-745) is a subnormal; nothing here can overflow)
        e = np.exp(-np.abs(x))
        return np.where(np.isnan(x), np.nan, np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)))


def region_export(vals, order, scale, group=8):
    """(label int32 [V], probs float64 [R, V]) of summed logits vals [V, R]: p = sigmoid(scale * vals), plane-major."""
    vals = np.asarray(vals, dtype=np.float64)
    return merge_groups(vals, order, group), stable_sigmoid(scale * vals).T.copy()


def paste_full(seg, probs, shape_before_cropping, bbox, transpose_backward):
    """(label int64, probs float64 [R, ...]) in the original geometry: zeros outside the crop box."""
    full = tuple(int(v) for v in shape_before_cropping)
    sl = tuple(slice(int(a), int(b)) for a, b in bbox)
    fs = np.zeros(full, dtype=np.int64)
    fp = np.zeros((len(probs), *full), dtype=np.float64)
    fs[sl] = seg
    fp[(slice(None), *sl)] = probs
    tb = list(transpose_backward)
    return fs.transpose(tb), fp.transpose([0] + [a + 1 for a in tb])


def prob_bound(want, dtype):
    """One unit in the last place of `dtype` (np.float16 / np.float32) at the float64 value `want`, floored at the type's smallest
    subnormal (2^-24 / 2^-149): the double evaluation errs by a few 1e-16, the final rounding by half a unit.  NaN where want is NaN."""
    want = np.asarray(want, dtype=np.float64)
    mant, emin, floor = {np.float16: (10, -14, 2.0 ** -24), np.float32: (23, -126, 2.0 ** -149)}[dtype]
    with np.errstate(divide="ignore", invalid="ignore"):
        ex = np.floor(np.log2(np.abs(want)))
    ex = np.where(np.isfinite(ex), np.maximum(ex, emin), emin)
    return np.where(np.isnan(want), np.nan, np.maximum(2.0 ** (ex - mant), floor))
