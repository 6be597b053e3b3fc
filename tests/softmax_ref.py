"""Float64 restatement of the softmax end of the ensemble prediction (include/dgtta.h, "Softmax end of the ensemble prediction";
nnU-Net's save_probabilities definitions from memory, UNPINNED) and the rounding bounds the GPU tests hold the kernels to.

For voxel v, members m = 1..M, classes c:
    l_c = (sum_m W_m[c] . F_m(v) + n(v) bsum[c]) / (M n(v)),  p = softmax(l),  label = first argmax,
    confidence = p[label] = 1 / S,  entropy = ln S - D / S  with S = sum exp(l - l_max), D = sum (l - l_max) exp(l - l_max).

Bounds (u = 2^-24; everything per voxel, in float64, from the fp32 arrays the kernels read):
  * logit: a dot product of 32 M + 1 fp32 terms and one scale (the scale 1 / (M n) is rounded once and applied with one
    multiplication): |l - l_ref| <= delta = (32 M + 3) u (sum_m sum_k |w| |f| + n |bsum|) / (M n), whatever the summation order.
    delta(v) below is the maximum over the classes of the voxel.
  * probability: both the numerator and S move by at most exp(+-delta): p_ref (exp(2 delta) - 1).  The fp32 evaluation adds
    KAPPA u p_ref (1 + |x|), x = l - l_max: the subtraction and the exponential's argument reduction are relative to |x| (1 each),
    the exponential itself (2 ulp), the division (2: reciprocal and product) and the sums of S - a lane adds its 16 ceil(C / 32)
    classes, then the two lane halves: NL = 16 ceil(C / 32) + 1 roundings at most, in whatever order.  KAPPA = 4 + NL.
    Below 2^-126 fp32 results are subnormal or flushed: + 2^-126 absolute.  float16 storage adds 2^-11 p + 2^-25.
  * entropy: dH / dl_c = -p_c (ln p_c + H), so the logit error contributes delta sum_c p_c |ln p_c + H|; the fp32 evaluation
    KAPPA u (sum_c p_c |ln p_c + H| (1 + |x_c|) + 1 + ln S + sum_c p_c |x_c|): the same relative errors of the exponentials seen
    through the same derivative, the rounding of x inside D, and the roundings of S (absolute u near S = 1), the logarithm, the
    quotient and the final difference against the magnitudes of the two terms.
The tests assert err <= 2 x bound (the factor covers second-order terms); the measured max(err / bound) is in DESIGN.md."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126


def kappa(C):
    return 4 + 16 * ((C + 31) // 32) + 1


def head_logits(facc, nsum, w, bsum):
    """facc [M,V,32], nsum [V], w [M,C,32], bsum [C] (the fp32 arrays the kernel reads) -> (l [V,C], delta [V]) in float64."""
    facc, nsum, w, bsum = (np.asarray(a, dtype=np.float64) for a in (facc, nsum, w, bsum))
    M = facc.shape[0]
    s = np.einsum("mvk,mck->vc", facc, w) + nsum[:, None] * bsum[None]
    mag = np.einsum("mvk,mck->vc", np.abs(facc), np.abs(w)) + nsum[:, None] * np.abs(bsum)[None]
    mn = (M * nsum)[:, None]
    return s / mn, ((32 * M + 3) * U * mag / mn).max(axis=1)


def softmax_stats(l):
    """l [V,C] float64 -> dict(p [V,C], label [V] (first maximum), confidence, entropy, x = l - l_max, lnS)."""
    l = np.asarray(l, dtype=np.float64)
    label = l.argmax(axis=1)
    x = l - l.max(axis=1, keepdims=True)
    e = np.exp(x)
    S = e.sum(axis=1)
    p = e / S[:, None]
    ent = np.log(S) - (x * e).sum(axis=1) / S
    return {"p": p, "label": label, "confidence": 1.0 / S, "entropy": ent, "x": x, "lnS": np.log(S)}


def bounds(st, delta, prob_dtype=np.float32):
    """Rounding bounds of an fp32 evaluation with logit error delta [V] (0: exact logits): (p_bound [V,C], entropy_bound [V])."""
    p, x, H, lnS = st["p"], st["x"], st["entropy"], st["lnS"]
    k = kappa(p.shape[1])
    delta = np.asarray(delta, dtype=np.float64)
    pb = p * np.expm1(2.0 * delta)[:, None] + k * U * p * (1.0 + np.abs(x)) + TINY
    if np.dtype(prob_dtype) == np.float16:
        pb = pb + 2.0 ** -11 * p + 2.0 ** -25
    sens = p * np.abs((x - lnS[:, None]) + H[:, None])      # p_c |ln p_c + H|
    hb = delta * sens.sum(axis=1) + k * U * ((sens * (1.0 + np.abs(x))).sum(axis=1) + 1.0 + lnS + (p * np.abs(x)).sum(axis=1))
    return pb, hb + p.shape[1] * 128 * TINY


def f64_path_bounds(st, delta, prob_dtype=np.float32):
    """Bounds of the class-group path, which evaluates in float64 and rounds once on the way out: logit error delta [V] or scalar
    (0 when the reference uses the very values the path formed), 64 float64 roundings (2^-53) for the merge and finalize
    arithmetic, then the storage rounding - float32 2^-24 relative (2^-149 absolute below the normal range), float16
    2^-11 p + 2^-25.  -> (p_bound [V,C], entropy_bound [V])."""
    p, x, H, lnS = st["p"], st["x"], st["entropy"], st["lnS"]
    delta = np.broadcast_to(np.asarray(delta, dtype=np.float64), H.shape)
    e64 = 64 * 2.0 ** -53
    pb = p * np.expm1(2.0 * delta)[:, None] + e64 * p * (1.0 + np.abs(x))
    pb = pb + (2.0 ** -11 * p + 2.0 ** -25 if np.dtype(prob_dtype) == np.float16 else U * p + 2.0 ** -149)
    sens = p * np.abs((x - lnS[:, None]) + H[:, None])
    hb = delta * sens.sum(axis=1) + e64 * ((sens * (1.0 + np.abs(x))).sum(axis=1) + 1.0 + lnS + (p * np.abs(x)).sum(axis=1))
    return pb, hb + U * H + 2.0 ** -149


def online_merge(groups, scale, sel):
    """The class-group form in plain numpy: groups = [(c0, vals [V,cg])] in any order, l = scale * vals.  Running maximum m,
    S = sum exp(l - m), D = sum (l - m) exp(l - m), rescaled when the maximum moves.  -> (confidence, entropy, P [K,V])."""
    V = groups[0][1].shape[0]
    m, S, D = np.full(V, -np.inf), np.zeros(V), np.zeros(V)
    stash = np.zeros((len(sel), V))
    for c0, vals in groups:
        lg = scale * np.asarray(vals, dtype=np.float64)
        m2 = np.maximum(m, lg.max(axis=1))
        with np.errstate(invalid="ignore"):
            d = np.where(np.isfinite(m), m - m2, 0.0)
        r = np.where(np.isfinite(m), np.exp(d), 0.0)
        D = r * (D + d * S)
        S = r * S
        m = m2
        x = lg - m[:, None]
        e = np.exp(x)
        S = S + e.sum(axis=1)
        D = D + (x * e).sum(axis=1)
        for k, c in enumerate(sel):
            if c0 <= c < c0 + lg.shape[1]:
                stash[k] = lg[:, c - c0]
    return 1.0 / S, np.log(S) - D / S, np.exp(stash - m[None]) / S[None]


def paste_full(seg, probs, conf, ent, sel, shape_before_cropping, bbox, transpose_backward):
    """The original-geometry convention: outside the crop box label 0, p[class 0] = 1, every other class 0, confidence 1,
    entropy 0; then transpose_backward on the spatial axes."""
    full = tuple(int(v) for v in shape_before_cropping)
    sl = tuple(slice(int(a), int(b)) for a, b in bbox)
    fs = np.zeros(full, dtype=np.int64)
    fp = np.zeros((len(sel), *full), dtype=np.float64)
    if 0 in sel:
        fp[list(sel).index(0)] = 1.0
    fc, fe = np.ones(full), np.zeros(full)
    fs[sl], fc[sl], fe[sl] = seg, conf, ent
    fp[(slice(None), *sl)] = probs
    tb = list(transpose_backward)
    return fs.transpose(tb), fp.transpose([0] + [a + 1 for a in tb]), fc.transpose(tb), fe.transpose(tb)
