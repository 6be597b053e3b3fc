"""The 3x3x3 convolution (padding 1, stride 1 | 2) and the 2x2x2 stride-2 transposed convolution of dg_tta_amd/csrc/conv_*.hip
and convt_*.hip restated in float64 (test infrastructure): torch on the CPU, no autograd, no torch.nn.functional conv - one
matrix product per row of three taps, written out.  Activations are channels last ([B, D, H, W, C]) in and out; weights keep torch's layout
([Cout, Cin, 3, 3, 3]; transposed conv: [Cin, Cout, 2, 2, 2]).

    y[b][vo][co]  = bias[co] + sum_{tap, ci} x[b][s vo + tap - 1][ci] w[co][ci][tap]                (zero padding)
    dx[b][vi][ci] = sum over (tap, vo) with s vo + tap - 1 = vi, and co, of dy[b][vo][co] w[co][ci][tap]
    dw[co][ci][tap] = sum_{b, vo} x[b][s vo + tap - 1][ci] dy[b][vo][co]          db[co] = sum_{b, vo} dy[b][vo][co]
    out[b][2 v + o][co] = bias[co] + sum_ci x[b][v][ci] w[ci][co][o]              (transposed conv, o in {0, 1}^3)

Beside them the anisotropic layers of conv_aniso.hip in the same style (conva_*, convTa_*): kernel (kd, 3, 3) with kd = 1 | 3, padding
(kd // 2, 1, 1), one stride per axis, and the transposed conv with kernel = stride in {1, 2}^3.

The second half is what tests/test_gpu_conv_exact.py, tests/test_gpu_aniso_exact.py and tests/test_conv_ref.py share: operands on
which every kernel must be
EXACT.  x, w and dy are drawn from {-1, 0, 1} and the bias from small integers, so every product is exact, every fp32 partial
sum is an integer far below 2^24 whatever the order, and every output is an integer that bf16 (|v| <= 256) and fp16 hold
exactly: a kernel's result must then torch.equal the float64 one.  The case lists live here so that the CPU test can check
those magnitude conditions for exactly the cases the GPU test runs.
"""
import functools

import torch

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ the operators
def out_extent(n, stride):
    return (n - 1) // stride + 1


def _pad1(x):
    B, D, H, W, C = x.shape
    xp = torch.zeros(B, D + 2, H + 2, W + 2, C, dtype=x.dtype)
    xp[:, 1:-1, 1:-1, 1:-1] = x
    return xp


def _tap_view(xp, kd, kh, kw, out_dims, s):
    """The voxels of the padded input that tap (kd, kh, kw) pairs with the output voxels: [B, Do, Ho, Wo, C]."""
    Do, Ho, Wo = out_dims
    return xp[:, kd:kd + s * (Do - 1) + 1:s, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s]


def _row_view(xp, kd, kh, out_dims, s):
    """The three kw taps of row (kd, kh) at once, [B, Do, Ho, Wo, 3 C] ordered (kw, c): channels last, the three voxels a row of
    taps reads are one contiguous run of 3 C elements (a read-only overlapping view; one matrix product instead of three)."""
    B, _, _, _, C = xp.shape
    sb, sd, sh, sw, sc = xp.stride()
    return xp.as_strided((B, *out_dims, 3 * C), (sb, s * sd, s * sh, s * sw, sc), xp.storage_offset() + kd * sd + kh * sh)


def _rows():
    return [(kd, kh) for kd in range(3) for kh in range(3)]


def conv3_fwd(x, w, bias=None, stride=1):
    B, D, H, W, C = x.shape
    od = tuple(out_extent(n, stride) for n in (D, H, W))
    xp = _pad1(x.to(F64))
    w = w.to(F64)
    y = torch.zeros(B, *od, w.shape[0], dtype=F64)
    for kd, kh in _rows():
        y += _row_view(xp, kd, kh, od, stride) @ w[:, :, kd, kh, :].permute(2, 1, 0).reshape(3 * C, -1)      # [(kw, ci), co]
    return y if bias is None else y + bias.to(F64)


def conv3_dgrad(dy, w, in_dims, stride=1):
    B = dy.shape[0]
    D, H, W = in_dims
    od = tuple(out_extent(n, stride) for n in (D, H, W))
    assert tuple(dy.shape[1:4]) == od
    w = w.to(F64)
    C = w.shape[1]
    dxp = torch.zeros(B, D + 2, H + 2, W + 2, C, dtype=F64)
    for kd, kh in _rows():
        t = dy.to(F64) @ w[:, :, kd, kh, :].permute(0, 2, 1).reshape(-1, 3 * C)                              # [co, (kw, ci)]
        for kw in range(3):
            _tap_view(dxp, kd, kh, kw, od, stride).add_(t[..., kw * C:(kw + 1) * C])
    return dxp[:, 1:-1, 1:-1, 1:-1].contiguous()


def conv3_wgrad(x, dy, stride=1):
    od = tuple(dy.shape[1:4])
    C = x.shape[-1]
    xp = _pad1(x.to(F64))
    g = dy.to(F64).reshape(-1, dy.shape[-1])
    dw = torch.zeros(dy.shape[-1], C, 3, 3, 3, dtype=F64)
    for kd, kh in _rows():
        dw[:, :, kd, kh, :] = (g.t() @ _row_view(xp, kd, kh, od, stride).reshape(-1, 3 * C)).reshape(-1, 3, C).permute(0, 2, 1)
    return dw


def conv3_dbias(dy):
    return dy.to(F64).sum(dim=(0, 1, 2, 3))


def _offsets():
    return [(od, oh, ow) for od in range(2) for oh in range(2) for ow in range(2)]


def convT_fwd(x, w, bias=None):
    B, D, H, W, _ = x.shape
    w = w.to(F64)
    out = torch.zeros(B, 2 * D, 2 * H, 2 * W, w.shape[1], dtype=F64)
    for od, oh, ow in _offsets():
        out[:, od::2, oh::2, ow::2] = x.to(F64) @ w[:, :, od, oh, ow]
    return out if bias is None else out + bias.to(F64)


def convT_dgrad(dout, w):
    B, D2, H2, W2, _ = dout.shape
    w = w.to(F64)
    dx = torch.zeros(B, D2 // 2, H2 // 2, W2 // 2, w.shape[0], dtype=F64)
    for od, oh, ow in _offsets():
        dx += dout[:, od::2, oh::2, ow::2].to(F64) @ w[:, :, od, oh, ow].t()
    return dx


def convT_wgrad(x, dout):
    cin, cout = x.shape[-1], dout.shape[-1]
    dw = torch.zeros(cin, cout, 2, 2, 2, dtype=F64)
    xf = x.to(F64).reshape(-1, cin)
    for od, oh, ow in _offsets():
        dw[:, :, od, oh, ow] = xf.t() @ dout[:, od::2, oh::2, ow::2].to(F64).reshape(-1, cout)
    return dw


# ------------------------------------------------------------------------------------------------ the anisotropic operators
# dg_tta_amd/csrc/conv_aniso.hip: kernel (kd, 3, 3) with kd in {1, 3}, padding (kd // 2, 1, 1), stride (sd, sh, sw) in {1, 2}^3, and
# the transposed conv with kernel = stride.  Per axis, with k the kernel extent, p = k // 2 and s the stride:
#     y[vo] = bias + sum_{tap, ci} x[s vo + tap - p] w[tap]          out extent (n + 2 p - k) // s + 1
#     out[s v + o][co] = bias[co] + sum_ci x[v][ci] w[ci][co][o]     (transposed conv, o in [0, sd) x [0, sh) x [0, sw))
def out_extent_k(n, k, stride):
    return (n + 2 * (k // 2) - k) // stride + 1


def aniso_out_dims(in_dims, kd, stride):
    return tuple(out_extent_k(n, k, s) for n, k, s in zip(in_dims, (kd, 3, 3), stride))


def _pad_k(x, kd):
    B, D, H, W, C = x.shape
    pd = kd // 2
    xp = torch.zeros(B, D + 2 * pd, H + 2, W + 2, C, dtype=x.dtype)
    xp[:, pd:pd + D, 1:-1, 1:-1] = x
    return xp


def _unpad_k(xp, kd):
    pd = kd // 2
    return xp[:, pd:xp.shape[1] - pd, 1:-1, 1:-1].contiguous()


def _tap_view_a(xp, td, th, tw, out_dims, stride):
    """_tap_view with one step per axis."""
    (Do, Ho, Wo), (sd, sh, sw) = out_dims, stride
    return xp[:, td:td + sd * (Do - 1) + 1:sd, th:th + sh * (Ho - 1) + 1:sh, tw:tw + sw * (Wo - 1) + 1:sw]


def _row_view_a(xp, td, th, out_dims, stride):
    """_row_view with one step per axis: the three kw taps of row (td, th), [B, Do, Ho, Wo, 3 C] ordered (kw, c)."""
    B, _, _, _, C = xp.shape
    sb, sd, sh, sw, sc = xp.stride()
    return xp.as_strided((B, *out_dims, 3 * C), (sb, stride[0] * sd, stride[1] * sh, stride[2] * sw, sc),
                         xp.storage_offset() + td * sd + th * sh)


def _rows_k(kd):
    return [(td, th) for td in range(kd) for th in range(3)]


def conva_fwd(x, w, bias=None, stride=(1, 1, 1)):
    """x [B, D, H, W, Cin], w [Cout, Cin, kd, 3, 3] -> [B, Do, Ho, Wo, Cout]."""
    C, kd = x.shape[-1], w.shape[2]
    od = aniso_out_dims(x.shape[1:4], kd, stride)
    xp = _pad_k(x.to(F64), kd)
    w = w.to(F64)
    y = torch.zeros(x.shape[0], *od, w.shape[0], dtype=F64)
    for td, th in _rows_k(kd):
        y += _row_view_a(xp, td, th, od, stride) @ w[:, :, td, th, :].permute(2, 1, 0).reshape(3 * C, -1)    # [(kw, ci), co]
    return y if bias is None else y + bias.to(F64)


def conva_dgrad(dy, w, in_dims, stride=(1, 1, 1)):
    B, (D, H, W) = dy.shape[0], in_dims
    w = w.to(F64)
    C, kd = w.shape[1], w.shape[2]
    od = aniso_out_dims(in_dims, kd, stride)
    assert tuple(dy.shape[1:4]) == od
    dxp = torch.zeros(B, D + 2 * (kd // 2), H + 2, W + 2, C, dtype=F64)
    for td, th in _rows_k(kd):
        t = dy.to(F64) @ w[:, :, td, th, :].permute(0, 2, 1).reshape(-1, 3 * C)                              # [co, (kw, ci)]
        for tw in range(3):
            _tap_view_a(dxp, td, th, tw, od, stride).add_(t[..., tw * C:(tw + 1) * C])
    return _unpad_k(dxp, kd)


def conva_wgrad(x, dy, kd, stride=(1, 1, 1)):
    od = tuple(dy.shape[1:4])
    assert od == aniso_out_dims(x.shape[1:4], kd, stride)
    C = x.shape[-1]
    xp = _pad_k(x.to(F64), kd)
    g = dy.to(F64).reshape(-1, dy.shape[-1])
    dw = torch.zeros(dy.shape[-1], C, kd, 3, 3, dtype=F64)
    for td, th in _rows_k(kd):
        dw[:, :, td, th, :] = (g.t() @ _row_view_a(xp, td, th, od, stride).reshape(-1, 3 * C)).reshape(-1, 3, C).permute(0, 2, 1)
    return dw


def conva_dbias(dy):
    return conv3_dbias(dy)


def _offsets_s(stride):
    return [(od, oh, ow) for od in range(stride[0]) for oh in range(stride[1]) for ow in range(stride[2])]


def convTa_fwd(x, w, bias=None):
    """x [B, D, H, W, Cin], w [Cin, Cout, sd, sh, sw] (kernel = stride) -> [B, sd D, sh H, sw W, Cout]."""
    B, D, H, W, _ = x.shape
    w = w.to(F64)
    sd, sh, sw = w.shape[2:]
    out = torch.zeros(B, sd * D, sh * H, sw * W, w.shape[1], dtype=F64)
    for od, oh, ow in _offsets_s((sd, sh, sw)):
        out[:, od::sd, oh::sh, ow::sw] = x.to(F64) @ w[:, :, od, oh, ow]
    return out if bias is None else out + bias.to(F64)


def convTa_dgrad(dout, w):
    w = w.to(F64)
    sd, sh, sw = w.shape[2:]
    B, Do, Ho, Wo, _ = dout.shape
    dx = torch.zeros(B, Do // sd, Ho // sh, Wo // sw, w.shape[0], dtype=F64)
    for od, oh, ow in _offsets_s((sd, sh, sw)):
        dx += dout[:, od::sd, oh::sh, ow::sw].to(F64) @ w[:, :, od, oh, ow].t()
    return dx


def convTa_wgrad(x, dout, stride):
    cin, cout = x.shape[-1], dout.shape[-1]
    sd, sh, sw = stride
    dw = torch.zeros(cin, cout, sd, sh, sw, dtype=F64)
    xf = x.to(F64).reshape(-1, cin)
    for od, oh, ow in _offsets_s(stride):
        dw[:, :, od, oh, ow] = xf.t() @ dout[:, od::sd, oh::sh, ow::sw].to(F64).reshape(-1, cout)
    return dw


def abs_bound(op, *operands, **kw):
    """sum |a b| per output element of `op`: the same operator applied to the magnitudes of its tensor operands."""
    return op(*[t.abs() if torch.is_tensor(t) else t for t in operands], **kw)


def gstats_sums(dx, y_prev, mean, rstd, gamma, beta, slope):
    """What the fused data gradient leaves for the InstanceNorm backward of the previous block (instnorm_ref's S0 and the raw
    form of S1): a = gamma (y - mean) rstd + beta, da = dx if a > 0 else slope dx; returns (sum_v da, sum_v da y), each [B, C].
    dx, y_prev: [B, ..., C]; mean, rstd: [B, C]; gamma, beta: [C]."""
    B, C = dx.shape[0], dx.shape[-1]
    g, y = dx.to(F64).reshape(B, -1, C), y_prev.to(F64).reshape(B, -1, C)
    a = (y - mean.to(F64)[:, None, :]) * rstd.to(F64)[:, None, :] * gamma.to(F64) + beta.to(F64)
    da = torch.where(a > 0, g, slope * g)
    return da.sum(dim=1), (da * y).sum(dim=1)


# ------------------------------------------------------------------------------------------------ integer operands
def ternary(shape, p, gen):
    """float64 tensor of -1 / 0 / +1: nonzero with probability p, the sign uniform."""
    nz = torch.rand(shape, generator=gen, dtype=F64) < p
    sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int64) * 2 - 1
    return (nz * sign).to(F64)


def integers(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64).to(F64)


def densities(cin, cout):
    """The draw rule: x and dy nonzero with probability 2/3; w with min(2/3, 32 / K), K = Cin for the forward (and the
    transposed conv's forward), Cout for the data gradients."""
    return dict(x=2.0 / 3, dy=2.0 / 3, w_fwd=min(2.0 / 3, 32.0 / cin), w_dgrad=min(2.0 / 3, 32.0 / cout))


BIAS_RANGE = 3          # bias in [-3, 3]
BASE_RANGE = 8          # accumulate base in [-8, 8]
LIMIT_16BIT = 256       # integers of magnitude <= 256 are exact in bf16 (and fp16)
LIMIT_F32 = 2 ** 24

# (B, Cin, Cout, D, H, W) of the INPUT volume; see the table in tests/test_gpu_conv_exact.py for which kernel each one reaches
GENERIC_CASES = [(1, 32, 32, 9, 7, 45), (2, 16, 64, 6, 10, 16), (1, 32, 48, 8, 8, 8), (1, 320, 320, 4, 4, 4), (1, 16, 32, 20, 20, 12)]
ROWS_CASES = [(1, 32, 32, 9, 13, 45), (1, 16, 32, 4, 8, 33), (1, 64, 96, 8, 8, 70)]
# the last: more column jobs than CUs - 64 input channels make columns of 32 x 4 voxels, 4 * 2 * 3 * 11 = 264 of them for the 256
# CUs, in the forward and in the data gradient (a 32-channel case of that many columns needs three times the voxels)
RING_CASES = [(1, 32, 32, 9, 13, 45), (2, 64, 96, 6, 7, 64), (2, 32, 64, 6, 17, 32), (4, 64, 64, 3, 41, 65)]
S2_CASES = [(1, 32, 64, 6, 10, 72), (1, 32, 128, 9, 7, 66), (2, 64, 128, 4, 6, 64), (1, 16, 32, 10, 12, 14)]
S2_ODD_DGRAD_CASE = (1, 16, 32, 9, 7, 13)
# weight gradient, stride 1: ragged Cin 12 / 24 (ld rounded up to 8), W <= 16 planes, 1x1x1, batch > 1, 320 channels at 4^3
WGRAD_CASES = [(1, 32, 32, 9, 13, 45), (2, 12, 32, 6, 17, 32), (1, 24, 32, 6, 9, 33), (1, 64, 96, 7, 8, 70), (1, 8, 32, 7, 8, 32),
               (1, 24, 40, 5, 7, 6), (2, 40, 64, 3, 11, 16), (1, 32, 32, 1, 1, 1), (5, 32, 32, 2, 3, 2), (1, 320, 320, 4, 4, 4)]
WGRAD_S2_CASES = [(1, 32, 64, 8, 8, 32), (2, 16, 32, 6, 6, 20), (1, 40, 64, 6, 4, 34), (1, 320, 320, 4, 4, 8)]
CONVT_CASES = [(1, 64, 32, 4, 6, 40), (2, 128, 64, 3, 4, 32), (2, 24, 16, 4, 4, 8), (1, 320, 256, 4, 4, 4)]
# dgtta_conv3d_k3_dgrad_gstats, Cin / Cout in the conv's own sense (dx and y_prev have Cin channels, dy has Cout)
GSTATS_RING_CASES = [(1, 32, 32, 9, 13, 45), (2, 64, 32, 6, 7, 64), (1, 64, 64, 5, 9, 40)]      # the last: dy with 64 channels (the ring's two K halves)
GSTATS_ROWS_CASES = [(1, 32, 16, 4, 8, 64), (2, 32, 16, 8, 16, 32)]      # whole tiles (4 x 8 x 32), as the row-reuse kernel asks
GSTATS_SLOPE = 0.25


def fwd_dgrad_cases():
    """Every (case, stride) whose forward / data gradient the GPU test runs."""
    seen, out = set(), []
    for c in GENERIC_CASES + ROWS_CASES + RING_CASES:
        if (c, 1) not in seen:
            seen.add((c, 1)), out.append((c, 1))
    return out + [(c, 2) for c in S2_CASES + [S2_ODD_DGRAD_CASE]]


def _gen(case, salt):
    return torch.Generator().manual_seed(1000003 * salt + sum((i + 1) * int(c) for i, c in enumerate(case)))


@functools.lru_cache(maxsize=None)
def conv_problem(case, stride):
    """Operands and float64 results of one forward / data-gradient case (computed once per process; treat as read-only)."""
    B, cin, cout, D, H, W = case
    g = _gen(case, 10 + stride)
    p = densities(cin, cout)
    od = tuple(out_extent(n, stride) for n in (D, H, W))
    x = ternary((B, D, H, W, cin), p["x"], g)
    w = ternary((cout, cin, 3, 3, 3), p["w_fwd"], g)
    bias = integers((cout,), -BIAS_RANGE, BIAS_RANGE, g)
    dy = ternary((B, *od, cout), p["dy"], g)
    wd = ternary((cout, cin, 3, 3, 3), p["w_dgrad"], g)
    base = integers((B, D, H, W, cin), -BASE_RANGE, BASE_RANGE, g)
    y = conv3_fwd(x, w, bias, stride)
    dx = conv3_dgrad(dy, wd, (D, H, W), stride)
    return dict(x=x, w=w, bias=bias, dy=dy, wd=wd, base=base, y=y, dx=dx, od=od)


@functools.lru_cache(maxsize=None)
def wgrad_problem(case, stride):
    B, cin, cout, D, H, W = case
    g = _gen(case, 20 + stride)
    p = densities(cin, cout)
    od = tuple(out_extent(n, stride) for n in (D, H, W))
    x = ternary((B, D, H, W, cin), p["x"], g)
    dy = ternary((B, *od, cout), p["dy"], g)
    base_w = integers((cout, cin, 3, 3, 3), -BASE_RANGE, BASE_RANGE, g)
    base_b = integers((cout,), -BASE_RANGE, BASE_RANGE, g)
    return dict(x=x, dy=dy, base_w=base_w, base_b=base_b, dw=conv3_wgrad(x, dy, stride), db=conv3_dbias(dy))


@functools.lru_cache(maxsize=None)
def convT_problem(case):
    """x [B,D,H,W,Cin]; the output is the first Cout channels of a concat buffer of 2 Cout, and dcat is that buffer's gradient."""
    B, cin, cout, D, H, W = case
    g = _gen(case, 30)
    x = ternary((B, D, H, W, cin), 2.0 / 3, g)
    w = ternary((cin, cout, 2, 2, 2), min(2.0 / 3, 32.0 / cin), g)
    bias = integers((cout,), -BIAS_RANGE, BIAS_RANGE, g)
    dcat = ternary((B, 2 * D, 2 * H, 2 * W, 2 * cout), 2.0 / 3, g)
    wd = ternary((cin, cout, 2, 2, 2), min(2.0 / 3, 32.0 / cout), g)
    base_w = integers((cin, cout, 2, 2, 2), -BASE_RANGE, BASE_RANGE, g)
    base_b = integers((cout,), -BASE_RANGE, BASE_RANGE, g)
    dout = dcat[..., :cout]
    return dict(x=x, w=w, bias=bias, dcat=dcat, wd=wd, base_w=base_w, base_b=base_b, out=convT_fwd(x, w, bias),
                dx=convT_dgrad(dout, wd), dw=convT_wgrad(x, dout), db=conv3_dbias(dout))


@functools.lru_cache(maxsize=None)
def gstats_problem(case):
    """Integer dy and w, integer y_prev in [-3, 3], mean = 1/2, rstd = 1, gamma in {+-1, +-2}, beta = 0, slope 1/4: the
    pre-activation gamma (y - 1/2) is exact and never 0, da is an exact multiple of 1/4."""
    B, cin, cout, D, H, W = case
    g = _gen(case, 40)
    dy = ternary((B, D, H, W, cout), 2.0 / 3, g)
    w = ternary((cout, cin, 3, 3, 3), min(2.0 / 3, 32.0 / cout), g)
    y_prev = integers((B, D, H, W, cin), -3, 3, g)
    gamma = (integers((cin,), 1, 2, g) * (integers((cin,), 0, 1, g) * 2 - 1))
    beta = torch.zeros(cin, dtype=F64)
    mean, rstd = torch.full((B, cin), 0.5, dtype=F64), torch.ones(B, cin, dtype=F64)
    dx = conv3_dgrad(dy, w, (D, H, W), 1)
    s0, s1 = gstats_sums(dx, y_prev, mean, rstd, gamma, beta, GSTATS_SLOPE)
    return dict(dy=dy, w=w, y_prev=y_prev, gamma=gamma, beta=beta, mean=mean, rstd=rstd, dx=dx, s0=s0, s1=s1)


# ------------------------------------------------------------------------------------------------ anisotropic cases
# what tests/test_gpu_aniso_exact.py runs and tests/test_conv_ref.py checks the conditions of; every conv case with both kd and
# all eight strides, every transposed case with the seven strides that are not (1, 1, 1)
ANISO_KDS = (1, 3)
ANISO_STRIDES = [(sd, sh, sw) for sd in (1, 2) for sh in (1, 2) for sw in (1, 2)]
ANISO_CONVT_STRIDES = [s for s in ANISO_STRIDES if s != (1, 1, 1)]
# Wo 72 / 36: the 32-wide tile (sd = 1) and the 16-wide one (sd = 2), ragged in W, H, D, Cin (16-channel K chunk) and Cout (32), 18 tiles at
# stride 1 | Wo 28 / 14: the 16- and the 8-wide tile, Cin 12 (the first layer's ragged row), batch 2, 40 tiles at stride 1 (the XCD
# swizzle) | the 8-wide tile at sw = 1, Cout < 32, one tile along D | odd extents: forward only where a strided axis is odd | Wo 40 /
# 20: the one tile the four above leave out, 16-wide with sd = 1 and sw = 2 (and the 16-wide tile under several data-gradient classes)
ANISO_CONV_CASES = [(1, 24, 40, 6, 10, 72), (2, 12, 32, 6, 20, 28), (1, 16, 8, 4, 6, 12), (1, 16, 32, 5, 7, 13), (1, 8, 16, 4, 6, 40)]
# batch 2 with Cin 24 and odd extents | Cin 40 > 32, ragged against it | rows of 36 voxels (the 32-wide tile) with Cin = 2 x 32
ANISO_CONVT_CASES = [(2, 24, 16, 3, 5, 7), (1, 40, 24, 4, 6, 18), (1, 64, 32, 2, 4, 36)]


def aniso_grads_defined(case, stride):
    """The library's data and weight gradient ask for an even input extent along every strided axis."""
    return all(s == 1 or n % 2 == 0 for n, s in zip(case[3:], stride))


def _stride_code(stride):
    return (stride[0] - 1) * 4 + (stride[1] - 1) * 2 + (stride[2] - 1)


@functools.lru_cache(maxsize=None)
def aniso_conv_problem(case, kd, stride):
    """conv_problem for kernel (kd, 3, 3) and stride (sd, sh, sw); dx is None where the library refuses the data gradient."""
    B, cin, cout, D, H, W = case
    g = _gen(case, 100 + 10 * kd + _stride_code(stride))
    p = densities(cin, cout)
    od = aniso_out_dims((D, H, W), kd, stride)
    x = ternary((B, D, H, W, cin), p["x"], g)
    w = ternary((cout, cin, kd, 3, 3), p["w_fwd"], g)
    bias = integers((cout,), -BIAS_RANGE, BIAS_RANGE, g)
    dy = ternary((B, *od, cout), p["dy"], g)
    wd = ternary((cout, cin, kd, 3, 3), p["w_dgrad"], g)
    base = integers((B, D, H, W, cin), -BASE_RANGE, BASE_RANGE, g)
    dx = conva_dgrad(dy, wd, (D, H, W), stride) if aniso_grads_defined(case, stride) else None
    return dict(x=x, w=w, bias=bias, dy=dy, wd=wd, base=base, y=conva_fwd(x, w, bias, stride), dx=dx, od=od)


@functools.lru_cache(maxsize=None)
def aniso_wgrad_problem(case, kd, stride):
    B, cin, cout, D, H, W = case
    assert aniso_grads_defined(case, stride)
    g = _gen(case, 300 + 10 * kd + _stride_code(stride))
    p = densities(cin, cout)
    od = aniso_out_dims((D, H, W), kd, stride)
    x = ternary((B, D, H, W, cin), p["x"], g)
    dy = ternary((B, *od, cout), p["dy"], g)
    base_w = integers((cout, cin, kd, 3, 3), -BASE_RANGE, BASE_RANGE, g)
    base_b = integers((cout,), -BASE_RANGE, BASE_RANGE, g)
    return dict(x=x, dy=dy, base_w=base_w, base_b=base_b, dw=conva_wgrad(x, dy, kd, stride), db=conva_dbias(dy), od=od)


@functools.lru_cache(maxsize=None)
def aniso_convT_problem(case, stride):
    """convT_problem for kernel = stride: the output is the first Cout channels of a concat buffer of 2 Cout, dcat its gradient."""
    B, cin, cout, D, H, W = case
    sd, sh, sw = stride
    g = _gen(case, 500 + _stride_code(stride))
    x = ternary((B, D, H, W, cin), 2.0 / 3, g)
    w = ternary((cin, cout, sd, sh, sw), min(2.0 / 3, 32.0 / cin), g)
    bias = integers((cout,), -BIAS_RANGE, BIAS_RANGE, g)
    dcat = ternary((B, sd * D, sh * H, sw * W, 2 * cout), 2.0 / 3, g)
    wd = ternary((cin, cout, sd, sh, sw), min(2.0 / 3, 32.0 / cout), g)
    base_w = integers((cin, cout, sd, sh, sw), -BASE_RANGE, BASE_RANGE, g)
    base_b = integers((cout,), -BASE_RANGE, BASE_RANGE, g)
    dout = dcat[..., :cout]
    return dict(x=x, w=w, bias=bias, dcat=dcat, wd=wd, base_w=base_w, base_b=base_b, out=convTa_fwd(x, w, bias),
                dx=convTa_dgrad(dout, wd), dw=convTa_wgrad(x, dout, stride), db=conv3_dbias(dout))
