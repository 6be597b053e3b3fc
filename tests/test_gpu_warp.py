"""GPU: the affine warp kernels of warp.hip and the segmentation head fused with the inverse warp, called through the C
ABI, against the float64 restatement tests/warp_ref.py (licensed by tests/test_warp_ref.py): every dispatch branch of
dgtta_affine_warp3d_fwd / _bwd, both forward kernels of dgtta_seghead_warp_fwd, dgtta_seghead_warp_bwd / _bwd_g16, over one
named table of maps (MAPS) that reaches the branches of the owner-computes candidate search random maps never reach: exact
lattice positions (floor ties), 90-degree rotations and an axis permutation (m[j][0] == 0: the `bounds_w` false branch),
the same with 1e-5 in place of a zero, samples and candidates beyond every face (the lo / hi clamps), the acceptance edge
of the search (diag 0.38 / 0.37 / 0.29 / 0.28), a singular map.

Every bound follows from the arithmetic (u = 2^-24; u_T = the storage type's unit roundoff; SUB_T = half the spacing of fp16
subnormals, an absolute term).  No flat tolerance anywhere.

  position     delta, per axis and sample of the batch, in voxels: the kernel's fp32 sample position against the float64 one.
               Base coordinate: five roundings of values <= 1 (step, step j, -1 + ., . (n - 1), / n): 5u.  g = fma chain + th3:
               four roundings of partial sums <= A = |th0| + |th1| + |th2| + |th3|, inputs off by 5u: 9u A.  The reference code's
               (g - x) + x (`tta_grid_algebra`): two more roundings of <= A + 1.  i = ((g + 1) n - 1) / 2: three roundings.
                 delta = u (n / 2) (9 A + 3 (A + 1) + 2 (A + 1) [algebra]) + u / 2
  forward      linear modes are continuous in the position, across cell faces and the zero-padding boundary, so NO element is
               excluded: moving the position by delta moves the sample by at most sum_axis delta_axis L_axis, L = the largest
               |difference of axis neighbours| of the sampled volume (continued by zeros / by `sub`, or by its faces with border
               padding) over the 3 x 3 x 3 cells around the float64 cell - fp32 may floor into the adjacent cell.  Blend: a corner
               weight is a product of three differences (5 roundings), x - sub (1), the product (1), eight additions (8):
                 |out - ref| <= sum_axis delta L + 16u warp(|x - sub|) + u |ref|
               nearest copies values: samples whose float64 position is within 1e-4 (> delta, asserted) of a half-integer on
               some axis are left out (under 1 % per case, asserted), all others match BIT FOR BIT ((x - sub) + sub in fp32).
  adjoint      a weight moves by at most delta_x + delta_y + delta_z; S1 = sum |g| over the candidates (samples with the voxel
               among their corners, or within delta of it), n their number, A = sum |w g| (warp_abs_adjoint):
                 |gsrc - ref| <= (delta_x + delta_y + delta_z) S1 + (n + 6) u A          (5 + 1 roundings per term, n - 1 additions)
               gather against scatter (NDHWC zeros against the same gradient through the NCDHW entry, whose scatter takes
               corners() straight from the forward, no search): the same fp32 terms, two orders of summation:
                 |gather - scatter| <= 2 (n - 1) u (A + (delta_x + delta_y + delta_z) S1)
               ADDITION to the (n - 1) u A first stated for this comparison, which counts the n - 1 roundings of ONE sum: each
               of the two sums makes its own and is within (n - 1) u A of the exact sum of the terms, so 2 (n - 1) is what the
               arithmetic gives for their difference.  The kernels reach 1.22 of (n - 1) u A (gather-vec-C36-4x5x17, tta008).
               A candidate dropped by the search shows here from a weight of about 1e-6.
               sparse gradient (fused backward): with the logit gradient non-zero on every third destination voxel per axis and
               a map that takes the lattice to itself, every feature-map voxel receives at most ONE term (asserted), so no sum
               is formed and gz must equal the atomic scatter followed by dgtta_seghead_bwd BIT FOR BIT: a candidate that the
               fused kernel's own copy of the search drops is a wrong gz however small its weight.
  fused fwd    out = W (blend of z) + b (sum of the in-volume weights): the blend (14), the 32-term chain (32), two additions:
                 |out - ref| <= sum_axis delta L[logits] + 48u (|W| warp(|z|) + |b| warp(1)) + 2u |ref|
               against head_then_warp in float64 on the storage-rounded z.
  fused bwd    acc = the gathered logit gradient (adjoint bound E_acc above, C = nsel), then
                 gz   E32 = |W|^T E_acc + 16u |W|^T |acc|;  u_T (|ref| + E32) + SUB_T + E32
                 dw   formed on the matrix cores from d16 = the 16-bit copy of acc, so every gathered value carries u_T before
                      the sum: e16 = E_acc + u_T (|acc| + E_acc) + SUB_T;  sum_v |z| e16 + N u sum_v |acc z| + u |result|,
                      N = B D H W terms in fp32 (the 16-bit products are exact in fp32)
                 db   fp32 wave sums (63 additions at most: 2^-18), then double, one rounding to float:
                      sum_v E_acc + 2^-18 sum_v |acc| + u |result|
               accumulate = 1 on pre-loaded dw / db: one more rounding of the sum, u |result|.

Buffers: every output is pre-filled with NaN, padding columns of outputs (ldc > C) with a sentinel that must survive, padding
columns of inputs and every workspace with NaN.  Each comparison prints its largest error / bound ratio.

Branch reached per case id: the `branch` field of FWD_CASES / BWD_CASES / HEAD_FWD_CASES and the docstrings of the tests.

Measured on an MI355X (largest error / bound per group):
  a  forward, linear: 0.145 (rows4), 0.138 (kernel<1,true>), 0.101 (kernel<1,false>) - the position term is a worst case over
     the neighbourhood; nearest (kernel<4,true>, <1,true>, <1,false>): every compared sample bit for bit, 0 .. 0.5 % left out
  b  backward against float64: 0.089 (gather<16,true>), 0.057 (gather<16,false>), 0.055 (scatter); gather against scatter:
     0.609 of 2 (n - 1) u sum |terms| - one or two ulps of the result at elements of 4 .. 12 candidates
  c  fused forward: 0.162 on the matrix cores, 0.162 with DGTTA_HEADWARP_MFMA=0
  d  fused backward: 0.961 (gz: the 16-bit storage rounding itself goes up to half an ulp = u_T |ref|); gz and dw equal the
     two-step path bit for bit, and gz of the sparse gradient the scatter path, on every case listed there
  e  supported() agrees with the backward on every map and shape; diag(0.38) accepted and correct, 0.37 / 0.29 / 0.28 / singular
     refused with nothing written

Two defects of warp.hip that these cases reach are fixed with them:
  1. With 4 or 12 selected classes dgtta_seghead_warp_supported said 1, but dgtta_seghead_warp_bwd returned
     DGTTA_ERR_UNSUPPORTED from its weight-gradient step after gz had been written (case d 1x8x8x18 shift_half, nsel 12).
     Both now refuse up front when dw_sel is wanted; gz and db_sel alone are still computed.
  2. dgtta_affine_warp3d_bwd with src_ldc > C cleared whole rows of src_ldc elements on the scatter paths (border padding,
     declined maps) - the neighbouring columns of a wider buffer.  Only the operand columns are zeroed now."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import warp_ref as wref
from conftest import reload_kernel_switches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
U = 2.0 ** -24
U_T = {0: 0.0, 1: 2.0 ** -8, 2: 2.0 ** -11}
SUB_T = {0: 0.0, 1: 0.0, 2: 2.0 ** -25}
SENTINEL = -77.0
OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
PAD = {"zeros": 0, "border": 1}
INTERP = {"linear": 0, "nearest": 1}
CIN = 32


# ------------------------------------------------------------------------------------------------ the map list
def _vox(M, t=(0.0, 0.0, 0.0)):
    """theta of the VOXEL-space map p = M (v - c_dst) + c_src + t (rows / columns x, y, z; c = the volume's centre), so that
    a rotation is a rotation of the lattice on a non-cubic volume too: th[j][i] = M[j][i] n_i / S_j, th[j][3] = 2 t_j / S_j."""
    def make(dst, src):
        n, S = (dst[2], dst[1], dst[0]), (src[2], src[1], src[0])
        th = torch.zeros(3, 4, dtype=torch.float64)
        for j in range(3):
            for i in range(3):
                th[j, i] = M[j][i] * n[i] / S[j]
            th[j, 3] = 2.0 * t[j] / S[j]
        return th.float()
    return make


def _norm(rows):
    return lambda dst, src: torch.tensor(rows, dtype=torch.float64).float()


def _diag(s):
    return _vox([[s, 0, 0], [0, s, 0], [0, 0, s]])


def _tta008(dst, src):
    from oracle import tta as otta
    draw = torch.randn(1, 3, 4, generator=torch.Generator().manual_seed(8))
    return otta.rand_affine_from_draw(draw, 0.08)[1][0].float()


def _strong(dst, src):
    g = torch.Generator().manual_seed(33)                       # (this draw: 134 candidates per voxel, the fused backward takes it)
    M = torch.eye(3, dtype=torch.float64) + 0.3 * torch.randn(3, 3, generator=g, dtype=torch.float64)
    t = 1.5 * torch.randn(3, generator=g, dtype=torch.float64)
    return _vox(M.tolist(), t.tolist())(dst, src)


_I = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
_ROT_Z = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
MAPS = {
    "identity": _vox(_I),                                       # sample positions are lattice points: floor ties
    "shift_int": _vox(_I, (2.0, -1.0, 1.0)),
    "shift_half": _vox(_I, (0.5, 0.5, 0.5)),
    "outside": _norm([[1, 0, 0, 4.0], [0, 1, 0, 0], [0, 0, 1, 0]]),      # every sample beyond the x face: all zeros
    "tta008": _tta008,                                          # the near-identity draw of the TTA loop
    "strong": _strong,
    "rot_x": _vox([[1, 0, 0], [0, 0, -1], [0, 1, 0]]),          # m[1][0] = m[2][0] = 0
    "rot_y": _vox([[0, 0, 1], [0, 1, 0], [-1, 0, 0]]),          # m[0][0] = m[1][0] = 0
    "rot_z": _vox(_ROT_Z),                                      # m[0][0] = m[2][0] = 0
    "perm": _vox([[0, 1, 0], [0, 0, 1], [1, 0, 0]]),            # m[0][0] = m[1][0] = 0
    "rot_z_eps": _vox([[1e-5, -1, 0], [1, 0, 0], [0, 0, 1]]),   # just above the 1e-6 test of bounds_w
    "reflect": _vox([[-1, 0, 0], [0, 1, 0], [0, 0, -1]]),
    "shear": _vox([[1, 0.31, 0.17], [0, 1, 0.23], [0, 0, 1]]),
    "magnify": _vox([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 1]]),     # anisotropic magnification x 2
    "diag038": _diag(0.38),                                     # prod(2 e + 1) = 245.7: host and device accept
    "diag037": _diag(0.37),                                     # 262.8: the device alone
    "diag029": _diag(0.29),                                     # 492: the device alone
    "diag028": _diag(0.28),                                     # 540: neither
    "singular": _norm([[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0]]),
    "fit": _norm([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]),   # the normalised identity: a pure resize when dst != src
}
ALL = [m for m in MAPS if m != "fit"]
HOST_REFUSED = ("diag037", "diag029", "diag028", "singular")
# nearest: no map whose positions are half-integers throughout (shift_half; magnify and the rotations on mixed parities)
NEAREST = ["identity", "shift_int", "reflect", "tta008", "strong", "shear", "outside"]
RESIZE = ["fit", "tta008", "strong", "rot_z", "shift_half", "diag038"]


def _thetas(names, dst, src=None):
    return torch.stack([MAPS[n](dst, src or dst) for n in names]).contiguous()


def _batches(names, B):
    """The map list dealt to calls of B samples (the last call wraps around); a list of tuples is taken as the calls."""
    if isinstance(names[0], tuple):
        return list(names)
    return [tuple(names[(i + j) % len(names)] for j in range(B)) for i in range(0, len(names), B)]


def _vol64(theta, size):
    """prod(2 e_i + 1), e = the absolute row sums of the inverse voxel-space map: the candidates per source voxel."""
    n = torch.tensor([size[2], size[1], size[0]], dtype=torch.float64)
    m = theta[:, :3].double() * n[:, None] / n[None, :]
    if abs(float(torch.linalg.det(m))) < 1e-12:
        return math.inf
    e = torch.linalg.inv(m).abs().sum(dim=1)
    return float((2 * e + 1).prod())


# ------------------------------------------------------------------------------------------------ bounds (float64, CPU)
def _delta(theta, src_size, algebra):
    """[B, 3] (x, y, z): the position bound of the module docstring."""
    th = theta.double()
    A = th.abs().sum(dim=2)
    n = torch.tensor([src_size[2], src_size[1], src_size[0]], dtype=torch.float64)
    return U * (n / 2 * (9 * A + 3 * (A + 1) + (2 * (A + 1) if algebra else 0.0)) + 0.5)


def _position_term(vol, theta, dst_size, pad, delta):
    """sum_axis delta_axis L_axis per output element.  vol [B, Ds, Hs, Ws, C] is the sampled volume (minus `sub`)."""
    B, Ds, Hs, Ws, C = vol.shape
    src_size = (Ds, Hs, Ws)
    pos = wref._padded(wref.sample_positions(theta, dst_size, src_size), src_size, pad)
    P = vol.permute(0, 4, 1, 2, 3)
    if pad == "border":
        P = torch.cat([P[:, :, :1].expand(-1, -1, 3, -1, -1), P, P[:, :, -1:].expand(-1, -1, 3, -1, -1)], dim=2)
        P = torch.cat([P[:, :, :, :1].expand(-1, -1, -1, 3, -1), P, P[:, :, :, -1:].expand(-1, -1, -1, 3, -1)], dim=3)
        P = torch.cat([P[..., :1].expand(-1, -1, -1, -1, 3), P, P[..., -1:].expand(-1, -1, -1, -1, 3)], dim=4)
    else:
        P = F.pad(P, (3, 3, 3, 3, 3, 3))
    # cell of every sample in padded coordinates; cells further out than the padding sample nothing but the continuation
    cz, cy, cx = (p.floor().long().clamp(-3, n + 2) + 3 for p, n in zip((pos[2], pos[1], pos[0]), src_size))
    b = torch.arange(B).view(-1, 1, 1, 1)
    out = torch.zeros(B, *dst_size, C, dtype=torch.float64)
    for axis, dim in ((0, 4), (1, 3), (2, 2)):              # x, y, z
        d = P.diff(dim=dim).abs()                           # entry i: |P[i + 1] - P[i]|
        padw = [0, 0, 0, 0, 0, 0]
        padw[2 * (4 - dim) + 1] = 1
        d = F.pad(d, padw)
        # cells c - 1 .. c + 1: along the axis the pairs (c - 1, c) .. (c + 1, c + 2), across it the lines c - 1 .. c + 2
        padl = [1, 2, 1, 2, 1, 2]
        padl[2 * (4 - dim) + 1] = 1
        kernel = [4, 4, 4]
        kernel[dim - 2] = 3
        L = F.max_pool3d(F.pad(d, padl), kernel_size=kernel, stride=1)
        out += delta[:, axis].view(-1, 1, 1, 1, 1) * L.permute(0, 2, 3, 4, 1)[b, cz, cy, cx]
    return out


def _fwd_bound(x64, sub, theta, dst_size, pad, algebra, ref):
    xs = x64 - sub
    d = _delta(theta, tuple(x64.shape[1:4]), algebra)
    return _position_term(xs, theta, dst_size, pad, d) + 16 * U * wref.warp(xs.abs(), theta, dst_size, pad) + U * ref.abs()


def _adjoint(g64, theta, src_size, pad, algebra):
    """Reference and bounds of the adjoint of one call, computed once and shared by its comparisons."""
    d = _delta(theta, src_size, algebra)
    tol = tuple(d[:, a].view(-1, 1, 1, 1) for a in range(3))
    cnt, S1 = wref.candidate_sums(g64, theta, src_size, pad, tol)
    A = wref.warp_abs_adjoint(g64, theta, src_size, pad)
    moved = d.sum(dim=1).view(-1, 1, 1, 1, 1) * S1
    n = cnt[..., None]
    return SimpleNamespace(ref=wref.warp_adjoint(g64, theta, src_size, pad), bound=moved + (n + 6) * U * A,
                           order=2 * (n - 1).clamp(min=0) * U * (A + moved), n=cnt)


def _ratio(err, bound):
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(torch.nan_to_num(r, nan=math.inf).max())


def _within(what, got, ref, bound):
    """Asserts |got - ref| <= bound element by element (NaN fails) and prints the largest error / bound."""
    err = (got - ref).abs()
    ratio = _ratio(err, bound)
    print(f"RATIO {what}: max err/bound {ratio:.3f} (max abs err {float(torch.nan_to_num(err, nan=math.inf).max()):.3e})")
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f}"
    return ratio


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _volume(B, size, C, seed):
    """[B, D, H, W, C] float32 draws on the CPU; shared, nothing modifies it."""
    g = torch.Generator().manual_seed(7919 * seed + 131 * B + 17 * C + size[0] * 10007 + size[1] * 101 + size[2])
    return torch.randn(B, *size, C, generator=g) + 0.25


SEL16 = [97, 3, 104, 0, 55, 12, 71, 33, 8, 90, 41, 2, 66, 19, 100, 27]      # non-monotone rows of a 105-class head


@functools.lru_cache(maxsize=None)
def _head_params():
    g = torch.Generator().manual_seed(105)
    return torch.randn(105, CIN, generator=g) * 0.3, torch.randn(105, generator=g)


def _sel(nsel, with_sel):
    return torch.tensor(SEL16[:nsel], dtype=torch.int32) if with_sel else None


# ------------------------------------------------------------------------------------------------ device buffers
def _lib():
    from dg_tta_amd import _lib as L
    return L.load()


class Rows:
    """n rows of leading dimension ld; the operand is columns 0 .. C-1 and starts `lead` elements into the allocation.
    Everything that is not operand holds `pad`; the operand holds `values` or NaN."""

    def __init__(self, n, C, ld, pad, values=None, lead=0, dtype=torch.float32):
        self.n, self.C, self.ld, self.pad, self.lead = n, C, ld, pad, lead
        self.flat = torch.full((lead + n * ld + 16,), pad, dtype=dtype, device=DEV)
        self.rows = self.flat[lead:lead + n * ld].view(n, ld)
        fill = torch.full((n, C), math.nan, dtype=dtype) if values is None else values.reshape(n, C).to(dtype)
        self.rows[:, :C] = fill.to(DEV)
        self.ptr = self.rows.data_ptr()

    def get(self):
        return self.rows[:, :self.C].contiguous().cpu()

    def assert_padding_untouched(self, what):
        t = self.flat.clone()
        t[self.lead:self.lead + self.n * self.ld].view(self.n, self.ld)[:, :self.C] = self.pad
        same = (t == self.pad) | (torch.isnan(t) & math.isnan(self.pad))
        assert bool(same.all()), f"{what}: an element outside the operand was written"


def _opts(**kw):
    o = dict(ndhwc=1, lds=(0, 0), leads=(0, 0), pad="zeros", interp="linear", algebra=1, sub=None)
    o.update(kw)
    return SimpleNamespace(**o)


def k_warp_fwd(x, theta, dst_size, o):
    """dgtta_affine_warp3d_fwd on x [B, Ds, Hs, Ws, C] float32 (CPU) -> [B, Dd, Hd, Wd, C] float32 (CPU)."""
    from dg_tta_amd._lib import check, ptr, stream_of
    B, Ds, Hs, Ws, C = x.shape
    Dd, Hd, Wd = dst_size
    th = theta.to(DEV)
    sub = None if o.sub is None else torch.tensor([o.sub], dtype=torch.float32, device=DEV)
    if o.ndhwc:
        src = Rows(B * Ds * Hs * Ws, C, C + o.lds[0], math.nan, x, lead=o.leads[0])
        dst = Rows(B * Dd * Hd * Wd, C, C + o.lds[1], SENTINEL, lead=o.leads[1])
        sp, dp, sld, dld = src.ptr, dst.ptr, src.ld, dst.ld
    else:
        src_t = x.permute(0, 4, 1, 2, 3).contiguous().to(DEV)
        dst_t = torch.full((B, C, Dd, Hd, Wd), math.nan, device=DEV)
        sp, dp, sld, dld = ptr(src_t), ptr(dst_t), C, C
    check(_lib().dgtta_affine_warp3d_fwd(sp, ptr(th), dp, B, C, Ds, Hs, Ws, Dd, Hd, Wd, o.ndhwc, sld, dld, PAD[o.pad], INTERP[o.interp],
                                         o.algebra, ptr(sub), stream_of()), "affine_warp3d_fwd")
    torch.cuda.synchronize()
    if o.ndhwc:
        dst.assert_padding_untouched("warp_fwd dst")
        assert torch.equal(src.get().view(-1), x.reshape(-1)), "the forward modified src"
        return dst.get().view(B, Dd, Hd, Wd, C)
    return dst_t.permute(0, 2, 3, 4, 1).contiguous().cpu()


def k_warp_bwd(g, theta, src_size, o, expect=OK):
    """dgtta_affine_warp3d_bwd on g [B, Dd, Hd, Wd, C] float32 (CPU) -> grad_src [B, Ds, Hs, Ws, C] float32 (CPU)."""
    from dg_tta_amd._lib import ptr, stream_of
    B, Dd, Hd, Wd, C = g.shape
    Ds, Hs, Ws = src_size
    th = theta.to(DEV)
    if o.ndhwc:
        gd = Rows(B * Dd * Hd * Wd, C, C + o.lds[1], math.nan, g, lead=o.leads[1])
        gs = Rows(B * Ds * Hs * Ws, C, C + o.lds[0], SENTINEL, lead=o.leads[0])
        gp, sp, sld, dld = gd.ptr, gs.ptr, gs.ld, gd.ld
    else:
        gd_t = g.permute(0, 4, 1, 2, 3).contiguous().to(DEV)
        gs_t = torch.full((B, C, Ds, Hs, Ws), math.nan, device=DEV)
        gp, sp, sld, dld = ptr(gd_t), ptr(gs_t), C, C
    rc = _lib().dgtta_affine_warp3d_bwd(gp, ptr(th), sp, B, C, Ds, Hs, Ws, Dd, Hd, Wd, o.ndhwc, sld, dld, PAD[o.pad], o.algebra,
                                        stream_of())
    torch.cuda.synchronize()
    assert rc == expect, f"affine_warp3d_bwd returned {rc}: {_lib().dgtta_last_error().decode(errors='replace')}"
    if o.ndhwc:
        gs.assert_padding_untouched("warp_bwd grad_src")
        assert torch.equal(gd.get().view(-1), g.reshape(-1)), "the backward modified grad_dst"
        return gs.get().view(B, Ds, Hs, Ws, C)
    return gs_t.permute(0, 2, 3, 4, 1).contiguous().cpu()


def k_head_fwd(z_t, w, bias, sel, nsel, theta, algebra, dt):
    """dgtta_seghead_warp_fwd on z_t [B, D, H, W, 32] in the storage type (CPU) -> [B, D, H, W, nsel] float32 (CPU)."""
    from dg_tta_amd._lib import check, ptr, stream_of
    B, D, H, W, _ = z_t.shape
    zr = Rows(B * D * H * W, CIN, CIN, math.nan, z_t, dtype=TDT[dt])
    out = Rows(B * D * H * W, nsel, nsel, SENTINEL)
    wd, bd, th = w.to(DEV), bias.to(DEV), theta.to(DEV)
    sd = None if sel is None else sel.to(DEV)
    check(_lib().dgtta_seghead_warp_fwd(zr.ptr, ptr(wd), ptr(bd), ptr(sd), nsel, ptr(th), out.ptr, B, CIN, D, H, W, algebra, dt,
                                        stream_of()), "seghead_warp_fwd")
    torch.cuda.synchronize()
    out.assert_padding_untouched("seghead_warp_fwd out")
    assert torch.equal(zr.get().view(torch.int16), z_t.reshape(-1, CIN).view(torch.int16)), "the forward modified z"
    return out.get().view(B, D, H, W, nsel)


def k_head_bwd(z_t, gout, theta, w, sel, nsel, dt, o):
    """dgtta_seghead_warp_bwd (gout float32) / _bwd_g16 (gout in the storage type).  o: algebra, accumulate, dw0 / db0 (pre-loaded
    values or None = NaN), want_dw, want_db.  -> (rc, gz [B, D, H, W, 32] as stored, dw [nsel, 32] or None, db [nsel] or None)."""
    from dg_tta_amd._lib import ptr, stream_of
    lib = _lib()
    B, D, H, W, _ = z_t.shape
    n = B * D * H * W
    zr = Rows(n, CIN, CIN, math.nan, z_t, dtype=TDT[dt])
    g16 = gout.dtype != torch.float32
    gr = Rows(n, nsel, nsel, math.nan, gout, dtype=gout.dtype)
    gz = Rows(n, CIN, CIN, SENTINEL, dtype=TDT[dt])
    dw = Rows(nsel, CIN, CIN, SENTINEL, o.dw0) if o.want_dw else None
    db = Rows(1, nsel, nsel, SENTINEL, o.db0) if o.want_db else None
    wd, th = w.to(DEV), theta.to(DEV)
    h_theta = theta.clone().contiguous()
    sd = None if sel is None else sel.to(DEV)
    nws = lib.dgtta_seghead_warp_bwd_ws_bytes(B, CIN, nsel, D, H, W)
    assert nws > 0
    ws = torch.full((nws + 64,), 0xFF, dtype=torch.uint8, device=DEV)            # all-ones: NaN in every float type
    fn = lib.dgtta_seghead_warp_bwd_g16 if g16 else lib.dgtta_seghead_warp_bwd
    rc = fn(zr.ptr, gr.ptr, ptr(th), h_theta.data_ptr(), ptr(wd), ptr(sd), nsel, gz.ptr, dw.ptr if dw else None, db.ptr if db else None,
            ptr(ws), nws, B, CIN, D, H, W, o.algebra, o.accumulate, dt, stream_of())
    torch.cuda.synchronize()
    assert bool((ws[nws:] == 0xFF).all()), "seghead_warp_bwd wrote past its workspace"
    for r, what in ((gz, "gz"), (dw, "dw"), (db, "db")):
        if r is not None:
            r.assert_padding_untouched(f"seghead_warp_bwd {what}")
    assert torch.equal(zr.get().view(torch.int16), z_t.reshape(-1, CIN).view(torch.int16)), "the backward modified z"
    return rc, gz.get().view(B, D, H, W, CIN), (dw.get() if dw else None), (db.get().view(-1) if db else None)


def k_head_bwd_unfused(p, gl):
    """dgtta_seghead_bwd (Cin = lddx = 32, lddo = nsel: head_dgrad_lds_kernel) on the fp32 logit gradient gl [B, D, H, W, nsel]
    of problem p -> (dx [B, D, H, W, 32] as stored, dw [nsel, 32], db [nsel])."""
    from dg_tta_amd._lib import check, ptr, stream_of
    lib = _lib()
    B, D, H, W, _ = p.z_t.shape
    V, nsel, dt = D * H * W, p.nsel, p.dt
    zr = Rows(B * V, CIN, CIN, math.nan, p.z_t, dtype=TDT[dt])
    glr = Rows(B * V, nsel, nsel, math.nan, gl)
    dx = Rows(B * V, CIN, CIN, SENTINEL, dtype=TDT[dt])
    dw2, db2 = Rows(nsel, CIN, CIN, SENTINEL), Rows(1, nsel, nsel, SENTINEL)
    nws = lib.dgtta_seghead_bwd_ws_bytes(B, CIN, nsel, V)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=DEV)
    wd, sd = p.w.to(DEV), (None if p.sel is None else p.sel.to(DEV))
    check(lib.dgtta_seghead_bwd(zr.ptr, CIN, glr.ptr, nsel, ptr(wd), ptr(sd), nsel, dx.ptr, CIN, dw2.ptr, db2.ptr, ptr(ws), nws, B, CIN, V, 0,
                                dt, stream_of()), "seghead_bwd")
    torch.cuda.synchronize()
    return dx.get().view(B, D, H, W, CIN), dw2.get(), db2.get().view(-1)


# ------------------------------------------------------------------------------------------------ a. forward, every branch
def FC(id, branch, B, C, src, maps, dst=None, interps=("linear",), **kw):
    return SimpleNamespace(id=id, branch=branch, B=B, C=C, src=src, dst=dst or src, maps=maps, interps=interps, o=kw)


FWD_CASES = [
    # warp_fwd_rows4_kernel: NDHWC, C % 4 == 0, 16-byte rows, linear.  H ragged against WARP_ROWS = 8 everywhere.
    FC("rows4-B3-C16-7x13x37", "rows4", 3, 16, (7, 13, 37), [("tta008", "strong", "rot_z")]),      # three maps in one call
    FC("rows4-C4-5x11x18-ld+4+8-border-sub", "rows4", 1, 4, (5, 11, 18), ALL, lds=(4, 8), pad="border", algebra=0, sub=0.7),
    FC("rows4-C8-7x9x21-zeros-sub", "rows4", 2, 8, (7, 9, 21), ALL, sub=-1.3),
    FC("rows4-C8-resize", "rows4", 2, 8, (5, 6, 18), RESIZE, dst=(7, 9, 21), algebra=0),
    FC("rows4-C4-1x9x21", "rows4", 1, 4, (1, 9, 21), ALL),                                         # a size-1 axis
    # warp_fwd_kernel<4, true>: the same operands with nearest interpolation
    FC("vec4-nearest-C8-7x9x21", "kernel<4,true>", 2, 8, (7, 9, 21), NEAREST, interps=("nearest",)),
    FC("vec4-nearest-C4-border-sub-ld+4", "kernel<4,true>", 1, 4, (5, 11, 18), NEAREST, interps=("nearest",), pad="border", sub=0.7,
       lds=(4, 4), algebra=0),
    # warp_fwd_kernel<1, true>: C = 5; ld no multiple of 4; a base pointer 4 bytes off
    FC("scalar-C5-7x9x21", "kernel<1,true>", 1, 5, (7, 9, 21), ALL),
    FC("scalar-C5-nearest", "kernel<1,true>", 2, 5, (7, 9, 21), NEAREST, interps=("nearest",), sub=0.7),
    FC("scalar-C8-ld+1-border-sub", "kernel<1,true>", 2, 8, (5, 6, 18), ALL, lds=(1, 1), pad="border", sub=0.7, algebra=0),
    FC("scalar-C8-src+4B", "kernel<1,true>", 1, 8, (5, 6, 18), NEAREST, interps=("linear", "nearest"), leads=(1, 0)),
    FC("scalar-C8-dst+4B-resize", "kernel<1,true>", 1, 8, (7, 9, 21), RESIZE, dst=(5, 6, 18), leads=(0, 1)),
    # warp_fwd_kernel<1, false>: NCDHW
    FC("ncdhw-C3-7x9x21", "kernel<1,false>", 2, 3, (7, 9, 21), ALL, ndhwc=0),
    FC("ncdhw-C3-border-sub", "kernel<1,false>", 1, 3, (5, 6, 18), NEAREST, interps=("linear", "nearest"), ndhwc=0, pad="border",
       sub=0.7, algebra=0),
    FC("ncdhw-C2-resize-1x6x9", "kernel<1,false>", 1, 2, (1, 6, 9), RESIZE, dst=(2, 5, 11), ndhwc=0),
]


def _fwd_branch(c):
    """The dispatch of dgtta_affine_warp3d_fwd restated: which kernel the case's operands select."""
    if not c.o.get("ndhwc", 1):
        return "kernel<1,false>"
    lds, leads = c.o.get("lds", (0, 0)), c.o.get("leads", (0, 0))
    v4 = c.C % 4 == 0 and (c.C + lds[0]) % 4 == 0 and (c.C + lds[1]) % 4 == 0 and leads[0] % 4 == 0 and leads[1] % 4 == 0
    if not v4:
        return "kernel<1,true>"
    return "rows4" if c.interps == ("linear",) else "kernel<4,true>"


@pytest.mark.parametrize("c", FWD_CASES, ids=lambda c: c.id)
def test_warp_forward_vs_float64(c):
    assert _fwd_branch(c) == c.branch
    x = _volume(c.B, c.src, c.C, 1)
    x64 = x.double()
    worst = 0.0
    for interp in c.interps:
        o = _opts(interp=interp, **c.o)
        sub = 0.0 if o.sub is None else float(torch.tensor(o.sub, dtype=torch.float32))
        for names in _batches(c.maps, c.B):
            theta = _thetas(names, c.dst, c.src)
            got = k_warp_fwd(x, theta, c.dst, o)
            tag = f"a {c.id} {interp} {'+'.join(names)}"
            if interp == "linear":
                ref = wref.warp(x64, theta, c.dst, o.pad, "linear", sub)
                worst = max(worst, _within(tag, got.double(), ref, _fwd_bound(x64, sub, theta, c.dst, o.pad, o.algebra, ref)))
                if "outside" in names and o.pad == "zeros":
                    b = names.index("outside")
                    assert bool((got[b] == torch.tensor(sub, dtype=torch.float32)).all()), "samples outside the volume must give `sub`"
                continue
            # nearest: bit for bit away from the rounding ties
            delta = _delta(theta, c.src, o.algebra)
            assert float(delta.max()) < 1e-4
            pos = wref._padded(wref.sample_positions(theta, c.dst, c.src), c.src, o.pad)
            tie = torch.zeros_like(pos[0], dtype=torch.bool)
            for p in pos:
                tie |= ((p - p.floor()) - 0.5).abs() < 1e-4
            share = float(tie.float().mean())
            assert share < 0.01, f"{tag}: {share:.2%} of the samples are within 1e-4 of a tie"
            idx, inb = wref._flat_index(*(p.round().long() for p in pos), c.src)
            s32 = torch.tensor(sub, dtype=torch.float32)
            ref32 = torch.where(inb[..., None], x.reshape(-1, c.C)[idx] - s32, torch.zeros(())) + s32         # fp32, as the kernel
            keep = ~tie
            print(f"RATIO {tag}: {int(keep.sum())} of {keep.numel()} samples compared bit for bit")
            assert not bool(torch.isnan(got).any())
            assert torch.equal(got[keep], ref32[keep]), f"{tag}: nearest differs from the copied value"
    print(f"GROUP a forward {c.branch}: {worst:.3f}")


# ------------------------------------------------------------------------------------------------ b. backward
BWD_CASES = [
    # warp_bwd_gather_kernel<16, true>; sizes ragged against the 16 x 4 x 4 tile
    FC("gather-vec-B2-C16-7x9x21", "gather<16,true>", 2, 16, (7, 9, 21), ALL),
    FC("gather-vec-C4-5x6x18-ld+4+8", "gather<16,true>", 1, 4, (5, 6, 18), ALL, lds=(4, 8), algebra=0),
    # several channel tiles, the last one partial
    FC("gather-vec-C20-5x6x18", "gather<16,true>", 1, 20, (5, 6, 18), ["tta008", "rot_z", "strong", "diag038", "identity"]),
    FC("gather-vec-C36-4x5x17", "gather<16,true>", 1, 36, (4, 5, 17), ["tta008", "perm", "strong", "diag038", "shift_half"]),
    FC("gather-vec-resize", "gather<16,true>", 2, 8, (5, 6, 18), RESIZE, dst=(7, 9, 21)),
    FC("gather-vec-1x2x64", "gather<16,true>", 1, 4, (1, 2, 64), ALL),
    # warp_bwd_gather_kernel<16, false>: C = 5, ld no multiple of 4, a misaligned base
    FC("gather-scalar-C5-5x6x18", "gather<16,false>", 1, 5, (5, 6, 18), ALL),
    FC("gather-scalar-C21-ld+2", "gather<16,false>", 1, 21, (4, 5, 17), ["tta008", "rot_x", "strong", "diag029"], lds=(2, 1)),
    FC("gather-scalar-C8-out+4B", "gather<16,false>", 2, 8, (7, 9, 21), ["tta008", "rot_y", "strong", "identity"], leads=(1, 0)),
    FC("gather-scalar-C8-g+4B", "gather<16,false>", 1, 8, (5, 6, 18), ["tta008", "rot_z_eps", "shear", "magnify"], leads=(0, 1)),
    # the atomic scatter: border padding (NDHWC, rows wider than C: only the operand columns may be zeroed) and NCDHW
    FC("scatter-ndhwc-border-C8-ld+4", "scatter<1,true>", 2, 8, (5, 6, 18), ALL, pad="border", lds=(4, 0)),
    FC("scatter-ndhwc-border-C5", "scatter<1,true>", 1, 5, (7, 9, 21), ["tta008", "strong", "outside", "rot_z"], pad="border", algebra=0),
    FC("scatter-ncdhw-zeros-C3", "scatter<1,false>", 2, 3, (7, 9, 21), ALL, ndhwc=0),
    FC("scatter-ncdhw-border-resize", "scatter<1,false>", 1, 3, (5, 6, 18), RESIZE, dst=(7, 9, 21), ndhwc=0, pad="border"),
]


def _bwd_branch(c):
    o = _opts(**c.o)
    if not o.ndhwc:
        return "scatter<1,false>"
    if o.pad != "zeros":
        return "scatter<1,true>"
    vec = c.C % 4 == 0 and (c.C + o.lds[0]) % 4 == 0 and (c.C + o.lds[1]) % 4 == 0 and o.leads[0] % 4 == 0 and o.leads[1] % 4 == 0
    return "gather<16,true>" if vec else "gather<16,false>"


@pytest.mark.parametrize("c", BWD_CASES, ids=lambda c: c.id)
def test_warp_backward_vs_float64_and_gather_vs_scatter(c):
    """1. grad_src against warp_adjoint in float64.  2. Where the call takes the owner-computes gather (NDHWC, zeros): the same
    grad_dst and theta through the NCDHW entry (atomic scatter, corners() straight from the forward) - the same fp32 terms
    in another order, so the two agree to 2 (n - 1) u sum |terms| per element; a candidate the search drops shows here."""
    assert _bwd_branch(c) == c.branch
    o = _opts(**c.o)
    g = _volume(c.B, c.dst, c.C, 2)
    g64 = g.double()
    worst = [0.0, 0.0]
    for names in _batches(c.maps, c.B):
        theta = _thetas(names, c.dst, c.src)
        adj = _adjoint(g64, theta, c.src, o.pad, o.algebra)
        got = k_warp_bwd(g, theta, c.src, o)
        tag = f"b {c.id} {'+'.join(names)}"
        worst[0] = max(worst[0], _within(tag, got.double(), adj.ref, adj.bound))
        for b, name in enumerate(names):
            if name == "outside" and o.pad == "zeros":
                assert not bool(got[b].any()), "no sample inside the volume: the gradient is zero"
        if c.branch.startswith("gather"):
            scat = k_warp_bwd(g, theta, c.src, _opts(ndhwc=0, algebra=o.algebra))
            err = (got.double() - scat.double()).abs()
            at = int(torch.nan_to_num(err / adj.order.clamp(min=1e-300), nan=math.inf).argmax())
            print(f"  (largest gather - scatter difference {float(err.view(-1)[at]):.3e} at an element of n = {int(adj.n.view(-1)[at // c.C])} candidates)")
            worst[1] = max(worst[1], _within(f"{tag} gather vs scatter", got.double(), scat.double(), adj.order))
    print(f"GROUP b backward {c.branch}: vs float64 {worst[0]:.3f}, gather vs scatter {worst[1]:.3f}")


def test_warp_backward_batch_of_accepted_and_declined_maps():
    """One call, B = 3: the gather handles the accepted map and returns at once for the singular one and for diag(0.28)
    (540 candidates per voxel), which warp_bwd_zero_if_declined_kernel zeroes and warp_bwd_kernel (only_declined) scatters.
    Rows wider than C: the zeroing may touch the operand columns only."""
    names = ("tta008", "singular", "diag028")
    size, C = (7, 9, 21), 16
    g = _volume(3, size, C, 3)
    theta = _thetas(names, size)
    for o in (_opts(lds=(4, 0)), _opts(lds=(1, 1))):                     # the 16-byte and the scalar gather
        adj = _adjoint(g.double(), theta, size, "zeros", 1)
        got = k_warp_bwd(g, theta, size, o)
        for b, name in enumerate(names):
            _within(f"b mixed ld+{o.lds[0]} {name}", got[b].double(), adj.ref[b], adj.bound[b])
        assert float(got[1].abs().max()) > 0 and float(got[2].abs().max()) > 0
    # B = 17: the declined-batch table of the scatter has 16 entries
    g17 = _volume(17, (2, 3, 5), 4, 4)
    out = k_warp_bwd(g17, _thetas(("identity",) * 17, (2, 3, 5)), (2, 3, 5), _opts(), expect=UNSUPPORTED)
    assert bool(torch.isnan(out).all()), "a refused call wrote grad_src"


# ------------------------------------------------------------------------------------------------ c. fused forward
def HC(id, B, size, dt, nsel, with_sel, maps, algebra=1):
    return SimpleNamespace(id=id, B=B, size=size, dt=dt, nsel=nsel, with_sel=with_sel, maps=maps, algebra=algebra)


HEAD_FWD_CASES = [   # W = 17, 64, 65, 70: one and two 64-voxel tiles, both ragged; H ragged against 8
    HC("W17-B2-bf16-nsel8-sel", 2, (3, 11, 17), 1, 8, True, ALL),
    HC("W17-fp16-nsel16", 1, (3, 11, 17), 2, 16, False, ALL),
    HC("W64-fp16-nsel4-sel", 1, (2, 9, 64), 2, 4, True, ["tta008", "rot_x", "strong", "outside", "shift_half", "identity"]),
    HC("W65-bf16-nsel12", 1, (2, 5, 65), 1, 12, False, ["tta008", "rot_z", "strong", "diag038", "reflect"], algebra=0),
    HC("W70-B2-fp16-nsel12-sel", 2, (2, 10, 70), 2, 12, True, ["tta008", "strong", "perm", "shift_int", "magnify", "shear"]),
    HC("W70-bf16-nsel16-sel", 1, (1, 3, 70), 1, 16, True, ["tta008", "rot_y", "outside", "singular"]),
    HC("W17-bf16-nsel4", 1, (4, 6, 17), 1, 4, False, ["tta008", "rot_z_eps", "diag028", "shift_half"]),
]


@functools.lru_cache(maxsize=None)
def _head_fwd_reference(B, size, dt, nsel, with_sel, names, algebra):
    """Storage-rounded z, reference and bound of one fused forward call; shared by the two kernels."""
    w, bias = _head_params()
    sel = _sel(nsel, with_sel)
    z_t = _volume(B, size, CIN, 5).to(TDT[dt])
    z64 = z_t.double()
    theta = _thetas(names, size)
    idx = None if sel is None else sel.long()
    ws64, bs64 = (w[:nsel] if idx is None else w[idx]).double(), (bias[:nsel] if idx is None else bias[idx]).double()
    logits = z64 @ ws64.t() + bs64
    ref = wref.warp(logits, theta, size)
    d = _delta(theta, size, algebra)
    terms = wref.warp(z64.abs(), theta, size) @ ws64.abs().t() + bs64.abs() * wref.warp(torch.ones(B, *size, 1, dtype=torch.float64), theta, size)
    bound = _position_term(logits, theta, size, "zeros", d) + 48 * U * terms + 2 * U * ref.abs()
    # the bias enters scaled by the in-volume weight: where no corner is inside, the logit is exactly zero
    return SimpleNamespace(z_t=z_t, theta=theta, ref=ref, bound=bound, w=w, bias=bias, sel=sel)


@pytest.mark.parametrize("kernel", ["mfma", "fma"])
@pytest.mark.parametrize("c", HEAD_FWD_CASES, ids=lambda c: c.id)
def test_head_warp_forward_vs_float64(c, kernel, monkeypatch):
    """head_warp_fwd_mfma_kernel (the default) and head_warp_fwd_kernel (DGTTA_HEADWARP_MFMA=0) against head_then_warp."""
    if kernel == "fma":
        monkeypatch.setenv("DGTTA_HEADWARP_MFMA", "0")
    reload_kernel_switches()
    worst = 0.0
    for names in _batches(c.maps, c.B):
        r = _head_fwd_reference(c.B, c.size, c.dt, c.nsel, c.with_sel, names, c.algebra)
        nrow = None if c.with_sel else c.nsel
        got = k_head_fwd(r.z_t, r.w[:nrow] if nrow else r.w, r.bias[:nrow] if nrow else r.bias, r.sel, c.nsel, r.theta, c.algebra, c.dt)
        worst = max(worst, _within(f"c {c.id} {kernel} {'+'.join(names)}", got.double(), r.ref, r.bound))
        for b, name in enumerate(names):
            if name == "outside":
                assert not bool(got[b].any()), "no corner inside the volume: the bias must not enter"
    print(f"GROUP c fused forward {kernel}: {worst:.3f}")


# ------------------------------------------------------------------------------------------------ d. fused backward
HEAD_BWD_SHAPES = [(1, 8, 8, 18), (2, 5, 12, 32), (1, 6, 10, 64), (1, 1, 2, 64)]      # B D H W a multiple of 128, ragged tiles
# (dt, gout in the storage type, nsel, sel set, accumulate, dw wanted, db wanted): dealt to the maps in turn
# nsel = 4 / 12: no weight gradient (its matrix-core plan reads rows of 8 or 16 classes; refused up front, see e.)
HEAD_BWD_CONFIGS = [
    (1, False, 16, True, 0, True, True), (2, True, 8, False, 0, True, True), (2, False, 12, True, 1, False, True),
    (1, True, 4, True, 1, False, True), (1, False, 8, True, 0, False, True), (2, False, 16, False, 0, True, False),
    (2, True, 12, False, 0, False, False), (1, True, 16, False, 1, True, True), (2, False, 4, False, 0, False, True),
    (2, False, 8, True, 1, True, False),
]


def _head_bwd_problem(B, size, names, cfg, seed=6):
    dt, g16, nsel, with_sel, accumulate, want_dw, want_db = cfg
    w, _ = _head_params()
    sel = _sel(nsel, with_sel)
    z_t = _volume(B, size, CIN, seed).to(TDT[dt])
    gout = _volume(B, size, nsel, seed + 1)
    gout = gout.to(TDT[dt]) if g16 else gout
    theta = _thetas(names, size)
    gen = torch.Generator().manual_seed(nsel)
    dw0 = torch.randn(nsel, CIN, generator=gen) * 50 if accumulate else None
    db0 = torch.randn(nsel, generator=gen) * 50 if accumulate else None
    o = SimpleNamespace(algebra=1, accumulate=accumulate, dw0=dw0, db0=db0, want_dw=want_dw, want_db=want_db)
    return SimpleNamespace(dt=dt, nsel=nsel, sel=sel, w=w if with_sel else w[:nsel].contiguous(), z_t=z_t, gout=gout, theta=theta, o=o)


def _check_head_bwd(tag, p, gz, dw, db):
    """gz, dw, db of one fused backward call against float64, with the bounds of the module docstring."""
    dt, size = p.dt, tuple(p.z_t.shape[1:4])
    idx = None if p.sel is None else p.sel.long()
    ws64 = (p.w if idx is None else p.w[idx]).double()
    z64, g64 = p.z_t.double(), p.gout.double()
    adj = _adjoint(g64, p.theta, size, "zeros", p.o.algebra)
    gl = adj.ref
    e32 = adj.bound @ ws64.abs() + 16 * U * (gl.abs() @ ws64.abs())
    gz_ref = gl @ ws64
    ratios = [_within(f"{tag} gz", gz.double(), gz_ref, U_T[dt] * (gz_ref.abs() + e32) + SUB_T[dt] + e32)]
    if dw is not None:
        e16 = adj.bound + U_T[dt] * (gl.abs() + adj.bound) + SUB_T[dt]
        N = z64.shape[0] * size[0] * size[1] * size[2]
        ref = torch.einsum("bdhwk,bdhwc->kc", gl, z64) + (p.o.dw0.double() if p.o.accumulate else 0.0)
        bound = torch.einsum("bdhwk,bdhwc->kc", e16, z64.abs()) + N * U * torch.einsum("bdhwk,bdhwc->kc", gl.abs(), z64.abs())
        ratios.append(_within(f"{tag} dw", dw.double(), ref, bound + (2 if p.o.accumulate else 1) * U * ref.abs()))
    if db is not None:
        ref = gl.sum(dim=(0, 1, 2, 3)) + (p.o.db0.double() if p.o.accumulate else 0.0)
        bound = adj.bound.sum(dim=(0, 1, 2, 3)) + 2.0 ** -18 * gl.abs().sum(dim=(0, 1, 2, 3))
        ratios.append(_within(f"{tag} db", db.double(), ref, bound + (2 if p.o.accumulate else 1) * U * ref.abs()))
    return ratios, gl


@pytest.mark.parametrize("shape", HEAD_BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_warp_backward_vs_float64(shape):
    """head_warp_bwd_kernel<T, false, G16> + the matrix-core weight gradient + head_warp_bias_finalize_kernel over the whole
    host-accepted part of the map list; the configurations (storage type, gout type, nsel, sel, accumulate, dw / db NULL) are
    dealt to the maps in turn, starting at a different one per shape.  The host accepts every one of these maps at every one of
    these shapes (the TTA draw on the flattest volume has 123 candidates per voxel): a refusal here is a failure."""
    B, size = shape[0], tuple(shape[1:])
    lib = _lib()
    worst = 0.0
    for i, names in enumerate(_batches([m for m in ALL if m not in HOST_REFUSED], B)):
        cfg = HEAD_BWD_CONFIGS[(i + HEAD_BWD_SHAPES.index(shape) * 2) % len(HEAD_BWD_CONFIGS)]
        p = _head_bwd_problem(B, size, names, cfg)
        tag = f"d {'x'.join(map(str, shape))} {'+'.join(names)} cfg{cfg}"
        sup = lib.dgtta_seghead_warp_supported(p.theta.data_ptr(), B, CIN, 8 * ((p.nsel + 7) // 8), *size, p.dt)      # (the maps)
        assert lib.dgtta_seghead_warp_supported(p.theta.data_ptr(), B, CIN, p.nsel, *size, p.dt) == (sup if p.nsel % 8 == 0 else 0)
        rc, gz, dw, db = k_head_bwd(p.z_t, p.gout, p.theta, p.w, p.sel, p.nsel, p.dt, p.o)
        assert sup == 1 and rc == OK, f"{tag}: supported() = {sup}, the backward returned {rc}"
        ratios, gl = _check_head_bwd(tag, p, gz, dw, db)
        worst = max(worst, *ratios)
        for b, name in enumerate(names):
            if name == "outside":
                assert not bool(gz[b].float().any())
            if name == "diag038":        # accepted: the true gradient, not zeros
                assert float(gl[b].abs().max()) > 0.1 and float(gz[b].float().abs().max()) > 0.01
    print(f"GROUP d fused backward {'x'.join(map(str, shape))}: {worst:.3f}")


@pytest.mark.parametrize("case", [((1, 8, 8, 18), "rot_z", 1, 16), ((1, 8, 8, 18), "diag038", 2, 8), ((2, 5, 12, 32), "perm", 2, 16),
                                  ((1, 6, 10, 64), "diag038", 1, 12), ((1, 1, 2, 64), "rot_y", 2, 4), ((2, 5, 12, 32), "strong", 1, 8),
                                  ((1, 8, 8, 18), "shear", 2, 16)],
                         ids=lambda c: "{}-{}-dt{}-nsel{}".format("x".join(map(str, c[0])), *c[1:]))
def test_head_warp_backward_equals_the_two_step_path_bit_for_bit(case):
    """gz and (nsel = 8 / 16) dw of the fused backward against dgtta_affine_warp3d_bwd (C = ldc = nsel: warp_bwd_gather_kernel<16, true>, the
    same candidate search and accumulation order) followed by dgtta_seghead_bwd (Cin = lddx = 32, lddo = nsel:
    head_dgrad_lds_kernel, the same k-ordered fmaf chain and the same 16-bit copy for the weight gradient): BIT for bit.
    db differs by its reduction order: within the sum of both paths' bounds."""
    shape, name, dt, nsel = case
    B, size = shape[0], tuple(shape[1:])
    want_dw = nsel % 8 == 0
    p = _head_bwd_problem(B, size, (name,) * B if B == 1 else (name, "tta008"), (dt, False, nsel, True, 0, want_dw, True))
    rc, gz, dw, db = k_head_bwd(p.z_t, p.gout, p.theta, p.w, p.sel, p.nsel, p.dt, p.o)
    assert rc == OK
    _check_head_bwd(f"d2 {case}", p, gz, dw, db)
    gl = k_warp_bwd(p.gout, p.theta, size, _opts())                                   # fp32 logit gradient, rows of nsel
    two, dw2, db2 = k_head_bwd_unfused(p, gl)
    assert not bool(torch.isnan(gz.float()).any())
    assert torch.equal(gz.view(torch.int16), two.view(torch.int16)), "gz differs from warp_bwd followed by seghead_bwd"
    if want_dw:
        assert torch.equal(dw, dw2), "dw differs from warp_bwd followed by seghead_bwd"
    adj = _adjoint(p.gout.double(), p.theta, size, "zeros", 1)
    tot = adj.ref.abs().sum(dim=(0, 1, 2, 3))
    # (fused: wave sums of 64, 2^-18; dgtta_seghead_bwd: a thread adds up to 64 fp32 terms before double, 2^-18; a rounding each)
    _within(f"d2 {case} db vs two-step", db.double(), db2.double(), 2 * (2.0 ** -18 * tot + U * tot))


LATTICE_MAPS = ["identity", "shift_int", "shift_half", "rot_x", "rot_y", "rot_z", "perm", "rot_z_eps", "reflect", "outside"]


@pytest.mark.parametrize("case", [((1, 8, 8, 18), 1, 16), ((2, 5, 12, 32), 2, 8), ((1, 6, 10, 64), 2, 16), ((1, 1, 2, 64), 1, 8)],
                         ids=lambda c: "{}-dt{}-nsel{}".format("x".join(map(str, c[0])), *c[1:]))
def test_head_warp_backward_of_a_sparse_gradient_equals_scatter_then_head_bit_for_bit(case):
    """The fused kernel's own copy of the candidate search, at the accuracy of a single dropped term.  The logit gradient is
    non-zero on every third destination voxel per axis; the maps take the lattice to itself (up to 1e-5 for rot_z_eps), so the
    corner sets of two such samples are at least one voxel apart and every feature-map voxel receives at most one term
    (asserted from the float64 candidates, rounding tolerance included).  No sum is formed, so the gathered gradient equals
    the atomic scatter's (dgtta_affine_warp3d_bwd, NCDHW: corners() straight from the forward, no search) bit for bit, and gz
    equals dgtta_seghead_bwd on it bit for bit.  On the lattice maps the fp32 positions fall a few ulp beside lattice points:
    the candidates at distance 1 - a few ulp, with weights of 1e-6 and less, are exactly the ones the slack of the search
    (+0.02, 1.02) is there to keep.  (With the slack removed from both kernels these cases still pass on an MI355X: what fails
    then is the gather-against-scatter comparison of dgtta_affine_warp3d_bwd, rot_x+rot_y and shift_half+diag038.)"""
    shape, dt, nsel = case
    B, size = shape[0], tuple(shape[1:])
    worst_small = math.inf
    for names in _batches(LATTICE_MAPS, B):
        p = _head_bwd_problem(B, size, names, (dt, False, nsel, True, 0, False, False))
        mask = torch.zeros(B, *size, 1)
        mask[:, ::3, ::3, ::3] = 1.0
        p.gout = (p.gout * mask * 1024.0).contiguous()
        d = _delta(p.theta, size, 1)
        tol = tuple(d[:, a].view(-1, 1, 1, 1) for a in range(3))
        _, hits = wref.candidate_sums(mask.double(), p.theta, size, "zeros", tol)
        assert float(hits.max()) <= 1.0, "a voxel has two candidates: the comparison would depend on the order of a sum"
        rc, gz, _, _ = k_head_bwd(p.z_t, p.gout, p.theta, p.w, p.sel, p.nsel, p.dt, p.o)
        assert rc == OK
        scat = k_warp_bwd(p.gout, p.theta, size, _opts(ndhwc=0))
        two, _, _ = k_head_bwd_unfused(p, scat)
        nz = scat.abs().amax(dim=-1)
        small = nz[(nz > 0)]
        if small.numel():
            worst_small = min(worst_small, float(small.min()))
        tag = f"d3 {'x'.join(map(str, shape))} {'+'.join(names)}"
        print(f"RATIO {tag}: {int((nz > 0).sum())} voxels with a term, the smallest {float(small.min()) if small.numel() else 0.0:.3e}")
        assert not bool(torch.isnan(gz.float()).any())
        assert torch.equal(gz.view(torch.int16), two.view(torch.int16)), f"{tag}: gz differs from scatter followed by seghead_bwd"
        for b, name in enumerate(names):
            if float(scat[b].abs().max()) > 0:
                assert float(gz[b].float().abs().max()) > 0
    print(f"GROUP d3 sparse gradient {'x'.join(map(str, shape))}: bit for bit; smallest term {worst_small:.3e}")


# ------------------------------------------------------------------------------------------------ e. acceptance, arguments
@pytest.mark.parametrize("shape", [(1, 8, 8, 18), (1, 1, 2, 64), (1, 6, 10, 64)], ids=lambda s: "x".join(map(str, s)))
def test_supported_agrees_with_what_the_backward_accepts(shape):
    """host_map_ok() against the device's inverse_map(): the fused backward has no scatter fallback, so a map the host accepts
    and the device declines would give a silent zero gradient.  For every map of the list: supported() == (the backward
    returns OK); refused -> DGTTA_ERR_UNSUPPORTED and nothing written; accepted -> the gradient is correct (the float64
    comparison, which a zero gradient fails).  The acceptance edge: diag(0.38) (245.7 candidates) is accepted, 0.37 (262.8),
    0.29 (492), 0.28 (540) and the singular map are refused; any other map is accepted below 250 and refused above 262."""
    B, size = shape[0], tuple(shape[1:])
    lib = _lib()
    cfg = (1, False, 8, True, 0, True, True)
    for name in ALL:
        p = _head_bwd_problem(B, size, (name,), cfg)
        sup = lib.dgtta_seghead_warp_supported(p.theta.data_ptr(), B, CIN, p.nsel, *size, p.dt)
        rc, gz, dw, db = k_head_bwd(p.z_t, p.gout, p.theta, p.w, p.sel, p.nsel, p.dt, p.o)
        vol = _vol64(p.theta[0], size)
        print(f"ACCEPT {'x'.join(map(str, shape))} {name}: candidates {vol:.1f} supported {sup} rc {rc}")
        assert (rc == OK) == bool(sup), f"{name}: supported() = {sup} but the backward returned {rc}"
        if name in HOST_REFUSED or vol > 262:
            assert rc == UNSUPPORTED, name
        elif name == "diag038" or vol < 250:
            assert rc == OK, name
        if rc != OK:
            for t in (gz.float(), dw, db):
                assert bool(torch.isnan(t).all()), f"{name}: a refused call wrote an output"
        else:
            ratios, gl = _check_head_bwd(f"e {'x'.join(map(str, shape))} {name}", p, gz, dw, db)
            if name not in ("outside",) and float(gl.abs().max()) > 0:
                assert float(gz.float().abs().max()) > 0, f"{name}: accepted but the gradient is zero"


def test_argument_checks():
    """Refused calls launch nothing: every output keeps its fill."""
    from dg_tta_amd._lib import ptr, stream_of
    lib = _lib()
    B, size, nsel, dt = 1, (8, 8, 18), 8, 1
    D, H, W = size
    p = _head_bwd_problem(B, size, ("tta008",), (dt, False, nsel, True, 0, True, True))
    n = B * D * H * W
    h_theta = p.theta.clone().contiguous()
    sup = lib.dgtta_seghead_warp_supported
    assert sup(h_theta.data_ptr(), B, CIN, nsel, D, H, W, dt) == 1
    assert sup(h_theta.data_ptr(), B, CIN, 5, D, H, W, dt) == 0 and sup(h_theta.data_ptr(), B, CIN, 20, D, H, W, dt) == 0
    assert sup(h_theta.data_ptr(), B, 16, nsel, D, H, W, dt) == 0 and sup(h_theta.data_ptr(), B, CIN, nsel, D, H, W, 0) == 0
    assert sup(h_theta.data_ptr(), B, CIN, 4, D, H, W, dt) == 0 and sup(h_theta.data_ptr(), B, CIN, 12, D, H, W, dt) == 0      # (no dw)
    assert sup(h_theta.data_ptr(), B, CIN, 16, D, H, W, dt) == 1
    assert sup(None, B, CIN, nsel, D, H, W, dt) == 0 and sup(h_theta.data_ptr(), B, CIN, nsel, D, H, 17, dt) == 0
    th17 = _thetas(("identity",) * 17, (1, 8, 16))
    assert sup(th17.data_ptr(), 17, CIN, nsel, 1, 8, 16, dt) == 0 and sup(th17.data_ptr(), 16, CIN, nsel, 1, 8, 16, dt) == 1
    wsb = lib.dgtta_seghead_warp_bwd_ws_bytes
    assert wsb(B, CIN, nsel, D, H, 17) == 0 and wsb(0, CIN, nsel, D, H, W) == 0 and wsb(B, CIN, nsel, D, H, 0) == 0
    nws = wsb(B, CIN, nsel, D, H, W)
    assert nws > 0

    zr = Rows(n, CIN, CIN, math.nan, p.z_t, lead=8, dtype=TDT[dt])              # (lead 8 elements = 16 bytes: still aligned)
    gr = Rows(n, nsel, nsel, math.nan, p.gout, lead=4)
    gz = Rows(n, CIN, CIN, math.nan, lead=8, dtype=TDT[dt])
    out = Rows(n, nsel, nsel, math.nan, lead=4)
    dw, db = torch.full((nsel, CIN), math.nan, device=DEV), torch.full((nsel,), math.nan, device=DEV)
    wd, sd, th = p.w.to(DEV), p.sel.to(DEV), p.theta.to(DEV)
    bias = _head_params()[1].to(DEV)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=DEV)
    th17d = th17.to(DEV)
    st = stream_of()

    def fwd(z=zr.ptr, w=ptr(wd), b=ptr(bias), k=nsel, t=ptr(th), o=out.ptr, bb=B, cin=CIN, ww=W, d=dt):
        return lib.dgtta_seghead_warp_fwd(z, w, b, ptr(sd), k, t, o, bb, cin, D, H, ww, 1, d, st)

    def bwd(fn, z=zr.ptr, g=gr.ptr, t=ptr(th), ht=h_theta.data_ptr(), w=ptr(wd), k=nsel, o=gz.ptr, wsp=ptr(ws), nb=nws, bb=B, cin=CIN,
            ww=W, d=dt):
        return fn(z, g, t, ht, w, ptr(sd), k, o, ptr(dw), ptr(db), wsp, nb, bb, cin, D, H, ww, 1, 0, d, st)

    assert fwd(z=None) == BADARG and fwd(w=None) == BADARG and fwd(b=None) == BADARG and fwd(t=None) == BADARG and fwd(o=None) == BADARG
    assert fwd(k=5) == UNSUPPORTED and fwd(k=20) == UNSUPPORTED and fwd(cin=16) == UNSUPPORTED and fwd(d=0) == UNSUPPORTED
    assert fwd(z=zr.ptr + 2) == BADARG and fwd(o=out.ptr + 4) == BADARG and fwd(bb=0) == BADARG
    for fn in (lib.dgtta_seghead_warp_bwd, lib.dgtta_seghead_warp_bwd_g16):
        call = functools.partial(bwd, fn)
        for name in ("z", "g", "t", "ht", "w", "o", "wsp"):
            assert call(**{name: None}) == BADARG, name
        assert call(k=5) == UNSUPPORTED and call(k=20) == UNSUPPORTED and call(cin=16) == UNSUPPORTED and call(d=0) == UNSUPPORTED
        assert call(k=4) == UNSUPPORTED and call(k=12) == UNSUPPORTED          # with dw_sel: the weight gradient needs rows of 8 / 16
        assert call(bb=17, t=ptr(th17d), ht=th17.data_ptr()) == BADARG                    # (B > 16 is a bad dimension here)
        assert call(ww=17) == UNSUPPORTED                                                 # rows no multiple of 128
        assert call(nb=nws - 1) == WORKSPACE
        assert call(g=gr.ptr + 4) == BADARG and call(o=gz.ptr + 2) == BADARG
    assert lib.dgtta_last_error()
    torch.cuda.synchronize()
    for t in (gz.get().float(), out.get(), dw.cpu(), db.cpu()):
        assert bool(torch.isnan(t).all()), "a refused call wrote an output"
    # and the same buffers are fine for a valid call
    assert fwd() == OK and bwd(lib.dgtta_seghead_warp_bwd) == OK
    torch.cuda.synchronize()
    assert not bool(torch.isnan(gz.get().float()).any()) and not bool(torch.isnan(out.get()).any())

    # dgtta_affine_warp3d_*: null pointers, bad dimensions, ldc < C, bad modes
    x = Rows(n, 4, 4, math.nan, _volume(1, size, 4, 1))
    y = Rows(n, 4, 4, math.nan)
    wf, wb = lib.dgtta_affine_warp3d_fwd, lib.dgtta_affine_warp3d_bwd
    assert wf(None, ptr(th), y.ptr, 1, 4, D, H, W, D, H, W, 1, 4, 4, 0, 0, 1, None, st) == BADARG
    assert wf(x.ptr, ptr(th), y.ptr, 1, 4, D, H, W, D, H, W, 1, 3, 4, 0, 0, 1, None, st) == BADARG
    assert wf(x.ptr, ptr(th), y.ptr, 1, 4, D, H, W, D, H, W, 1, 4, 4, 2, 0, 1, None, st) == BADARG
    assert wf(x.ptr, ptr(th), y.ptr, 1, 4, D, H, W, D, H, W, 1, 4, 4, 0, 2, 1, None, st) == BADARG
    assert wf(x.ptr, ptr(th), y.ptr, 1, 4, D, 0, W, D, H, W, 1, 4, 4, 0, 0, 1, None, st) == BADARG
    assert wb(x.ptr, ptr(th), None, 1, 4, D, H, W, D, H, W, 1, 4, 4, 0, 1, st) == BADARG
    assert wb(x.ptr, ptr(th), y.ptr, 1, 4, D, H, W, D, H, W, 1, 4, 3, 0, 1, st) == BADARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.get()).all()), "a refused call wrote an output"
