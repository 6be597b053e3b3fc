"""GPU: the InstanceNorm + LeakyReLU kernels of instnorm.hip, called through the C ABI, against the float64 restatement
tests/instnorm_ref.py (licensed by tests/test_instnorm_ref.py) at every branch of the dispatch: scalar / 16-byte
reductions, scalar / fast / slow apply kernels, statistics and backward sums from the kernel's own reduction pass or
from per-tile partial sums with a device-side header, accumulate 0 / 1, strided rows, the block-count caps, tiny V.

Each stage is isolated so that its error bound follows from the arithmetic it does (u = 2^-24; u_T = the storage
type's unit roundoff; SUB_T = half the spacing of the storage type's subnormals, an absolute term):

  statistics   the kernel's mean_rstd against stats() in float64.  A thread adds at most L <= 64 fp32 terms before the
               sums continue in double (asserted per case from reduce_blocks restated below), so a sum of terms t is
               within 63 u sum|t| < 2^-18 sum|t|; 2^-17 where the terms are rounded products.
                 mean            2^-18 E|y| + u |mean|
                 rstd, relative  dvar / (2 (var + eps)) + 2u,   dvar = 2^-17 E[y^2] + 2 |mean| dmean
  forward      z against forward() in float64 on the kernel's OWN float32 mean_rstd:
                 u_T |ref| + 8u ((|y| + |mean|) |rstd gamma| + |beta|) + SUB_T
  backward     mean_rstd is an input: float64 statistics cast to float32, given to kernel and reference alike.
                 dbeta, dgamma   2^-17 sum_{b,v} |da|,  2^-17 sum_{b,v} |da xhat|,  plus u |result|
                 dy              u_T |ref| + |gamma rstd| (8u (|da| + |c1| + |xhat c2|) + dc1 + |xhat| dc2) + SUB_T,
                                 dc1 = 2^-17 E|da|, dc2 = 2^-17 E|da xhat|     (c1 = S0 / V, c2 = S1 / V)
               With the sums taken in double (per-tile partials in), dc1 = 2u (|c1| + E|da|), dc2 likewise.

SUB_T is the one term added to the first derivation: a 16-bit float result below the type's normal range is rounded to
a multiple of the subnormal spacing (fp16: 2^-24), an absolute error of up to half of it that u_T |ref| does not cover.

LeakyReLU kink: fp32 and fp64 can decide a > 0 differently when a ~ 0, and one flipped decision moves every sum.  No
element is excluded from a comparison; instead gz is set to 0 wherever the float64 |a| < 1e-4 (|xhat gamma| + |beta| + 1)
(the kernel's a is within a few u of that scale), so that the decision cannot matter; under 1 % of the elements.

Every output buffer is pre-filled with NaN, padding columns of outputs with a sentinel that must survive, padding
columns of inputs and the workspace with NaN.  Each comparison prints its largest error / bound ratio.

Measured on an MI355X (no bound widened): 16-bit z and dy reach 0.98-1.00 of their bound - the storage rounding itself goes
up to half an ulp = u_T |ref| - and fp32 z / dy 0.28 / 0.34; mean, rstd, dgamma, dbeta from the kernels' own reductions stay
under 0.02 (the rounding errors of <= 64 terms do not line up), from double partial sums under 0.46."""
import ctypes
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import instnorm_ref as iref
from conftest import reload_kernel_switches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
U = 2.0 ** -24
U_T = {0: 0.0, 1: 2.0 ** -8, 2: 2.0 ** -11}
SUB_T = {0: 0.0, 1: 0.0, 2: 2.0 ** -25}
SLOPE = ctypes.c_float(0.01).value            # the values the kernels receive (float arguments of the C ABI)
EPS = ctypes.c_float(1e-5).value
SENTINEL = -77.0                              # exact in every storage type
OK, BADARG, WORKSPACE = 0, -1, -3


def _cdiv(a, b):
    return -(-a // b)


def reduce_blocks(V, B):
    """conv_api.h restated: >= 32 rows per workgroup up to min(2048, max(128, 4096 / B)) workgroups per sample."""
    return max(1, min(_cdiv(V, 32), min(2048, max(128, 4096 // B))))


# ------------------------------------------------------------------------------------------------ inputs and reference
@functools.lru_cache(maxsize=None)
def _inputs(B, C, V, dt, kind="normal"):
    """Draws of one case on the CPU (float32, rounded to the storage type, read back as float64) with every float64
    reference quantity and bound of the module docstring.  Computed once per case and shared; nothing modifies it."""
    g = torch.Generator().manual_seed(1000003 * B + 1009 * C + 17 * V + dt)
    std = torch.rand(C, generator=g) * 1.5 + 0.5
    if kind == "offset":                       # every channel's mean at 100 x its standard deviation
        y32 = (torch.randn(B, V, C, generator=g) + 100.0) * std
    else:
        y32 = torch.randn(B, V, C, generator=g) * std + torch.randn(C, generator=g)
    if kind == "constant":
        y32[:, :, 2] = 3.3
        y32[:, :, 5] = 0.0
    gz32 = torch.randn(B, V, C, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    y_t = y32.to(TDT[dt])
    y64, g64, b64 = y_t.double(), gamma.double(), beta.double()

    mean, rstd = iref.stats(y64, EPS)
    var_eps = 1.0 / rstd ** 2
    e_abs, e_sq = y64.abs().mean(dim=1), (y64 * y64).mean(dim=1)
    b_mean = 2.0 ** -18 * e_abs + U * mean.abs()
    b_rstd_rel = (2.0 ** -17 * e_sq + 2 * mean.abs() * b_mean) / (2 * var_eps) + 2 * U

    mr32 = torch.stack([mean, rstd], dim=-1).float()                     # the backward's input
    m32, r32 = mr32[..., 0].double(), mr32[..., 1].double()
    xhat, a = iref.pre_activation(y64, m32, r32, g64, b64)
    near = a.abs() < 1e-4 * ((xhat * g64).abs() + b64.abs() + 1.0)
    assert float(near.float().mean()) < 0.01, f"kink guard touches {float(near.float().mean()):.2%} of the elements"
    gz32[near] = 0.0
    gz_t = gz32.to(TDT[dt])
    gz64 = gz_t.double()
    dy, dgamma, dbeta, S0, S1 = iref.backward(gz64, y64, m32, r32, g64, b64, SLOPE)
    da = torch.where(a > 0, gz64, SLOPE * gz64)
    c1, c2 = S0 / V, S1 / V
    e_da, e_dax = da.abs().mean(dim=1), (da * xhat).abs().mean(dim=1)

    def bwd_bounds(dc1, dc2):
        gr = (g64 * r32).abs()[:, None, :]
        b_dy = U_T[dt] * dy.abs() + SUB_T[dt] + gr * (
            8 * U * (da.abs() + c1.abs()[:, None, :] + (xhat * c2[:, None, :]).abs()) + dc1[:, None, :] + xhat.abs() * dc2[:, None, :])
        return SimpleNamespace(dy=b_dy, dbeta=V * dc1.sum(dim=0) + U * dbeta.abs(), dgamma=V * dc2.sum(dim=0) + U * dgamma.abs())

    return SimpleNamespace(
        B=B, C=C, V=V, dt=dt, y_t=y_t, gz_t=gz_t, y64=y64, gz64=gz64, gamma=gamma, beta=beta, g64=g64, b64=b64,
        mean=mean, rstd=rstd, b_mean=b_mean, b_rstd_rel=b_rstd_rel, e_abs=e_abs, mr32=mr32, xhat=xhat, da=da,
        dy=dy, dgamma=dgamma, dbeta=dbeta,
        bwd=bwd_bounds(2.0 ** -17 * e_da, 2.0 ** -17 * e_dax),                                  # fp32 partial sums
        bwd_double=bwd_bounds(2 * U * (c1.abs() + e_da), 2 * U * (c2.abs() + e_dax)))          # sums taken in double


def _z_bound(inp, ref, mean_k, rstd_k):
    return (U_T[inp.dt] * ref.abs() + SUB_T[inp.dt] +
            8 * U * ((inp.y64.abs() + mean_k.abs()[:, None, :]) * (rstd_k * inp.g64).abs()[:, None, :] + inp.b64.abs()))


def _ratio(err, bound):
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(torch.nan_to_num(r, nan=math.inf).max())


def _within(what, got, ref, bound, factor=1.0):
    """Asserts |got - ref| <= factor * bound element by element (NaN fails) and prints the largest error / bound."""
    err = (got - ref).abs()
    ratio = _ratio(err, bound * factor)
    print(f"RATIO {what}: max err/bound {ratio:.3f} (max abs err {float(torch.nan_to_num(err, nan=math.inf).max()):.3e})")
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f}"
    return ratio


# ------------------------------------------------------------------------------------------------ device buffers
class Rows:
    """B*V rows of leading dimension ld in the storage type; the operand is columns col0 .. col0+C-1 and starts `lead`
    elements into the allocation.  Everything that is not operand holds `pad`."""

    def __init__(self, inp, ld, col0, pad, values=None, lead=0):
        self.B, self.V, self.C, self.ld, self.col0 = inp.B, inp.V, inp.C, ld, col0
        n = self.B * self.V * ld
        self.flat = torch.full((lead + n + 8,), pad, dtype=TDT[inp.dt], device=DEV)
        self.rows = self.flat[lead:lead + n].view(self.B * self.V, ld)
        self.pad, self.lead, self.n = pad, lead, n
        fill = torch.full((self.B * self.V, self.C), math.nan, dtype=TDT[inp.dt]) if values is None else values.reshape(-1, self.C)
        self.rows[:, col0:col0 + self.C] = fill.to(DEV)
        self.ptr = self.rows.data_ptr() + col0 * self.flat.element_size()

    def get(self):
        """The operand as stored, [B,V,C] on the CPU."""
        return self.rows[:, self.col0:self.col0 + self.C].contiguous().cpu().reshape(self.B, self.V, self.C)

    def assert_padding_untouched(self, what):
        t = self.flat.clone()
        t[self.lead:self.lead + self.n].view(-1, self.ld)[:, self.col0:self.col0 + self.C] = self.pad
        assert bool((t == self.pad).all()), f"{what}: an element outside the operand was written"


def _layout(C, ld_extra):
    """ld, col0.  ld_extra == C is the concat buffer: rows of 2C elements whose SECOND half is the operand."""
    return C + ld_extra, (C if ld_extra == C else 0)


def _lib():
    from dg_tta_amd import _lib as L
    return L.load()


def _ws(B, C, V):
    n = _lib().dgtta_instnorm_ws_bytes(B, C, V)
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV), n            # all-ones: NaN as double and as float


def _forward(inp, ld_extra=0, y_lead=0, out_lead=0, stats=None, with_z=True):
    """-> (mean_rstd [B,C,2] float32 on the CPU, z [B,V,C] as stored or None)."""
    from dg_tta_amd._lib import check, ptr, stream_of
    ld, col0 = _layout(inp.C, ld_extra)
    y = Rows(inp, ld, col0, math.nan, inp.y_t, lead=y_lead)
    z = Rows(inp, ld, col0, SENTINEL, lead=out_lead) if with_z else None
    gamma, beta = inp.gamma.to(DEV), inp.beta.to(DEV)
    mr = torch.full((inp.B, inp.C, 2), math.nan, device=DEV)
    ws, nws = _ws(inp.B, inp.C, inp.V)
    stats_d = None if stats is None else stats.to(DEV)
    check(_lib().dgtta_instnorm_lrelu_fwd(y.ptr, ld, ptr(stats_d), ptr(gamma), ptr(beta), ptr(mr), z.ptr if z else None,
                                          ld if z else 0, ptr(ws), nws, inp.B, inp.C, inp.V, EPS, SLOPE, inp.dt, stream_of()),
          "instnorm_lrelu_fwd")
    torch.cuda.synchronize()
    assert torch.equal(y.get().view(torch.uint8), inp.y_t.view(torch.uint8)), "the forward modified y"
    if stats is not None:
        assert torch.equal(stats_d.cpu().view(torch.int64), stats.view(torch.int64)), "the forward modified the statistics"
    if z is None:
        return mr.cpu(), None
    z.assert_padding_untouched("z")
    return mr.cpu(), z.get()


class Backward:
    """Buffers of one backward problem; run() may be called again on the same buffers (accumulate = 1)."""

    def __init__(self, inp, ld_extra=0, y_lead=0, out_lead=0):
        ld, col0 = _layout(inp.C, ld_extra)
        self.inp, self.ld = inp, ld
        self.y = Rows(inp, ld, col0, math.nan, inp.y_t, lead=y_lead)
        self.gz = Rows(inp, ld, col0, math.nan, inp.gz_t)
        self.dy = Rows(inp, ld, col0, SENTINEL, lead=out_lead)
        self.gamma, self.beta, self.mr = inp.gamma.to(DEV), inp.beta.to(DEV), inp.mr32.to(DEV)
        self.dgamma = torch.full((inp.C,), math.nan, device=DEV)
        self.dbeta = torch.full((inp.C,), math.nan, device=DEV)

    def run(self, accumulate=0, gstats=None):
        """-> (dy [B,V,C] as stored, dgamma, dbeta) on the CPU."""
        from dg_tta_amd._lib import check, ptr, stream_of
        inp, ld, lib = self.inp, self.ld, _lib()
        ws, nws = _ws(inp.B, inp.C, inp.V)
        head = (self.gz.ptr, ld, self.y.ptr, ld, ptr(self.gamma), ptr(self.beta), ptr(self.mr), self.dy.ptr, ld,
                ptr(self.dgamma), ptr(self.dbeta))
        tail = (ptr(ws), nws, inp.B, inp.C, inp.V, SLOPE, accumulate, inp.dt, stream_of())
        if gstats is None:
            check(lib.dgtta_instnorm_lrelu_bwd(*head, *tail), "instnorm_lrelu_bwd")
        else:
            gstats_d = gstats.to(DEV)
            check(lib.dgtta_instnorm_lrelu_bwd_gstats(*head, ptr(gstats_d), *tail), "instnorm_lrelu_bwd_gstats")
        torch.cuda.synchronize()
        self.dy.assert_padding_untouched("dy")
        assert torch.equal(self.y.get().view(torch.uint8), inp.y_t.view(torch.uint8)), "the backward modified y"
        assert torch.equal(self.gz.get().view(torch.uint8), inp.gz_t.view(torch.uint8)), "the backward modified gz"
        assert torch.equal(self.mr.cpu(), inp.mr32), "the backward modified mean_rstd"
        return self.dy.get(), self.dgamma.cpu(), self.dbeta.cpu()


def _check_stats(tag, inp, mr):
    mean_k, rstd_k = mr[..., 0].double(), mr[..., 1].double()
    r1 = _within(f"{tag} mean", mean_k, inp.mean, inp.b_mean)
    r2 = _within(f"{tag} rstd", rstd_k / inp.rstd, torch.ones_like(inp.rstd), inp.b_rstd_rel)
    return mean_k, rstd_k, max(r1, r2)


def _check_forward(tag, inp, mr, z):
    mean_k, rstd_k, _ = _check_stats(tag, inp, mr)
    ref = iref.forward(inp.y64, mean_k, rstd_k, inp.g64, inp.b64, SLOPE)         # on the kernel's own statistics
    _within(f"{tag} z", z.double(), ref, _z_bound(inp, ref, mean_k, rstd_k))


def _check_backward(tag, inp, out, bounds, factor=1.0):
    dy, dgamma, dbeta = out
    _within(f"{tag} dbeta", dbeta.double(), factor * inp.dbeta, bounds.dbeta, factor)
    _within(f"{tag} dgamma", dgamma.double(), factor * inp.dgamma, bounds.dgamma, factor)
    _within(f"{tag} dy", dy.double(), inp.dy, bounds.dy)


# ------------------------------------------------------------------------------------------------ a. every branch
CASES = [  # (B, C, V, dt, ld_extra)
    # scalar reduction + scalar apply (C no multiple of 16 bytes, or rows that are not); C > 64: a second c0 pass
    (1, 1, 257, 0, 0), (2, 5, 1000, 0, 3), (2, 12, 333, 1, 0), (1, 70, 129, 2, 2),
    # 16-byte reduction + fast apply (256 % G == 0); G = 1: rpi = 256; the last: the second half of a 2C concat buffer
    (2, 16, 1000, 0, 0), (1, 8, 777, 2, 0), (3, 32, 2049, 1, 0), (1, 64, 515, 1, 64),
    # very wide rows: G = 64, and G = 256 with rpi = 1
    (1, 512, 130, 1, 0), (1, 2048, 67, 1, 0),
    # 16-byte reduction + slow apply: G = 40 (16 of 256 threads idle in the reduction), G = 3, G = 24
    (2, 320, 300, 1, 0), (1, 24, 1001, 2, 8), (1, 96, 511, 0, 0),
    # block-count caps: 2048 blocks (finalize loops over > 256 partials); the 128-block floor with B * nblk partial rows
    (1, 8, 70001, 1, 0), (40, 8, 5000, 2, 0),
    # the 16-byte reduction deals rows to the workgroups 2 rpi at a time: with G = 1 (512 rows) only the first 137 of those
    # 2048 partials hold a row, and a finalize loop that counted partial 255 twice passed.  Partials past 256 that are not
    # zero: 16-byte reduction with G = 4 (128 rows at a time: workgroups < 547), scalar reduction (35 rows each: all 2048)
    (1, 32, 70001, 1, 0), (1, 5, 70001, 0, 0),
    # tiny V
    (2, 32, 1, 1, 0), (2, 32, 2, 0, 0), (1, 32, 31, 2, 0), (1, 5, 1, 0, 0),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B{}-C{}-V{}-dt{}-ld+{}".format(*c))
def test_forward_and_backward_vs_float64(case):
    B, C, V, dt, ld_extra = case
    # L <= 64: a workgroup of the scalar reduction owns cdiv(V, nblk) rows, dealt to >= 4 row groups; the 16-byte
    # reduction deals rows to the workgroups 2 rpi at a time, a thread takes two of them per round of nblk * 2 rpi rows
    assert _cdiv(V, reduce_blocks(V, B)) <= 64
    inp = _inputs(B, C, V, dt)
    tag = "a " + "-".join(map(str, case))

    mr, z = _forward(inp, ld_extra)
    _check_forward(tag, inp, mr, z)
    if V == 1:          # var = 0: rstd = 1 / sqrt(eps), xhat = 0, z = lrelu(beta); S0 = da, so dy = 0 exactly
        # (fp32 storage: sum y^2 - mean^2 alone leaves the fp32 rounding of y^2, 1.3 % of rstd here before the
        # finalize step took the variance of a single voxel as 0)
        rstd0 = float(torch.tensor(1.0 / math.sqrt(EPS), dtype=torch.float32))
        assert float((mr[..., 1].double() / rstd0 - 1).abs().max()) <= 2 * U
        zb = torch.where(inp.b64 > 0, inp.b64, SLOPE * inp.b64).expand(B, V, C)
        _within(f"{tag} z vs lrelu(beta)", z.double(), zb, _z_bound(inp, zb, mr[..., 0].double(), mr[..., 1].double()))
    if V == 2:
        assert bool(torch.isfinite(mr).all()) and bool(torch.isfinite(z.float()).all())

    bw = Backward(inp, ld_extra)
    out0 = bw.run(accumulate=0)
    _check_backward(tag, inp, out0, inp.bwd)
    if V == 1:
        assert bool((out0[0].double()[inp.dy == 0] == 0).all()), "dy != 0 where the reference's is exactly 0"
    if V == 2:
        assert all(bool(torch.isfinite(t.float()).all()) for t in out0)
    # accumulate = 1 on the same buffers: dgamma = fl(d + fl(S)) with d = fl(S): twice the summation error, which the
    # bound's 2^-17 holds with room (63 u of summation, 4 u of products), plus 4 u |S| of the three roundings
    out1 = bw.run(accumulate=1)
    _check_backward(f"{tag} accumulate", inp, out1, inp.bwd, factor=2.0)
    assert torch.equal(out1[0].view(torch.uint8), out0[0].view(torch.uint8)), "dy changed with accumulate = 1"


# ------------------------------------------------------------------------------------------------ b. misaligned rows
def test_misaligned_rows_take_the_scalar_kernels():
    """Base pointers 8 bytes into an allocation: y misaligned sends reduction and apply to the scalar kernels, z / dy
    misaligned the apply alone.  Same bounds as the aligned run, and the same results up to one rounding of the
    storage type: the fp32 value in front of that rounding differs by the order of the sums (both inside their bounds)."""
    inp = _inputs(2, 32, 515, 1)
    dt = inp.dt
    mr_a, z_a = _forward(inp)
    _check_forward("b aligned", inp, mr_a, z_a)
    bw_a = Backward(inp)
    out_a = bw_a.run()
    _check_backward("b aligned", inp, out_a, inp.bwd)
    assert bw_a.y.ptr % 16 == 0 and bw_a.dy.ptr % 16 == 0
    for name, y_lead, out_lead in (("y", 4, 0), ("outputs", 0, 4)):
        tag = f"b misaligned {name}"
        mr, z = _forward(inp, y_lead=y_lead, out_lead=out_lead)
        _check_forward(tag, inp, mr, z)
        bw = Backward(inp, y_lead=y_lead, out_lead=out_lead)
        assert bw.y.ptr % 16 == (8 if y_lead else 0) and bw.dy.ptr % 16 == (8 if out_lead else 0)
        out = bw.run()
        _check_backward(tag, inp, out, inp.bwd)
        # z: one storage rounding (an ulp is at most 2 u_T of the larger value), twice the fp32 part of the z bound, and
        # what the difference of the two runs' statistics moves: |gamma| (rstd |dmean| + |y - mean| |drstd|)
        m_a, r_a, m, r = (t.double() for t in (mr_a[..., 0], mr_a[..., 1], mr[..., 0], mr[..., 1]))
        za, zm = z_a.double(), z.double()
        fp32_part = _z_bound(inp, za, m_a, r_a) - U_T[dt] * za.abs()
        moved = inp.g64.abs() * (r_a * (m - m_a).abs())[:, None, :] + \
            inp.g64.abs() * (inp.y64 - m_a[:, None, :]).abs() * (r - r_a).abs()[:, None, :]
        _within(f"{tag} z vs aligned", zm, za, 2 * U_T[dt] * torch.maximum(za.abs(), zm.abs()) + 2 * fp32_part + moved)
        # backward: mean_rstd is the same input; the sums differ within both runs' bounds
        da_, dm = out_a[0].double(), out[0].double()
        fp32_part = inp.bwd.dy - U_T[dt] * inp.dy.abs()
        _within(f"{tag} dy vs aligned", dm, da_, 2 * U_T[dt] * torch.maximum(da_.abs(), dm.abs()) + 2 * fp32_part)
        _within(f"{tag} dgamma vs aligned", out[1].double(), out_a[1].double(), 2 * inp.bwd.dgamma)
        _within(f"{tag} dbeta vs aligned", out[2].double(), out_a[2].double(), 2 * inp.bwd.dbeta)


# ------------------------------------------------------------------------------------------------ c. streaming switch
@pytest.mark.parametrize("case", [(3, 32, 2049, 1, 0), (1, 64, 515, 2, 64)], ids=lambda c: "B{}-C{}-V{}-dt{}-ld+{}".format(*c))
def test_streaming_switch_is_bit_identical(case, monkeypatch):
    """DGTTA_IN_NT=0 (plain loads / stores in the fast apply path) against the default (non-temporal)."""
    B, C, V, dt, ld_extra = case
    inp = _inputs(B, C, V, dt)

    def run():
        reload_kernel_switches()
        mr, z = _forward(inp, ld_extra)
        dy, dgamma, dbeta = Backward(inp, ld_extra).run()
        return mr, z, dy, dgamma, dbeta

    monkeypatch.setenv("DGTTA_IN_NT", "0")
    plain = run()
    monkeypatch.delenv("DGTTA_IN_NT")
    streaming = run()
    _check_forward("c streaming", inp, streaming[0], streaming[1])
    _check_backward("c streaming", inp, streaming[2:], inp.bwd)
    for name, p, s in zip(("mean_rstd", "z", "dy", "dgamma", "dbeta"), plain, streaming):
        assert not bool(torch.isnan(s.float()).any()), name
        assert torch.equal(p, s), f"{name} differs between DGTTA_IN_NT=0 and the default"


# ------------------------------------------------------------------------------------------------ d. statistics from partials
def _check_stats_double(tag, inp, mr):
    """All arithmetic of the finalize step is double: 2u relative (mean: of max(|mean|, E|y|))."""
    mean_k, rstd_k = mr[..., 0].double(), mr[..., 1].double()
    _within(f"{tag} mean", mean_k, inp.mean, 2 * U * torch.maximum(inp.mean.abs(), inp.e_abs))
    _within(f"{tag} rstd", rstd_k / inp.rstd, torch.ones_like(inp.rstd), torch.full_like(inp.rstd, 2 * U))


@pytest.mark.parametrize("case", [(2, 32, 3000, 1, "normal"), (1, 5, 3000, 0, "normal"), (1, 5, 3000, 0, "offset")],
                         ids=lambda c: "B{}-C{}-V{}-dt{}-{}".format(*c))
def test_forward_from_epilogue_partials(case):
    """in_stats_finalize_kernel fed by a header: per-tile (sum y, sum y^2) in float64 for ragged partitions, some tiles
    empty, tile counts around the finalize loop's 256.  With the mean at 100 x the standard deviation the same 2u holds:
    the finalize step is not where offset data loses accuracy."""
    B, C, V, dt, kind = case
    inp = _inputs(B, C, V, dt, kind)
    for nblk in (1, 7, 255, 256, 257, 1000):
        buf = iref.partials(inp.y64, inp.y64 * inp.y64, iref.ragged_cuts(V, nblk, seed=nblk))
        mr, z = _forward(inp, stats=buf)
        tag = f"d {B}-{C}-{V}-{dt}-{kind} nblk={nblk}"
        _check_stats_double(tag, inp, mr)
        mean_k, rstd_k = mr[..., 0].double(), mr[..., 1].double()
        ref = iref.forward(inp.y64, mean_k, rstd_k, inp.g64, inp.b64, SLOPE)
        _within(f"{tag} z", z.double(), ref, _z_bound(inp, ref, mean_k, rstd_k))


# ------------------------------------------------------------------------------------------------ e. own reduction, offset mean
def test_own_reduction_with_offset_mean():
    """The kernel's own one-pass reduction (sum y, sum y^2 in fp32 per thread, then double) on data whose mean is 100 x
    its standard deviation: only the derived statistics bound is asserted (loose here: E[y^2] = 10^4 var makes it
    about 8 % of rstd); the measured relative rstd error is printed.  Measured on an MI355X: 1.7e-5 of rstd at the worst
    channel against a bound of 8.0e-2 - the rounding errors of a thread's <= 64 terms do not line up as the bound allows."""
    inp = _inputs(1, 16, 4096, 0, "offset")
    assert _cdiv(inp.V, reduce_blocks(inp.V, inp.B)) <= 64
    assert float((inp.mean.abs() * inp.rstd).min()) > 95.0                  # (the sample's own mean / std)
    mr, z = _forward(inp)
    _check_forward("e offset", inp, mr, z)
    rel = (mr[..., 1].double() / inp.rstd - 1).abs()
    print(f"MEASURED e offset-mean relative rstd error: max {float(rel.max()):.3e}, bound {float(inp.b_rstd_rel.max()):.3e}")


# ------------------------------------------------------------------------------------------------ f. constant channels
def test_constant_channel():
    """Two channels constant (3.3 and 0): var = 0, rstd = 1 / sqrt(eps) at most, so an error dmean of the mean is worth
    |gamma| dmean / sqrt(eps) in z on top of the z bound of lrelu(beta).  Everything is finite."""
    inp = _inputs(1, 8, 500, 0, "constant")
    mr, z = _forward(inp)
    assert bool(torch.isfinite(mr).all()) and bool(torch.isfinite(z).all())
    _check_forward("f constant", inp, mr, z)
    rs0 = 1.0 / math.sqrt(EPS)
    for c in (2, 5):
        assert float(inp.rstd[0, c]) == pytest.approx(rs0, rel=1e-12)
        b = inp.b64[c]
        zb = torch.where(b > 0, b, SLOPE * b).expand(inp.V)
        yc = inp.y64[0, :, c].abs()
        bound = inp.g64[c].abs() * inp.b_mean[0, c] * rs0 + 8 * U * ((yc + inp.mean[0, c].abs()) * rs0 * inp.g64[c].abs() + b.abs())
        _within(f"f constant channel {c} z vs lrelu(beta)", z[0, :, c].double(), zb, bound)
    dy, dgamma, dbeta = Backward(inp).run()
    assert all(bool(torch.isfinite(t).all()) for t in (dy, dgamma, dbeta))
    _check_backward("f constant", inp, (dy, dgamma, dbeta), inp.bwd)


# ------------------------------------------------------------------------------------------------ g. backward from gstats
@pytest.mark.parametrize("case", [(2, 32, 3000, 1, 0, "normal"), (1, 320, 300, 2, 0, "normal"), (2, 5, 1000, 0, 3, "normal"),
                                  (2, 5, 1000, 0, 3, "offset")], ids=lambda c: "B{}-C{}-V{}-dt{}-ld+{}-{}".format(*c))
def test_backward_from_gstats_partials(case):
    """in_bwd_finalize_kernel given mean_rstd: per-tile (sum g', sum g' y) in float64 (what the data-gradient kernel leaves) turned
    into c1, c2, dgamma, dbeta as rs (s1 - mu s0) in double - also where the mean is 100 x the standard deviation - and
    the apply pass on them, against the reference with the bounds of double sums and against dgtta_instnorm_lrelu_bwd
    on the same inputs within the sum of both paths' bounds."""
    B, C, V, dt, ld_extra, kind = case
    inp = _inputs(B, C, V, dt, kind)
    tag = "g " + "-".join(map(str, case))
    own = Backward(inp, ld_extra).run()
    _check_backward(f"{tag} reduction pass", inp, own, inp.bwd)
    for nblk in (1, 7, 256, 257, 600):
        buf = iref.partials(inp.da, inp.da * inp.y64, iref.ragged_cuts(V, nblk, seed=100 + nblk))
        out = Backward(inp, ld_extra).run(gstats=buf)
        _check_backward(f"{tag} nblk={nblk}", inp, out, inp.bwd_double)
        _within(f"{tag} nblk={nblk} dy vs reduction pass", out[0].double(), own[0].double(), inp.bwd.dy + inp.bwd_double.dy)
        _within(f"{tag} nblk={nblk} dgamma vs reduction pass", out[1].double(), own[1].double(), inp.bwd.dgamma + inp.bwd_double.dgamma)
        _within(f"{tag} nblk={nblk} dbeta vs reduction pass", out[2].double(), own[2].double(), inp.bwd.dbeta + inp.bwd_double.dbeta)
    out1 = Backward(inp, ld_extra)
    first = out1.run(gstats=buf)
    second = out1.run(accumulate=1, gstats=buf)
    _check_backward(f"{tag} accumulate", inp, second, inp.bwd_double, factor=2.0)
    assert torch.equal(first[0].view(torch.uint8), second[0].view(torch.uint8))


# ------------------------------------------------------------------------------------------------ h. argument checks
def test_argument_checks():
    """Rejected calls launch nothing: the outputs keep their NaN fill."""
    from dg_tta_amd._lib import ptr, stream_of
    lib = _lib()
    inp = _inputs(2, 5, 1000, 0)
    B, C, V, dt = inp.B, inp.C, inp.V, inp.dt
    assert lib.dgtta_instnorm_ws_bytes(0, C, V) == 0 and lib.dgtta_instnorm_ws_bytes(B, 0, V) == 0
    assert lib.dgtta_instnorm_ws_bytes(B, C, 0) == 0 and lib.dgtta_instnorm_ws_bytes(-1, C, V) == 0
    nblk = reduce_blocks(V, B)
    assert lib.dgtta_instnorm_ws_bytes(B, C, V) == _cdiv(B * nblk * C * 16, 256) * 256 + _cdiv(B * C * 8, 256) * 256

    y = Rows(inp, C, 0, math.nan, inp.y_t)
    gz = Rows(inp, C, 0, math.nan, inp.gz_t)
    z, dy = Rows(inp, C, 0, SENTINEL), Rows(inp, C, 0, SENTINEL)
    gamma, beta, mr_in = inp.gamma.to(DEV), inp.beta.to(DEV), inp.mr32.to(DEV)
    mr = torch.full((B, C, 2), math.nan, device=DEV)
    dgamma, dbeta = torch.full((C,), math.nan, device=DEV), torch.full((C,), math.nan, device=DEV)
    ws, nws = _ws(B, C, V)
    gstats = iref.partials(inp.da, inp.da * inp.y64, [0, V]).to(DEV)
    st = stream_of()

    def fwd(yp=y.ptr, ldy=C, b=B, c=C, v=V, n=nws):
        return lib.dgtta_instnorm_lrelu_fwd(yp, ldy, None, ptr(gamma), ptr(beta), ptr(mr), z.ptr, C, ptr(ws), n, b, c, v, EPS, SLOPE,
                                            dt, st)

    def bwd(fn, extra, yp=y.ptr, ldy=C, b=B, c=C, v=V, n=nws):
        return fn(gz.ptr, C, yp, ldy, ptr(gamma), ptr(beta), ptr(mr_in), dy.ptr, C, ptr(dgamma), ptr(dbeta), *extra, ptr(ws), n,
                  b, c, v, SLOPE, 0, dt, st)

    entries = [fwd, functools.partial(bwd, lib.dgtta_instnorm_lrelu_bwd, ()),
               functools.partial(bwd, lib.dgtta_instnorm_lrelu_bwd_gstats, (ptr(gstats),))]
    for call in entries:
        assert call(yp=None) == BADARG
        assert call(ldy=C - 1) == BADARG
        assert call(b=0) == BADARG and call(c=0) == BADARG and call(v=0) == BADARG and call(b=-1) == BADARG
        assert call(n=nws - 1) == WORKSPACE
    assert bwd(lib.dgtta_instnorm_lrelu_bwd_gstats, (None,)) == BADARG
    assert lib.dgtta_last_error()
    torch.cuda.synchronize()
    for t in (mr, dgamma, dbeta, z.get(), dy.get()):
        assert bool(torch.isnan(t).all()), "a rejected call wrote an output"

    # z = NULL with valid statistics: OK, mean_rstd filled, nothing else written
    stats = iref.partials(inp.y64, inp.y64 * inp.y64, iref.ragged_cuts(V, 7, seed=7))
    mr_full, _ = _forward(inp, stats=stats)
    mr_only, none = _forward(inp, stats=stats, with_z=False)           # (checks y and the statistics buffer afterwards)
    assert none is None and not bool(torch.isnan(mr_only).any()) and torch.equal(mr_only, mr_full)
    mr_own, _ = _forward(inp, with_z=False)
    _check_stats("h z=NULL", inp, mr_own)
