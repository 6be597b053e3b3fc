"""GPU: the GIN kernels of gin.hip, called through the C ABI with a workspace the test owns, against the float64 restatement
tests/gin_ref.py (licensed by tests/test_gin_ref.py).  The workspace layout is restated here: per-tile double partial sums
[B][tiles][2], the float norms [B][2] at align_up(., 256), the weight table after them.  Workspace and output are pre-filled
with NaN.  Kernels and shifts live in one NaN-filled arena, each followed by NaN, so that a read past a tensor's end (a k = 1
layer read as 27 taps, a sample index one too far) turns the output into NaN.  No element is excluded from any comparison;
each comparison prints its largest error / bound ratio; u = 2^-24.

3a  Exact chain.  Non-negative integer x, sparse 0/1 kernels, shifts in {1, 2}, alpha in {1, 0.5, 0}: the LeakyReLU is the
    identity and every layer and the blend are exact in float32 (licensed on the CPU: float32 == float64 bit for bit).  Only
    the norm pass and the final scale round.  `mixed` is recovered from out with the FLOAT64 norms and compared with the
    float64 mixed under the relative bound gin_ref.REL_RECOVER = 28 u: each norm 12 u (20 roundings per term of a sum of
    squares, halved by the root, + 1 for sqrtf; counted in gin_ref's docstring), the scale 4 u (1e-5 addition, reciprocal, two
    products).  max |mixed| of every case is at most 1 / (16 x 28 u) = 37449 (asserted), so an error of one unit in any
    intermediate is at least 16 x the tolerance.  All 16 kernel-size combinations at extents below the 4-voxel halo, one
    exact tile and a ragged shape; and the persistent loop: a shape with more than 2 x CU-count tiles, no multiple of the CU
    count (both asserted from torch.cuda.get_device_properties), different kernels per sample.
3b  Real operands.  randn x, kernels and shifts, alpha in (0, 1), 1 and 0.  Two limits, both against float64: the worst-case
    forward ceiling of gin_ref.chain (rigorous, loose), and: the kernel's largest error may not exceed ORACLE_FACTOR = 4 x the
    largest error of the float32 oracle.gin.gin_chain in the same case (same float32 formula, other summation order; 4 is
    the margin of a 54-term FMA chain against the CPU's blocked sums).  Norm preservation: |out_b| / |x_b| - 1 is
    -1e-5 / (|mixed_b| + 1e-5) within REL_RECOVER.  An all-zero sample next to a normal one gives a finite output.

Measured on an MI355X (no bound was widened to fit; largest error / bound per comparison): 3a the recovered mixed 0.13 of its
28 u (persistent-loop shapes 0.11), the kernel's norms 0.09 of their 12 u; 3b out 0.10 of the forward ceiling, the kernel's
largest error between 0.68 and 1.22 x the float32 oracle's over the 17 cases (largest: ks = (1, 3, 1, 1); limit 4), norm
preservation 0.09, norms 0.09.
"""
import ctypes
import functools
import math

import pytest
import torch

import gin_ref as gref
from oracle import gin as ogin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
TD, TH, TW = 8, 8, 32
ORACLE_FACTOR = 4.0
EXACT_CAP = 1.0 / (16 * gref.REL_RECOVER)


def _cdiv(a, b):
    return -(-a // b)


def _align(n, a=256):
    return _cdiv(n, a) * a


def tiles_per_sample(shape):
    return _cdiv(shape[1], TD) * _cdiv(shape[2], TH) * _cdiv(shape[3], TW)


def run(x, alpha, ks, kers, shifts):
    """One call of dgtta_gin_chain_fwd -> (out [B,1,D,H,W], norms [B,2] = (|x|, |mixed|) as the kernel took them), on the CPU."""
    from dg_tta_amd import _lib as L
    lib = L.load()
    b, _, d, h, w = x.shape
    per = tiles_per_sample((b, d, h, w))
    nws = lib.dgtta_gin_ws_bytes(b, d, h, w)
    off_n = _align(b * per * 16)
    assert nws == off_n + _align(b * 8) + _align(b * 336 * 4), "the workspace layout restated in this test is not the library's"
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=DEV)
    parts = [t.reshape(-1) for t in list(kers) + list(shifts)]
    offs, n = [], 0
    for p in parts:
        offs.append(n)
        n += p.numel() + 27 * max(p.numel(), 8)          # NaN behind every tensor: a k = 1 kernel read as 27 taps lands there
    arena = torch.full((n,), math.nan)
    for o, p in zip(offs, parts):
        arena[o:o + p.numel()] = p
    arena = arena.to(DEV)
    ptrs = [arena.data_ptr() + 4 * o for o in offs]
    x_d, al_d = x.to(DEV).contiguous(), alpha.to(DEV).contiguous()
    out = torch.full_like(x_d, math.nan)
    L.check(lib.dgtta_gin_chain_fwd(L.ptr(x_d), L.ptr(al_d), (ctypes.c_int * 4)(*[int(k) for k in ks]), (ctypes.c_void_p * 4)(*ptrs[:4]),
                                    (ctypes.c_void_p * 4)(*ptrs[4:]), L.ptr(out), L.ptr(ws), nws, b, d, h, w, L.stream_of()),
            "dgtta_gin_chain_fwd")
    torch.cuda.synchronize()
    assert torch.equal(x_d.cpu(), x), "the chain modified x"
    norms = ws[off_n:off_n + b * 8].cpu().view(torch.float32).reshape(b, 2).clone()
    return out.cpu(), norms


def _where(idx, shape):
    b_, d, h, w = shape
    x, y, z, b = idx % w, (idx // w) % h, (idx // (w * h)) % d, idx // (w * h * d)
    per_w, per_h = _cdiv(w, TW), _cdiv(h, TH)
    tile = b * tiles_per_sample(shape) + ((z // TD) * per_h + y // TH) * per_w + x // TW
    return f"b={b} d={z} h={y} w={x} (tile {tile})"


def _ratio(what, got, ref, bound, shape):
    err = (got.double() - ref).abs()
    r = torch.nan_to_num(err / bound, nan=math.inf)
    worst = float(r.max())
    print(f"RATIO {what}: max err/bound {worst:.3f} (max abs err {float(torch.nan_to_num(err, nan=math.inf).max()):.3e})")
    assert worst <= 1.0, (f"{what}: error / bound = {worst:.3f}, {int((r > 1).sum())} of {r.numel()} elements out, first at "
                          f"{_where(int((r > 1).reshape(-1).nonzero()[0]), shape)}, worst at {_where(int(r.argmax()), shape)}")
    return worst


def _check_norms(what, norms, ref, extra_mix=None):
    """gin_norm_kernel's two norms against float64 (extra_mix: what the error of mixed itself may add to |mixed|)."""
    for j, (name, r64) in enumerate((("|x|", ref.n_in), ("|mixed|", ref.n_mix))):
        bound = gref.REL_NORM * r64 + (extra_mix if j == 1 and extra_mix is not None else 0.0)
        err = (norms[:, j].double() - r64).abs()
        ratio = max((e / b_ if b_ > 0 else (0.0 if e == 0 else math.inf)) if e == e else math.inf
                    for e, b_ in zip(err.tolist(), torch.as_tensor(bound).expand_as(err).tolist()))
        print(f"RATIO {what} {name}: max err/bound {ratio:.3f}")
        assert ratio <= 1.0, f"{what}: block sums / pass B (gin_norm_kernel) {name}: {norms[:, j].tolist()} vs float64 {r64.tolist()}"


# ------------------------------------------------------------------------------------------------ 3a
@functools.lru_cache(maxsize=None)
def _exact(ks, shape, seed=0):
    x, alpha, k, kers, shifts = gref.exact_inputs(ks, shape, seed)
    return x, alpha, k, kers, shifts, gref.chain(x, alpha, k, kers, shifts, ceiling=False)


def _check_exact(ks, shape, seed=0):
    x, alpha, k, kers, shifts, ref = _exact(ks, shape, seed)
    top = float(ref.mixed.abs().max())
    assert 0 < top <= EXACT_CAP, f"exact case ks={ks} {shape}: max |mixed| {top} above the cap {EXACT_CAP:.0f}"
    assert all(float(s.min()) >= 1 for s in shifts)
    out, norms = run(x, alpha, k, kers, shifts)
    what = f"exact chain ks={ks} {shape}"
    rec = gref.recover_mixed(out, ref.n_in, ref.n_mix)
    _ratio(f"pass A (gin_chain_kernel) {what}: mixed recovered from out", rec, ref.mixed, gref.REL_RECOVER * ref.mixed.abs() + 2.0 ** -126, shape)
    _check_norms(what, norms, ref)


@pytest.mark.parametrize("shape", gref.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ks", gref.ALL_KS, ids=lambda k: "".join(map(str, k)))
def test_exact_chain(ks, shape):
    _check_exact(ks, shape)


def persistent_shape():
    """(B, D, H, W) with more than 2 x CU-count tiles, no multiple of the CU count: B = 2, (57, 57, 129) = 640 tiles on a
    256-CU part; deeper on a larger one."""
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    d = 57
    while 2 * tiles_per_sample((2, d, 57, 129)) <= 2 * cus or (2 * tiles_per_sample((2, d, 57, 129))) % cus == 0:
        d += 8
    shape = (2, d, 57, 129)
    n = 2 * tiles_per_sample(shape)
    assert n > 2 * cus and n % cus != 0, f"{n} tiles on {cus} CUs: the persistent loop is not exercised"
    assert tiles_per_sample(shape) % cus != 0           # a workgroup's tiles change sample
    return shape


@pytest.mark.parametrize("ks", [(3, 3, 3, 3), (1, 1, 1, 1), (3, 1, 3, 1), (1, 3, 1, 3)], ids=lambda k: "".join(map(str, k)))
def test_exact_chain_persistent_loop(ks):
    """Every workgroup runs at least two tiles (the register prefetch of tile + gridDim) and moves on to the next sample,
    whose kernels differ."""
    shape = persistent_shape()
    x, alpha, k, kers, shifts, ref = _exact(ks, shape)
    assert float(alpha[1]) > 0 and any(not torch.equal(kr[:kr.shape[0] // 2], kr[kr.shape[0] // 2:]) for kr in kers)
    _check_exact(ks, shape)


# ------------------------------------------------------------------------------------------------ 3b
@functools.lru_cache(maxsize=None)
def _real(ks, shape, seed=0):
    x, alpha, k, kers, shifts = gref.real_inputs(ks, shape, seed)
    ref = gref.chain(x, alpha, k, kers, shifts)
    o32 = ogin.gin_chain(x, alpha, k, kers, shifts)
    return x, alpha, k, kers, shifts, ref, float((o32.double() - ref.out).abs().max())


def _check_real(ks, shape, seed=0):
    x, alpha, k, kers, shifts, ref, oracle_err = _real(ks, shape, seed)
    what = f"real operands ks={ks} {shape}"
    out, norms = run(x, alpha, k, kers, shifts)
    _check_norms(what, norms, ref, extra_mix=ref.ceil_mixed.reshape(shape[0], -1).norm(dim=1))
    _ratio(f"{what}: out against the forward ceiling", out, ref.out, ref.ceil_out + 2.0 ** -126, shape)
    err = float((out.double() - ref.out).abs().max())
    print(f"RATIO {what}: kernel max err {err:.3e} / float32 oracle max err {oracle_err:.3e} = {err / oracle_err:.3f} (limit {ORACLE_FACTOR:g})")
    assert err <= ORACLE_FACTOR * oracle_err, (f"{what}: kernel max err {err:.3e} is {err / oracle_err:.2f} x the float32 oracle's "
                                              f"{oracle_err:.3e} (both against float64)")
    for b in range(shape[0]):
        expect = -gref.EPS32 / (float(ref.n_mix[b]) + gref.EPS32)
        got = float(out[b].double().norm() / ref.n_in[b]) - 1.0
        print(f"RATIO {what} norm preservation b={b}: {abs(got - expect) / gref.REL_RECOVER:.3f}")
        assert abs(got - expect) <= gref.REL_RECOVER, f"{what}: |out_{b}| / |x_{b}| - 1 = {got:.3e}, float64 {expect:.3e}"


@pytest.mark.parametrize("ks", gref.ALL_KS, ids=lambda k: "".join(map(str, k)))
def test_real_operands(ks):
    shape = (3, 9, 11, 37)
    alpha = _real(ks, shape)[1]
    assert 0 < float(alpha[0]) < 1 and sorted(alpha[1:].tolist()) == [0.0, 1.0]
    _check_real(ks, shape)


def test_real_operands_persistent_loop():
    _check_real((3, 1, 3, 3), persistent_shape())


def test_all_zero_sample_next_to_a_normal_one():
    ks = (3, 1, 3, 3)
    x, alpha, k, kers, shifts = gref.real_inputs(ks, (2, 9, 11, 37), 2)
    x = x.clone()
    x[1] = 0.0
    alpha = torch.tensor([0.3, 0.6])
    ref = gref.chain(x, alpha, k, kers, shifts)
    out, norms = run(x, alpha, k, kers, shifts)
    assert bool(torch.isfinite(out).all()) and float(norms[1, 0]) == 0.0 and float(norms[1, 1]) > 0.0
    assert bool((out[1] == 0).all()), "|x| = 0 scales the sample to 0"
    _ratio("all-zero neighbour: out against the forward ceiling", out, ref.out, ref.ceil_out + 2.0 ** -126, (2, 9, 11, 37))
