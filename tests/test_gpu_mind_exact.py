"""GPU: the MIND kernels of mind3d.hip, called through the C ABI with a workspace the test owns, against the float64
restatement tests/mind_ref.py (licensed by tests/test_mind_ref.py), pass by pass.  The workspace layout is restated here:
m = ssd - min as float32 [B][V][12], the per-tile double partial sums at align_up(., 256), the float global mean at the next
align_up(., 256).  Workspace and outputs are pre-filled with NaN (also the out_ldc padding, which the kernel must overwrite
with 0).  No element is excluded from any comparison; each comparison prints its largest error / bound ratio; u = 2^-24.

2a  Pass A bit for bit (mind_ssd_kernel).  Dyadic taps, integer image and noise, rw = 1: every intermediate of the D, H and W
    filter passes has at most 23 significant bits (mind_ref.exact_inputs; float32 == float64 bit for bit is licensed on the
    CPU), so the workspace m must EQUAL the float64 m at every voxel and channel: every tap, halo clamp, noise index and tile
    index.  All six built kernels (delta, taps) at extents below the halo R + delta, one exact tile, ragged, 81 tiles (launch
    order) and 8 / 16 tiles (permuted launch order).  The 7-tap kernels walk the last 20 columns of their q tile (row 13,
    columns 18..37) in a second pass; those feed the outputs of tile row 7, columns 12..31, which exist when H >= 8 and
    W >= 33 (asserted).  The global mean: m is exact, so only the 31 roundings of mind_ref.REL_GM apply: relative 32 u.
2b  Seeded form: dgtta_mind3d_fwd_seeded writes the same workspace m and the same output, bit for bit, as dgtta_mind3d_fwd fed
    dgtta_mind3d_noise_fill (Gaussian taps, rw = 0.05, randn image).
2c  Finish pass alone (mind_finish_kernel): out against mind_ref.finish in float64 on the kernel's OWN m and global mean read
    back from the workspace; the bound is mind_ref.finish_bound (a 12-term sum, a divide, the clamp, a divide, expf, and the
    16-bit store).  The case clamps on both sides (asserted from the float64 masks).  A constant image with rw = 0 is 0 / 0:
    NaN for NaN.
2d  End to end on real operands: Gaussian taps of sigma 0.6 / 1.0 / 1.7 / 2.0, both deltas, randn image and noise, rw = 0.05;
    m, the global mean and out against float64 under mind_ref.out_bound, which is derived per voxel from the reference:
    q = (e + rw n)^2 carries 2 |ev| dev + dev^2 + u q with dev = u (|e| + |rw n| + |ev|) (the sum can cancel, so this is NOT
    relative to q), the three filter passes add 3 (ntaps + 1) u ssd, m and var inherit these through the minimum and the mean,
    and out = exp(-m / var) moves by out (e^{dq} - 1).

Measured on an MI355X (no bound was widened to fit; largest error / bound per comparison): 2a all 54 cases equal, the global
mean at 0.066 of its 32 u; 2b all 30 cases bit-equal; 2c fp32 0.34, bf16 and fp16 0.997 (the storage rounding itself goes up to
half an ulp = u_T |ref|); 2d m 0.16, global mean 0.005, out 0.09 (the float32 oracle sits at 0.07 of the same bound on the CPU).
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import mind_ref as mref
from oracle.mind import gauss_taps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
U = 2.0 ** -24
U_T = {0: 0.0, 1: 2.0 ** -8, 2: 2.0 ** -11}
SUB_T = {0: 0.0, 1: 2.0 ** -134, 2: 2.0 ** -25}
RW = float(np.float32(0.05))
TD, TH, TW = 8, 8, 32


def _cdiv(a, b):
    return -(-a // b)


def _align(n, a=256):
    return _cdiv(n, a) * a


def ntiles(shape):
    b, d, h, w = shape
    return b * _cdiv(d, TD) * _cdiv(h, TH) * _cdiv(w, TW)


def _lib():
    from dg_tta_amd import _lib as L
    return L.load()


def run(img, taps, rw, delta, noise=None, seed=None, ndhwc=False, ldc=12, dt=0):
    """One call of dgtta_mind3d_fwd (noise: tensor) or dgtta_mind3d_fwd_seeded (seed: (seed, offset, b0)).
    -> m [B,V,12] float32, global mean (float32 value), out as stored ([B,12,D,H,W] or [B,V,ldc]); all on the CPU."""
    from dg_tta_amd._lib import check, ptr, stream_of
    lib = _lib()
    b, _, d, h, w = img.shape
    v = d * h * w
    nws = lib.dgtta_mind3d_ws_bytes(b, d, h, w)
    off_p = _align(b * v * 12 * 4)
    off_g = off_p + _align(ntiles((b, d, h, w)) * 8)
    assert nws == off_g + 256, "the workspace layout restated in this test is not the library's"
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=DEV)            # all-ones: NaN as float and as double
    out = torch.full((b, v, ldc) if ndhwc else (b, 12, d, h, w), math.nan, dtype=TDT[dt], device=DEV)
    img_d = img.to(DEV).contiguous()
    h_taps = (ctypes.c_float * len(taps))(*taps)
    tail = (float(rw), int(delta), h_taps, len(taps), ptr(out), int(ndhwc), int(ldc), dt, ptr(ws), nws, b, d, h, w, stream_of())
    if seed is None:
        noise_d = noise.to(DEV).contiguous()
        check(lib.dgtta_mind3d_fwd(ptr(img_d), ptr(noise_d), *tail), "dgtta_mind3d_fwd")
    else:
        check(lib.dgtta_mind3d_fwd_seeded(ptr(img_d), seed[0], seed[1], seed[2], *tail), "dgtta_mind3d_fwd_seeded")
    torch.cuda.synchronize()
    ws = ws.cpu()
    m = ws[:b * v * 12 * 4].view(torch.float32).reshape(b, v, 12).clone()
    gm = float(ws[off_g:off_g + 4].view(torch.float32)[0])
    return m, gm, out.cpu()


def _where(idx, shape):
    """'b d h w c (tile ...)' of a flat index into m [B][V][12]."""
    b_, d, h, w = shape
    c = idx % 12
    vox = idx // 12
    x, y, z, b = vox % w, (vox // w) % h, (vox // (w * h)) % d, vox // (w * h * d)
    return f"b={b} d={z} h={y} w={x} c={c} (tile d{z // TD} h{y // TH} w{x // TW})"


def _ratio(what, got, ref, bound):
    """Asserts |got - ref| <= bound element by element (NaN fails), prints the largest error / bound."""
    err = (got.double() - ref).abs()
    r = torch.nan_to_num(err / bound, nan=math.inf)
    worst = float(r.max())
    print(f"RATIO {what}: max err/bound {worst:.3f} (max abs err {float(torch.nan_to_num(err, nan=math.inf).max()):.3e})")
    assert worst <= 1.0, f"{what}: error / bound = {worst:.3f} at flat index {int(r.argmax())}"
    return worst


# ------------------------------------------------------------------------------------------------ 2a
@functools.lru_cache(maxsize=None)
def _exact(delta, ntaps, shape):
    img, noise, taps, rw = mref.exact_inputs(delta, ntaps, shape)
    return img, noise, taps, rw, mref.stages(img, noise, taps, rw, delta)


@pytest.mark.parametrize("shape", mref.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("delta,ntaps", mref.EXACT_KERNELS)
def test_pass_a_bit_for_bit(delta, ntaps, shape):
    # vacuity guards: the launch order is permuted exactly where the table says, and the 7-tap second-pass columns feed outputs
    assert (ntiles(shape) % 8 == 0) == (shape in [(1, 9, 10, 37), (1, 16, 16, 64), (2, 16, 16, 40)])
    assert sum(1 for s in mref.EXACT_SHAPES if s[2] >= 8 and s[3] >= 33) >= 3
    img, noise, taps, rw, ref = _exact(delta, ntaps, shape)
    m, gm, _ = run(img, taps, rw, delta, noise=noise)
    bad = (m.double() != ref.m) | torch.isnan(m)
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(
            f"pass A (mind_ssd_kernel) delta={delta} taps={ntaps} {shape}: workspace m differs from the exact float64 m at "
            f"{int(bad.sum())} of {bad.numel()} elements, first at {_where(i, shape)}: got {float(m.reshape(-1)[i])!r}, "
            f"expected {float(ref.m.reshape(-1)[i])!r}")
    g64 = float(ref.gm)
    err = abs(gm - g64)
    print(f"RATIO global mean delta={delta} taps={ntaps} {shape}: err/bound {err / (mref.REL_GM * g64) if g64 else float(err > 0):.3f}")
    assert err <= mref.REL_GM * g64, f"pass A/B (block sums, mind_reduce_kernel): global mean {gm!r} vs float64 {g64!r}"


# ------------------------------------------------------------------------------------------------ 2b
SIGMA_OF = {3: 0.6, 5: 1.0, 7: 2.0}


@functools.lru_cache(maxsize=None)
def _randn_img(shape):
    b, d, h, w = shape
    return torch.randn(b, 1, d, h, w, generator=torch.Generator().manual_seed(sum(shape))) * 1.5 + 0.5


@pytest.mark.parametrize("shape", [(1, 1, 2, 3), (2, 2, 1, 40), (1, 3, 9, 33), (1, 9, 10, 70), (2, 16, 16, 40)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("delta,ntaps", mref.EXACT_KERNELS)
def test_seeded_equals_tensor_form_bit_for_bit(delta, ntaps, shape):
    from dg_tta_amd._lib import check, ptr, stream_of
    b, d, h, w = shape
    seed, offset, b0 = 0x1234567887654321, 2 ** 32 + 3, 1
    taps = [float(t) for t in gauss_taps(SIGMA_OF[ntaps])]
    assert len(taps) == ntaps
    noise = torch.full((b, 12, d, h, w), math.nan, device=DEV)
    check(_lib().dgtta_mind3d_noise_fill(ptr(noise), seed, offset, b0, b, d, h, w, stream_of()), "dgtta_mind3d_noise_fill")
    img = _randn_img(shape)
    m_t, gm_t, out_t = run(img, taps, RW, delta, noise=noise)
    m_s, gm_s, out_s = run(img, taps, RW, delta, seed=(seed, offset, b0))
    assert not bool(torch.isnan(m_t).any()) and not bool(torch.isnan(out_t).any())
    bad = m_s.view(torch.int32) != m_t.view(torch.int32)
    assert not bool(bad.any()), (f"pass A, seeded form (mind_column_seeded) delta={delta} taps={ntaps} {shape}: m differs from the "
                                 f"tensor form at {int(bad.sum())} elements, first at {_where(int(bad.reshape(-1).nonzero()[0]), shape)}")
    assert np.float32(gm_s).tobytes() == np.float32(gm_t).tobytes(), "seeded form: global mean differs from the tensor form"
    assert torch.equal(out_s.view(torch.int32), out_t.view(torch.int32)), "seeded form: out differs from the tensor form"


# ------------------------------------------------------------------------------------------------ 2c
@functools.lru_cache(maxsize=None)
def _clamp_case(batch):
    img, noise = mref.clamp_inputs()
    if batch == 2:                               # second sample: mirrored along W and 3 x the contrast
        img = torch.cat([img, 3.0 * img.flip(-1)])
        noise = torch.cat([noise, noise.flip(-2)])
    return img, noise


LAYOUTS = [(False, 12, 0)] + [(True, ldc, dt) for dt in (0, 1, 2) for ldc in (12, 13, 16)]


def _check_finish(what, img, noise, taps, rw, ndhwc, ldc, dt, need_low):
    b = img.shape[0]
    m, gm, out = run(img, taps, rw, 1, noise=noise, ndhwc=ndhwc, ldc=ldc, dt=dt)
    ref, var, varc, low, high = mref.finish(m, gm)
    n_low, n_high = int(low.sum()), int(high.sum())
    print(f"{what}: {n_low} low-clamped, {n_high} high-clamped of {low.numel()} voxels")
    assert n_high > 0 and (n_low > 0 or not need_low), f"{what}: vacuous, the clamp is not reached ({n_low} low, {n_high} high)"
    if ndhwc:
        pad = out[..., 12:]
        assert bool((pad == 0).all()), f"{what}: finish pass (mind_finish_kernel) left an out_ldc padding channel that is not 0"
        got = out[..., :12]
    else:
        got = out.reshape(b, 12, -1).permute(0, 2, 1)
    q = m.double() / varc[..., None]
    _ratio(f"finish pass (mind_finish_kernel) {what}", got, ref, mref.finish_bound(ref, q, U_T[dt], SUB_T[dt]))


@pytest.mark.parametrize("rw", [0.0, RW])
@pytest.mark.parametrize("ndhwc,ldc,dt", LAYOUTS)
def test_finish_pass_alone(ndhwc, ldc, dt, rw):
    """rw = 0: the flat halves sit on the low clamp, the spike's neighbourhood on the high one.  rw = 0.05: the noise lifts
    everything off the low clamp (none low-clamped is this case's property), the high clamp stays."""
    img, noise = _clamp_case(1)
    _check_finish(f"{'ndhwc' if ndhwc else 'ncdhw'} ldc={ldc} {TDT[dt]} rw={rw:g}", img, noise, [float(t) for t in gauss_taps(0.5)],
                  rw, ndhwc, ldc, dt, need_low=rw == 0.0)


@pytest.mark.parametrize("ndhwc,ldc,dt", [(False, 12, 0), (True, 13, 2), (True, 16, 1)])
def test_finish_pass_alone_batch_of_two(ndhwc, ldc, dt):
    img, noise = _clamp_case(2)
    _check_finish(f"B=2 {'ndhwc' if ndhwc else 'ncdhw'} ldc={ldc} {TDT[dt]} rw=0", img, noise, [float(t) for t in gauss_taps(0.5)],
                  0.0, ndhwc, ldc, dt, need_low=True)


@pytest.mark.parametrize("ndhwc,ldc,dt", [(False, 12, 0), (True, 13, 0), (True, 16, 1), (True, 12, 2)])
def test_constant_image_without_noise_is_nan_for_nan(ndhwc, ldc, dt):
    img = torch.full((2, 1, 3, 9, 33), 0.7)
    noise = torch.zeros(2, 12, 3, 9, 33)
    ref = mref.stages(img, noise, [0.25, 0.5, 0.25], 0.0, 1)
    assert bool(torch.isnan(ref.out).all())
    m, gm, out = run(img, [0.25, 0.5, 0.25], 0.0, 1, noise=noise, ndhwc=ndhwc, ldc=ldc, dt=dt)
    assert bool((m == 0).all()) and gm == 0.0, "pass A: a constant image without noise must give m = 0 and a global mean of 0"
    got = out[..., :12] if ndhwc else out
    assert bool(torch.isnan(got).all()), "finish pass (mind_finish_kernel): 0 / 0 must be NaN, as float64 gives"
    if ndhwc:
        assert bool((out[..., 12:] == 0).all()), "finish pass: padding channels must be 0"


# ------------------------------------------------------------------------------------------------ 2d
@functools.lru_cache(maxsize=None)
def _real(delta, sigma, shape):
    b, d, h, w = shape
    g = torch.Generator().manual_seed(int(10 * sigma) + 100 * delta + sum(shape))
    img = torch.randn(b, 1, d, h, w, generator=g) * 1.5
    noise = torch.randn(b, 12, d, h, w, generator=g)
    taps = [float(t) for t in gauss_taps(sigma)]
    return img, noise, taps, mref.stages(img, noise, taps, RW, delta)


@pytest.mark.parametrize("shape", [(1, 9, 10, 70), (2, 16, 16, 40)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("sigma", [0.6, 1.0, 1.7, 2.0])
@pytest.mark.parametrize("delta", [1, 2])
def test_end_to_end_on_real_operands(delta, sigma, shape):
    assert (ntiles(shape) % 8 == 0) == (shape == (2, 16, 16, 40))       # one shape in launch order, one permuted
    img, noise, taps, ref = _real(delta, sigma, shape)
    m, gm, out = run(img, taps, RW, delta, noise=noise)
    what = f"delta={delta} sigma={sigma} {shape}"
    dm = ref.dssd + ref.dssd.max(dim=-1, keepdim=True)[0] + U * ref.m
    _ratio(f"pass A (mind_ssd_kernel) m {what}", m, ref.m, dm + mref.TINY)
    gb = mref.gm_bound(ref)
    print(f"RATIO global mean {what}: err/bound {abs(gm - float(ref.gm)) / gb:.3f}")
    assert abs(gm - float(ref.gm)) <= gb, f"pass A/B global mean {what}: {gm!r} vs float64 {float(ref.gm)!r}"
    _ratio(f"out {what}", mref.to_voxel_major(out), ref.out_vm, mref.out_bound(ref, len(taps)))


def test_groups_are_separate_calls():
    """ops.mind3d(groups=2) on B = 4 = two calls of B = 2 (one variance-clamp mean per group), bit for bit."""
    from dg_tta_amd import ops
    g = torch.Generator().manual_seed(11)
    img = torch.randn(4, 1, 9, 10, 37, generator=g)
    img[2:] *= 20.0                              # the groups' global means differ by 400 x
    noise = torch.randn(4, 12, 9, 10, 37, generator=g)
    img, noise = img.to(DEV), noise.to(DEV)
    grouped = ops.mind3d(img, noise, groups=2)
    parts = torch.cat([ops.mind3d(img[:2], noise[:2]), ops.mind3d(img[2:], noise[2:])])
    assert torch.equal(grouped, parts) and not bool(torch.isnan(grouped).any())
    assert not torch.equal(grouped, ops.mind3d(img, noise))
