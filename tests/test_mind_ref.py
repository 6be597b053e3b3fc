"""Licence of tests/mind_ref.py (CPU): the float64 restatement reproduces the committed goldens and oracle.mind.mind3d
within the float32 error ceiling it derives itself (out_bound: the oracle IS a float32 evaluation, so this also checks that the
ceiling holds for one), the dyadic cases of pass A are exact (float32 == float64 bit for bit), and the clamp case clamps on both
sides."""
import numpy as np
import pytest
import torch

import mind_ref as mref
from conftest import load_golden
from oracle import mind as omind

RW = float(np.float32(0.05))


def _taps(sigma):
    return [float(t) for t in omind.gauss_taps(sigma)]


def _check(out32, ref, ntaps, what):
    bound = mref.out_bound(ref, ntaps)
    err = (mref.to_voxel_major(out32.double()) - ref.out_vm).abs()
    ratio = float((err / bound).max())
    print(f"RATIO {what}: float32 evaluation vs float64, max err/bound {ratio:.3f} (max abs err {float(err.max()):.3e})")
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f}"


@pytest.mark.parametrize("tag", ["16", "ragged", "const"])
def test_reproduces_the_goldens(tag):
    g = load_golden(f"mind3d_{tag}")
    ref = mref.stages(g["img"], g["noise"], _taps(1.0), RW, 1)
    _check(g["out"], ref, 5, f"golden mind3d_{tag}")
    # the committed goldens never reach the variance clamp (the GPU tests bring their own case that does)
    print(f"golden mind3d_{tag}: low-clamped {int(ref.low.sum())}, high-clamped {int(ref.high.sum())} of {ref.low.numel()}")


@pytest.mark.parametrize("delta,sigma", [(1, 0.6), (1, 1.0), (2, 1.7), (2, 2.0)])
def test_reproduces_the_oracle(delta, sigma):
    g = torch.Generator().manual_seed(int(10 * sigma) + delta)
    img = torch.randn(2, 1, 9, 10, 37, generator=g) * 1.5
    noise = torch.randn(2, 12, 9, 10, 37, generator=g)
    taps = _taps(sigma)
    ref = mref.stages(img, noise, taps, RW, delta)
    _check(omind.mind3d(img, noise, delta=delta, sigma=sigma), ref, len(taps), f"oracle delta={delta} sigma={sigma}")
    # the finish pass alone, on the staged m and mean, is the same function
    out, _, _, low, high = mref.finish(ref.m, ref.gm)
    assert torch.equal(out, ref.out_vm) and torch.equal(low, ref.low) and torch.equal(high, ref.high)


@pytest.mark.parametrize("shape", mref.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("delta,ntaps", mref.EXACT_KERNELS)
def test_exact_cases_are_exact(delta, ntaps, shape):
    """The same formula in float32 equals float64 bit for bit, so any difference of the kernel's m is a kernel error."""
    img, noise, taps, rw = mref.exact_inputs(delta, ntaps, shape)
    assert all(float(np.float32(t)) == t for t in taps) and abs(sum(taps) - 1.0) == 0.0
    r64 = mref.stages(img, noise, taps, rw, delta)
    r32 = mref.stages(img, noise, taps, rw, delta, dtype=torch.float32)
    assert r32.m.dtype == torch.float32
    assert torch.equal(r32.ssd.double(), r64.ssd) and torch.equal(r32.m.double(), r64.m)
    assert float(r64.m.max()) > 0 or shape == (1, 1, 1, 1)


def test_clamp_case_clamps_on_both_sides():
    img, noise = mref.clamp_inputs()
    n = img.numel()
    r0 = mref.stages(img, noise, _taps(0.5), 0.0, 1)
    r5 = mref.stages(img, noise, _taps(0.5), RW, 1)
    print(f"rw 0: low {int(r0.low.sum())} high {int(r0.high.sum())}; rw 0.05: low {int(r5.low.sum())} high {int(r5.high.sum())} of {n}")
    assert int(r0.low.sum()) > n // 2 and int(r0.high.sum()) > 0
    assert int(r5.low.sum()) == 0 and int(r5.high.sum()) > 0
    assert bool(torch.isfinite(r0.out).all()) and bool(torch.isfinite(r5.out).all())


def test_constant_image_without_noise_is_nan():
    """m = 0 everywhere, the global mean is 0, the clamp leaves var = 0 and 0 / 0 is NaN: what mind.py computes."""
    img = torch.full((1, 1, 3, 4, 5), 0.7)
    ref = mref.stages(img, torch.zeros(1, 12, 3, 4, 5), _taps(0.5), 0.0, 1)
    assert float(ref.gm) == 0.0 and bool(torch.isnan(ref.out).all())
    assert bool(torch.isnan(omind.mind3d(img, torch.zeros(1, 12, 3, 4, 5), sigma=0.5, randn_weighting=0.0)).all())
