"""Licence of tests/gin_ref.py (CPU): the float64 restatement reproduces the committed goldens and oracle.gin.gin_chain within
the float32 forward error ceiling it derives itself, the exact cases are exact (float32 == float64 bit for bit up to `mixed`) and
stay under the magnitude cap, and the ceiling is loose enough to need the oracle-relative limit next to it."""
import pytest
import torch

import gin_ref as gref
from conftest import load_golden
from oracle import gin as ogin

# a one-unit error of an exact case must be at least 16 x the tolerance REL_RECOVER |mixed| of the GPU comparison
EXACT_CAP = 1.0 / (16 * gref.REL_RECOVER)


def _check(out32, ref, what):
    err = (out32.double() - ref.out).abs()
    ratio = float((err / ref.ceil_out.clamp(min=1e-300)).max())
    print(f"RATIO {what}: float32 oracle vs float64, max err/ceiling {ratio:.4f} (max abs err {float(err.max()):.3e})")
    assert ratio <= 1.0, f"{what}: error / ceiling = {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("i", range(7))
def test_reproduces_the_goldens(i):
    g = load_golden(f"gin_{i}")
    ks = [int(k) for k in g["ks"]]
    ref = gref.chain(g["x"], g["alpha"], ks, [g[f"ker{j}"] for j in range(4)], [g[f"shift{j}"] for j in range(4)])
    _check(g["out"], ref, f"golden gin_{i} ks={ks}")


@pytest.mark.parametrize("ks", gref.ALL_KS, ids=lambda k: "".join(map(str, k)))
def test_reproduces_the_oracle(ks):
    x, alpha, _, kers, shifts = gref.real_inputs(ks, (2, 9, 11, 37))
    ref = gref.chain(x, alpha, list(ks), kers, shifts)
    _check(ogin.gin_chain(x, alpha, list(ks), kers, shifts), ref, f"oracle ks={ks}")
    for b in range(2):      # norm preservation of the float64 result: 1e-5 / |mixed| off 1
        assert abs(float(ref.out[b].norm() / ref.n_in[b]) - 1.0) <= 1.01 * gref.EPS32 / float(ref.n_mix[b])


@pytest.mark.parametrize("shape", gref.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ks", gref.ALL_KS, ids=lambda k: "".join(map(str, k)))
def test_exact_cases_are_exact(ks, shape):
    x, alpha, k, kers, shifts = gref.exact_inputs(ks, shape)
    r64 = gref.chain(x, alpha, k, kers, shifts, ceiling=False)
    r32 = gref.chain(x, alpha, k, kers, shifts, dtype=torch.float32, ceiling=False)
    assert r32.mixed.dtype == torch.float32
    assert torch.equal(r32.y.double(), r64.y) and torch.equal(r32.mixed.double(), r64.mixed)
    assert bool((r64.y >= 1).all()) and bool((r64.y == r64.y.round()).all())        # positive integers: LeakyReLU = identity
    assert 0 < float(r64.mixed.abs().max()) <= EXACT_CAP, f"max |mixed| {float(r64.mixed.abs().max())} above {EXACT_CAP:.0f}"
    assert all(float(s.min()) >= 1 for s in shifts)
