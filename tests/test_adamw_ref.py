"""CPU: tests/adamw_ref.py (the float64 restatement the GPU tests of csrc/adamw.hip compare with) against
torch.optim.AdamW in float64."""
import numpy as np
import pytest
import torch

import adamw_ref


@pytest.mark.parametrize("hyper", [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
                                   dict(lr=0.05, betas=(0.5, 0.75), eps=1e-3, weight_decay=0.0)])
def test_adamw_ref_matches_torch_float64(hyper):
    """Six steps; the second parameter never has a gradient (skipped: no state in torch, untouched here), the last one has
    none on steps 1 and 4 - its step counter falls behind the others', so its bias corrections differ."""
    rng = np.random.RandomState(5)
    shapes = [(7,), (3, 5), (4,), (2, 3, 2)]
    p0 = [rng.normal(size=s) for s in shapes]
    tp = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in p0]
    opt = torch.optim.AdamW(tp, **hyper)
    rp = [p.copy() for p in p0]
    rm, rv = [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]
    steps = [0] * 4
    for it in range(6):
        grads = [rng.normal(size=s) * 3 for s in shapes]
        grads[1] = None
        if it in (0, 3):
            grads[3] = None
        for t, g in zip(tp, grads):
            t.grad = None if g is None else torch.tensor(g, dtype=torch.float64)
        opt.step()
        for i, g in enumerate(grads):                  # one call per parameter: each at its own step number
            if g is None:
                continue
            steps[i] += 1
            (rp[i],), (rm[i],), (rv[i],) = adamw_ref.adamw_step([rp[i]], [g], [rm[i]], [rv[i]], steps[i], hyper["lr"],
                                                                hyper["betas"], hyper["eps"], hyper["weight_decay"],
                                                                as_kernel=False)
        for i, t in enumerate(tp):
            np.testing.assert_allclose(t.detach().numpy(), rp[i], rtol=1e-12, atol=1e-14)
            st = opt.state[t]
            assert (len(st) == 0) == (steps[i] == 0)
            if st:
                assert int(st["step"]) == steps[i]
                np.testing.assert_allclose(st["exp_avg"].numpy(), rm[i], rtol=1e-12, atol=1e-15)
                np.testing.assert_allclose(st["exp_avg_sq"].numpy(), rv[i], rtol=1e-12, atol=1e-15)
    assert steps == [6, 0, 6, 4] and np.array_equal(rp[1], p0[1])


def test_adamw_ref_skips_none_inside_a_list_and_divides_the_loss_scale_out():
    rng = np.random.RandomState(1)
    p, m, v = ([rng.normal(size=9) for _ in range(3)] for _ in range(3))
    v = [np.abs(x) for x in v]
    g = [rng.normal(size=9), None, rng.normal(size=9)]
    a = adamw_ref.adamw_step(p, g, m, v, 3, 1e-3)
    b = adamw_ref.adamw_step(p, [None if x is None else x * 1024 for x in g], m, v, 3, 1e-3, grad_scale=1024.0)
    for x, y in zip(a, b):
        for s, t in zip(x, y):
            np.testing.assert_allclose(s, t, rtol=1e-15)
    assert np.array_equal(a[0][1], p[1]) and np.array_equal(a[1][1], m[1]) and np.array_equal(a[2][1], v[1])
    assert not np.array_equal(a[0][0], p[0]) and a[0][1] is not p[1]


def test_kernel_scalars_are_fp32_values_close_to_the_exact_ones():
    k = adamw_ref.kernel_scalars(1000, 1e-4, 0.9, 0.999, 1e-8, 0.01, 1024.0)
    e = adamw_ref.exact_scalars(1000, *(adamw_ref.f32(x) for x in (1e-4, 0.9, 0.999, 1e-8, 0.01)), 1024.0)
    for a, b in zip(k, e):
        assert a == adamw_ref.f32(a) and abs(a - b) <= 3 * 2.0 ** -24 * abs(b)
    assert k[6] == 2.0 ** -10
    # the exact tier of tests/test_gpu_adamw.py: every scalar is a power of two or 1/2, 3/4 and survives unchanged
    assert adamw_ref.kernel_scalars(1, 2.0 ** -6, 0.5, 0.75, 0.0, 2.0 ** -4) == (2.0 ** -10, 0.5, 0.75, 0.0, 2.0 ** -5, 0.5, 1.0)


def test_the_gpu_tests_comparison_rejects_nan_and_a_wrong_element():
    """tests/test_gpu_adamw.py's _worst, run here on made-up kernel results: the reference rounded to fp32 is within the bounds,
    one NaN in p, m or v - or all of them NaN - fails, and so does one element off by a few ulps."""
    from test_gpu_adamw import HYPER, _worst
    rng = np.random.RandomState(2)
    shapes = [5, 300]
    rnd = lambda s=1.0: [(rng.standard_normal(n) * s).astype(np.float32).astype(np.float64) for n in shapes]
    p, g, m, v = rnd(), rnd(), rnd(0.3), [x * x for x in rnd(0.5)]
    v = [x.astype(np.float32).astype(np.float64) for x in v]
    sc = adamw_ref.kernel_scalars(2, HYPER["lr"], *HYPER["betas"], HYPER["eps"], HYPER["weight_decay"])
    ref = adamw_ref.adamw_step(p, g, m, v, 2, **HYPER)
    dev = lambda arrs: [torch.from_numpy(a.astype(np.float32)) for a in arrs]
    w = _worst(p, g, m, v, *(dev(r) for r in ref), lambda i: sc)
    assert np.all(w <= 1.0) and np.all(w > 0)
    for k in range(3):
        outs = [dev(r) for r in ref]
        outs[k][1][299] = float("nan")
        with pytest.raises(AssertionError, match="not finite"):
            _worst(p, g, m, v, *outs, lambda i: sc)
    with pytest.raises(AssertionError, match="not finite"):
        _worst(p, g, m, v, *([torch.full((n,), float("nan")) for n in shapes] for _ in range(3)), lambda i: sc)
    outs = [dev(r) for r in ref]
    outs[0][1][7] *= 1 + 2.0 ** -20
    assert _worst(p, g, m, v, *outs, lambda i: sc)[0] > 1.0
