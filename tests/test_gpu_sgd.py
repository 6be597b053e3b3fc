"""GPU: the clipped SGD kernels of csrc/sgd.hip (dgtta_grad_sumsq, dgtta_sgd_step) and optim.HipSGD against the float64
restatement tests/sgd_ref.py (licensed by tests/test_sgd_ref.py).

Tensor set (every test): 40 tensors in one call, so the norm and the step both span two launches of 32; element counts
1, 255, 256, 4095, 4096, 4097 (one workgroup takes 4096 elements: below, at and above it), 70 001 (18 workgroups, the
last ragged), and an 8192-element view that starts 4 bytes into its allocation (full chunks on the scalar path, which
the 16-byte path must not take); the gradient of tensor 20 is None.

EXACT TIER.  Every operand is chosen so that each operation of the update is exact in fp32, fused or not: p, buf in
[-2, 2] and g in [-4, 4] are integers, lr = 2^-6, mu = 0.5, wd = 2^-4, loss scale 1024 on gradients pre-multiplied by
1024, max_norm = 2^20 above the norm (coef = 1).  Then d is a multiple of 2^-4 below 5, after the first step p is a
multiple of 2^-11 below 2.2; in the second step d and buf are multiples of 2^-15 below 8, u of 2^-16 below 8, lr u of
2^-22, and p stays below 4: 24 significant bits at most.  The squares (<= 2^24) and their per-thread sums of 16 are
integers times 2^20 below 2^29, the total an integer below 2^24 times 2^20.  The results equal the float64 reference
bit for bit after rounding to fp32.

TOLERANCE TIER.  p, buf ~ N(0, 1), g ~ 1024 N(0, 1) with loss scale 1024 (norm ~ sqrt(N) >> 12: clipping active),
nnU-Net's lr = 1e-2, mu = 0.99, wd = 3e-5 as the fp32 values the kernel receives.  u = 2^-24; every fp32 operation
rounds its result by at most u relative; the reference gets the same inputs.
  sumsq   a thread adds 16 rounded squares in fp32: (1 + u)^16 - 1 < 17 u relative to its (all positive) terms; the sums
          continue in double (2^-53 per addition, N / 16 + 260 of them: below u / 100); the result is rounded to fp32
          once: |S_k - S| <= 18 u S.
  coef    sqrt halves the relative error of S (9 u) and rounds (<= 1 ulp = 2 u allowed); the division by the loss scale
          is exact (power of two); norm + 1e-6 rounds (u; the constant's own rounding, 1e-6 * u absolute, is below
          u norm / 10^7); the division rounds (2 u allowed): |coef_k - coef| <= 14 u coef.  E_C = 16 u is asserted; the
          margin covers every second-order term.
  update  with the reference's values, in the order of the kernel:
            dgc  = (E_C + u) |gc|                                   gc = (g / 1024) coef
            dd   = dgc + u |wd p| + u |d|                           d = gc + wd p
            dbuf = dd                            (first step)       buf = d
                 = dd + u |mu buf_old| + u |buf| (later steps)      buf = mu buf_old + d
            du   = dd + mu dbuf + u |mu buf| + u |u|   (Nesterov)   u = d + mu buf
                 = dbuf                                (plain)      u = buf
            dp   = lr du + u |lr u| + u |p_new|                     p_new = p - lr u
          |p_k - p_ref| <= dp and |buf_k - buf_ref| <= dbuf element by element.
  norm after clipping   from the kernel's p_new of a first step, in float64: g'_k = (p - p_new) / (lr (1 + mu)) - wd p
          (Nesterov: u = (1 + mu) d; plain: the divisor is lr).  g'_k - g' = -dp_err / (lr (1 + mu)), so by the triangle
          inequality | ||g'_k|| - 12 norm / (norm + 1e-6) | <= ||dp|| / (lr (1 + mu)).
Each comparison prints its largest error / bound ratio.  Measured on an MI355X (no bound widened): p 0.99 - the final rounding
of p_new is the bound's largest term and round-to-nearest reaches half an ulp -, buf 0.54 (first step) and 0.84, sumsq 0.009,
the norm after clipping 0.001 (11.9999983 against 11.99999997)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import sgd_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
E_C = 16 * U
SIZES = (1, 255, 256, 4095, 4096, 4097)
NONE_AT = 20


def f32(x):
    return ctypes.c_float(x).value


def _shapes():
    sizes = [SIZES[i % len(SIZES)] for i in range(40)]
    sizes[7], sizes[33] = 70001, 8192                      # one per launch of 32
    return sizes


def _alloc(n, misaligned):
    if misaligned:                                         # a contiguous view that starts 4 bytes into its allocation
        t = torch.empty(n + 1, dtype=torch.float32, device=DEV)[1:]
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t
    return torch.empty(n, dtype=torch.float32, device=DEV)


def _upload(arrays):
    out = []
    for i, a in enumerate(arrays):
        if a is None:
            out.append(None)
            continue
        t = _alloc(a.size, misaligned=(a.size == 8192))
        t.copy_(torch.from_numpy(a.astype(np.float32)))
        out.append(t)
    return out


def _ints(rng, lo, hi, with_none=True):
    arrs = [rng.randint(lo, hi + 1, n).astype(np.float64) for n in _shapes()]
    if with_none:
        arrs[NONE_AT] = None
    return arrs


def _normals(rng, scale=1.0, with_none=True):
    arrs = [(rng.standard_normal(n) * scale).astype(np.float32).astype(np.float64) for n in _shapes()]
    if with_none:
        arrs[NONE_AT] = None
    return arrs


def _host(ts):
    return [None if t is None else t.cpu().numpy().astype(np.float64) for t in ts]


def _bits_equal(dev_tensors, ref_arrays, what):
    for i, (t, r) in enumerate(zip(dev_tensors, ref_arrays)):
        if r is None:
            continue
        got, want = t.cpu().numpy(), r.astype(np.float32)
        assert want.astype(np.float64).tolist() == r.tolist(), f"{what}[{i}]: the reference itself is not exact in fp32"
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}[{i}] ({got.size} elements) differs"


# ------------------------------------------------------------------------------------------------ exact tier
EX = dict(lr=2.0 ** -6, momentum=0.5, weight_decay=2.0 ** -4, max_norm=2.0 ** 20, grad_scale=1024.0)


def test_grad_sumsq_exact_reproducible_and_argument_checks():
    from dg_tta_amd import ops
    from dg_tta_amd._lib import DgttaError
    rng = np.random.RandomState(0)
    g = [None if a is None else a * 1024 for a in _ints(rng, -4, 4)]
    gd = _upload(g)
    want = sgd_ref.grad_sumsq(g)
    assert want == float(np.float32(want)) and want < 2.0 ** 44
    ws = torch.full((ops.grad_sumsq_ws_bytes(sum(a.size for a in g if a is not None), 40),), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((), float("nan"), device=DEV)
    a = ops.grad_sumsq(gd, out=out, ws=ws)
    assert a is out and float(a) == want
    b = ops.grad_sumsq(gd)                                  # own workspace, own output: the same bits
    assert torch.equal(a, b)
    r = _upload(_normals(np.random.RandomState(1), 1024.0))
    r1, r2 = ops.grad_sumsq(r), ops.grad_sumsq(r)
    assert torch.equal(r1, r2)
    s = sgd_ref.grad_sumsq(_host(r))
    print(f"\nsumsq error / bound {abs(float(r1) - s) / (18 * U * s):.3f}")
    assert abs(float(r1) - s) <= 18 * U * s
    assert float(ops.grad_sumsq([None, None], out=out)) == 0.0          # nothing to add: a clean zero
    with pytest.raises(ValueError):
        ops.grad_sumsq(gd, ws=torch.empty(8, dtype=torch.uint8, device=DEV))
    with pytest.raises(DgttaError):
        ops.grad_sumsq([torch.ones(3)])


@pytest.mark.parametrize("nesterov", [True, False])
def test_sgd_step_exact_first_and_second_step(nesterov):
    from dg_tta_amd import ops
    rng = np.random.RandomState(2 + nesterov)
    p0 = _ints(rng, -2, 2, with_none=False)
    pd = _upload(p0)
    bd = [_alloc(a.size, a.size == 8192).fill_(float("nan")) for a in p0]     # first step: written, never read
    rp, rb = [a.copy() for a in p0], [None] * 40
    for step in range(2):
        g = _ints(rng, -4, 4)
        gs = [None if a is None else a * 1024 for a in g]
        gd = _upload(gs)
        sumsq = ops.grad_sumsq(gd)
        first = step == 0
        # tensors without a gradient are skipped by the kernel: NULL in the table, their p / buf untouched
        ops.sgd_step(pd, gd, bd, EX["lr"], EX["momentum"], EX["weight_decay"], nesterov, first_step=first,
                     grad_scale=EX["grad_scale"], sumsq=sumsq, max_norm=EX["max_norm"])
        rp, rb, coef = sgd_ref.sgd_step(rp, gs, rb, EX["lr"], EX["momentum"], EX["weight_decay"], nesterov, EX["max_norm"],
                                        EX["grad_scale"])
        assert coef == 1.0
        _bits_equal(pd, rp, f"p after step {step + 1}")
        _bits_equal(bd, rb, f"buf after step {step + 1}")
    assert torch.isnan(bd[NONE_AT]).all() and torch.equal(pd[NONE_AT].cpu(), torch.from_numpy(p0[NONE_AT]).float())
    # p, g AND buf small integers, a later step, no clipping pointer at all (coef = 1 by definition)
    p, b, g = _ints(rng, -2, 2, False), _ints(rng, -2, 2, False), _ints(rng, -4, 4)
    pd, bd, gd = _upload(p), _upload(b), _upload([None if a is None else a * 1024 for a in g])
    ops.sgd_step(pd, gd, bd, EX["lr"], EX["momentum"], EX["weight_decay"], nesterov, first_step=False, grad_scale=1024.0)
    rp, rb, _ = sgd_ref.sgd_step(p, g, b, EX["lr"], EX["momentum"], EX["weight_decay"], nesterov, max_norm=None)
    _bits_equal(pd, rp, "p, integer buffers")
    _bits_equal(bd, rb, "buf, integer buffers")


# ------------------------------------------------------------------------------------------------ tolerance tier
def _bounds(p, g, b_old, lr, mu, wd, nesterov, coef, inv_scale):
    """(dp, dbuf, p_ref, buf_ref) per tensor, from the derivation in the module docstring."""
    out = []
    for pi, gi, bi in zip(p, g, b_old):
        if gi is None:
            out.append(None)
            continue
        gc = gi * inv_scale * coef
        d = gc + wd * pi
        dgc = (E_C + U) * np.abs(gc)
        dd = dgc + U * np.abs(wd * pi) + U * np.abs(d)
        if bi is None:
            buf, dbuf = d, dd
        else:
            buf = mu * bi + d
            dbuf = dd + U * np.abs(mu * bi) + U * np.abs(buf)
        if nesterov:
            u = d + mu * buf
            du = dd + mu * dbuf + U * np.abs(mu * buf) + U * np.abs(u)
        else:
            u, du = buf, dbuf
        pn = pi - lr * u
        out.append((lr * du + U * np.abs(lr * u) + U * np.abs(pn), dbuf, pn, buf))
    return out


@pytest.mark.parametrize("nesterov", [True, False])
def test_sgd_step_clipping_active_within_the_derived_bound(nesterov):
    from dg_tta_amd import ops
    rng = np.random.RandomState(10 + nesterov)
    lr, mu, wd, max_norm, scale = f32(1e-2), f32(0.99), f32(3e-5), 12.0, 1024.0
    p = _normals(rng, with_none=False)
    pd = _upload(p)
    bd = [_alloc(a.size, a.size == 8192).fill_(float("nan")) for a in p]
    b_old = [None] * 40
    for step in range(2):
        g = _normals(rng, scale)
        gd = _upload(g)
        sumsq = ops.grad_sumsq(gd)
        p_in = _host(pd)
        ops.sgd_step(pd, gd, bd, lr, mu, wd, nesterov, first_step=(step == 0), grad_scale=scale, sumsq=sumsq, max_norm=max_norm)
        s = sgd_ref.grad_sumsq(g)
        norm = np.sqrt(s) / scale
        assert norm > 20 * max_norm                                    # clipping well active
        coef = sgd_ref.clip_coef(s, max_norm, scale)
        bounds = _bounds(p_in, g, b_old, lr, mu, wd, nesterov, coef, 1.0 / scale)
        p_out, b_out = _host(pd), _host(bd)
        worst_p = worst_b = 0.0
        for i, bnd in enumerate(bounds):
            if bnd is None:
                assert np.array_equal(p_out[i], p_in[i]) and np.isnan(b_out[i]).all()
                continue
            dp, dbuf, pn, buf = bnd
            worst_p = max(worst_p, float(np.max(np.abs(p_out[i] - pn) / dp)))
            worst_b = max(worst_b, float(np.max(np.abs(b_out[i] - buf) / dbuf)))
        print(f"\nstep {step + 1} nesterov {nesterov}: p error / bound {worst_p:.3f}, buf error / bound {worst_b:.3f}")
        assert worst_p <= 1.0 and worst_b <= 1.0
        if step == 0:
            div = lr * (1 + mu) if nesterov else lr
            gk = [(a - c) / div - wd * a for a, c, gi in zip(p_in, p_out, g) if gi is not None]
            got = np.sqrt(sum(np.sum(x ** 2) for x in gk))
            want = max_norm * norm / (norm + 1e-6)
            bound = np.sqrt(sum(np.sum(bnd[0] ** 2) for bnd in bounds if bnd is not None)) / div
            print(f"norm after clipping {got:.9f}, expected {want:.9f}, error / bound {abs(got - want) / bound:.3f}")
            assert abs(got - want) <= bound and bound < 0.05
        b_old = [None if g[i] is None else b_out[i] for i in range(40)]


# ------------------------------------------------------------------------------------------------ the optimiser
def _params(arrays):
    return [torch.nn.Parameter(t) for t in _upload(arrays)]


def _set_grads(params, arrays):
    for p, g in zip(params, _upload(arrays)):
        p.grad = g


def _hip_sgd(params, **kw):
    from dg_tta_amd.optim import HipSGD
    return HipSGD(params, lr=EX["lr"], momentum=EX["momentum"], weight_decay=EX["weight_decay"], max_grad_norm=EX["max_norm"], **kw)


def test_hip_sgd_three_steps_twice_are_bit_identical():
    from dg_tta_amd.optim import HipSGD
    rng = np.random.RandomState(20)
    p0 = _normals(rng, with_none=False)
    grads = [_normals(rng, 3.0) for _ in range(3)]

    def run():
        params = _params(p0)
        opt = HipSGD(params)
        for g in grads:
            _set_grads(params, g)
            opt.step()
            opt.zero_grad(set_to_none=True)
        return [p.detach().clone() for p in params], [opt.state[p].get("momentum_buffer") for p in params]
    (pa, ba), (pb, bb) = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert ba[NONE_AT] is None and bb[NONE_AT] is None
    assert all(torch.equal(x, y) for x, y in zip(ba, bb) if x is not None)
    assert not torch.equal(pa[0], torch.from_numpy(p0[0]).float().to(DEV))


def test_hip_sgd_overflow_skips_the_step_and_the_next_one_is_a_first_step():
    rng = np.random.RandomState(30)
    p0 = _ints(rng, -2, 2, with_none=False)
    params = _params(p0)
    opt = _hip_sgd(params, grad_scale=1024.0)
    bad = [None if a is None else a * 1024 for a in _ints(rng, -4, 4)]
    bad[3][100] = np.inf
    _set_grads(params, bad)
    opt.step()
    _bits_equal([p.data for p in params], p0, "p after the skipped step")
    assert opt.resolve_overflow() is True and opt.grad_scale == 512.0 and opt.skipped_steps == 1
    assert all("momentum_buffer" not in opt.state[p] for p in params)            # still uninitialised
    g = _ints(rng, -4, 4)
    _set_grads(params, [None if a is None else a * 512 for a in g])
    opt.step()
    assert opt.resolve_overflow() is False and opt.grad_scale == 512.0
    rp, rb, _ = sgd_ref.sgd_step(p0, g, [None] * 40, EX["lr"], EX["momentum"], EX["weight_decay"], True, EX["max_norm"])
    _bits_equal([p.data for p in params], rp, "p after the clean step")           # buf = d: a first step
    _bits_equal([opt.state[p].get("momentum_buffer") for p in params], rb, "buf after the clean step")
    nan = [None if a is None else a * 512 for a in _ints(rng, -4, 4)]
    nan[39][0] = np.nan
    _set_grads(params, nan)
    opt.step()
    _bits_equal([p.data for p in params], rp, "p after the second skipped step")
    _bits_equal([opt.state[p].get("momentum_buffer") for p in params], rb, "buf after the second skipped step")
    assert opt.resolve_overflow() is True and opt.grad_scale == 256.0 and opt.skipped_steps == 2
    assert "momentum_buffer" in opt.state[params[0]] and "momentum_buffer" not in opt.state[params[NONE_AT]]


def test_hip_sgd_state_dict_interchanges_with_torch_sgd():
    from dg_tta_amd.optim import HipSGD
    rng = np.random.RandomState(40)
    p0 = _normals(rng, with_none=False)[:6]
    g1, g2 = _normals(rng, 0.1)[:6], _normals(rng, 0.1)[:6]
    g1[2] = g2[2] = None
    params = _params(p0)
    hip = HipSGD(params, max_grad_norm=None)
    _set_grads(params, g1)
    hip.step()
    sd = hip.state_dict()
    assert set(sd["state"]) == {0, 1, 3, 4, 5} and all(set(s) == {"momentum_buffer"} for s in sd["state"].values())
    # -> torch.optim.SGD: same buffers, and its next step is the reference's
    tparams = [torch.nn.Parameter(p.detach().clone()) for p in params]
    tsgd = torch.optim.SGD(tparams, lr=0.5)
    # (load_state_dict keeps a tensor that already has the parameter's device and dtype: without the copy torch's in-place
    # step would write into HipSGD's buffers)
    tsgd.load_state_dict(copy.deepcopy(sd))
    grp = tsgd.param_groups[0]
    assert (grp["lr"], grp["momentum"], grp["nesterov"], grp["weight_decay"], grp["dampening"]) == (1e-2, 0.99, True, 3e-5, 0.0)
    for i in (0, 1, 3, 4, 5):
        assert torch.equal(tsgd.state[tparams[i]]["momentum_buffer"], hip.state[params[i]]["momentum_buffer"])
    _set_grads(tparams, g2)
    tsgd.step()
    rp, rb, _ = sgd_ref.sgd_step(_host([p.data for p in params]), g2, [None if i == 2 else b for i, b in
                                 enumerate(_host([hip.state[p].get("momentum_buffer") for p in params]))],
                                 f32(1e-2), f32(0.99), f32(3e-5), True, max_norm=None)
    for t, r in zip(tparams, rp):
        np.testing.assert_allclose(t.detach().cpu().numpy(), r, rtol=1e-5, atol=1e-6)
    # ... and back: a HipSGD that loads torch's state continues exactly as the one that never stopped
    back_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    pre = torch.optim.SGD([torch.nn.Parameter(p.detach().clone()) for p in params], lr=1e-2, momentum=0.99, nesterov=True,
                          weight_decay=3e-5)
    pre.load_state_dict(copy.deepcopy(sd))
    back = HipSGD(back_params, max_grad_norm=None)
    back.load_state_dict(copy.deepcopy(pre.state_dict()))
    _set_grads(params, g2)
    _set_grads(back_params, g2)
    hip.step()
    back.step()
    for a, b in zip(params, back_params):
        assert torch.equal(a.detach(), b.detach())
    for a, b in zip(params, back_params):
        ba, bb = hip.state[a].get("momentum_buffer"), back.state[b].get("momentum_buffer")
        assert (ba is None) == (bb is None) and (ba is None or torch.equal(ba, bb))
