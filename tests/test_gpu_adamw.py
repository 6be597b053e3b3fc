"""GPU: the multi-tensor AdamW kernels of csrc/adamw.hip (dgtta_adamw_step, dgtta_grads_nonfinite) and optim.HipAdamW against
the float64 restatement tests/adamw_ref.py (licensed by tests/test_adamw_ref.py).

Tensor set (every test): 40 entries in one call.  Entries 20 and 31 have no gradient (NULL in the table: skipped, they do not
count towards the 32 tensors of a launch, and 31 is the 32nd entry), so the first launch takes entries 0..33 and the second
34..39: the table (`blk_start` walk) is exercised at the first workgroup of every tensor of both launches.  Element counts 1,
255, 256, 4095, 4096, 4097 (one workgroup takes 4096 elements: below, at and above it), 70 001 (18 workgroups, the last ragged;
one in each launch), and an 8192-element view that starts 4 bytes into its allocation.  Two more tensors that are NOT in the
table lie in the same allocations' neighbourhood and must stay bit-identical, as must p, m and v of the entries without gradient.

EXACT TIER.  Step 1 from zero state, b1 = 1/2, b2 = 3/4, eps = 0, lr = 2^-6, wd = 2^-4, p integer in [-2, 2], g a nonzero
integer in [-4, 4] (times the loss scale 1024, divided out exactly).  Then 1 - lr wd = 1 - 2^-10 and p (1 - 2^-10) are exact,
m = g / 2, v = (g / 4) g = g^2 / 4, sqrt(v) = |g| / 2 (a correctly rounded sqrt returns an exact root), sqrt(bc2) = 1/2,
denom = |g|, m / denom = +-1/2, lr / bc1 = 2^-5, and p_new = p (1 - 2^-10) -+ 2^-6 is a multiple of 2^-10 below 4: every
operation is exact in fp32 and the kernel's p, m, v equal the float64 reference bit for bit.

TOLERANCE TIER.  u = 2^-24; every fp32 operation rounds its result by at most u relative (sqrt and division: 2 u = 1 ulp
allowed); the reference gets the fp32 scalars the kernel receives (adamw_ref.kernel_scalars) and the same fp32 inputs; the loss
scale is a power of two, so g' = g / scale is exact.  With the reference's values, in the kernel's order:
    c1 = fl(1 - lr_wd), p1 = fl(p c1)                          dp1 = 2 u |p1|
    t = fl(fl(g' - m) fl(1 - b1)), m' = fl(m + t)              dm  = 3 u |t| + u |m'|
    a = fl(v b2), c = fl(fl(fl(1 - b2) g') g'), v' = fl(a + c) dv  = u |a| + 3 u |c| + u |v'|
    s = sqrt(v')                                               ds  = min(dv / (2 s), sqrt(dv)) + 2 u s
    q = fl(s / sqrt_bc2)                                       dq  = ds / sqrt_bc2 + 2 u q
    den = fl(q + eps)                                          dden = dq + u den
    r = fl(m' / den)                                           dr  = (dm + |r| dden) / (den - dden) + 2 u |r|
    w = fl(step_size r)                                        dw  = step_size dr + u |w|
    p' = fl(p1 - w)                                            dp  = dp1 + dw + u |p'|
Each bound is multiplied by 1 + 2^-20 (= 16 u) for the second-order terms.  |p_k - p'| <= dp, |m_k - m'| <= dm,
|v_k - v'| <= dv element by element; every comparison prints its largest error / bound.
Measured on an MI355X (no bound widened), largest error / bound: step 1 p 0.68, m 0.24, v 0.49; step 2 p 0.72, m 0.98, v 0.98;
step 1000 p 0.74, m 1.00 (0.997), v 0.97, the same with either loss scale; HipAdamW with mixed step counters p 0.73, m 0.99,
v 0.95.  The last rounding of m' and v' is the bounds' largest term and round-to-nearest reaches half an ulp, as in
tests/test_gpu_sgd.py.  The exact tier holds bit for bit."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import adamw_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
SIZES = (1, 255, 256, 4095, 4096, 4097)
NONE_AT = (20, 31)
N = 40


def _shapes():
    sizes = [SIZES[i % len(SIZES)] for i in range(N)]
    sizes[7], sizes[33], sizes[36] = 70001, 8192, 70001    # 33: the last tensor of the first launch; 36: in the second
    return sizes


def _alloc(n, misaligned):
    if misaligned:                                         # a contiguous view that starts 4 bytes into its allocation
        t = torch.empty(n + 1, dtype=torch.float32, device=DEV)[1:]
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t
    return torch.empty(n, dtype=torch.float32, device=DEV)


def _upload(arrays):
    out = []
    for a in arrays:
        if a is None:
            out.append(None)
            continue
        t = _alloc(a.size, misaligned=(a.size == 8192))
        t.copy_(torch.from_numpy(a.astype(np.float32)))
        out.append(t)
    return out


def _with_none(arrs):
    return [None if i in NONE_AT else a for i, a in enumerate(arrs)]


def _ints(rng, lo, hi, nonzero=False):
    out = []
    for n in _shapes():
        a = rng.randint(lo, hi + 1, n).astype(np.float64)
        if nonzero:
            a[a == 0] = hi
        out.append(a)
    return out


def _normals(rng, scale=1.0, positive=False):
    out = [(rng.standard_normal(n) * scale).astype(np.float32).astype(np.float64) for n in _shapes()]
    return [np.abs(a) for a in out] if positive else out


def _host(ts):
    return [None if t is None else t.cpu().numpy().astype(np.float64) for t in ts]


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _bits_equal(dev_tensors, ref_arrays, what):
    for i, (t, r) in enumerate(zip(dev_tensors, ref_arrays)):
        got, want = t.cpu().numpy(), r.astype(np.float32)
        assert want.astype(np.float64).tolist() == r.tolist(), f"{what}[{i}]: the reference itself is not exact in fp32"
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}[{i}] ({got.size} elements) differs"


def _bounds(p, g, m, v, sc):
    """(p', m', v', dp, dm, dv) of one tensor, from the derivation in the module docstring."""
    lr_wd, b1, b2, eps, step_size, sqrt_bc2, inv_scale = sc
    gi = g * inv_scale
    p1 = p * (1.0 - lr_wd)
    dp1 = 2 * U * np.abs(p1)
    t = (gi - m) * (1.0 - b1)
    mn = m + t
    dm = 3 * U * np.abs(t) + U * np.abs(mn)
    a, c = v * b2, ((1.0 - b2) * gi) * gi
    vn = a + c
    dv = U * np.abs(a) + 3 * U * np.abs(c) + U * np.abs(vn)
    s = np.sqrt(vn)
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.where(s > 0, np.minimum(dv / (2 * s), np.sqrt(dv)), np.sqrt(dv)) + 2 * U * s
    q = s / sqrt_bc2
    dq = ds / sqrt_bc2 + 2 * U * q
    den = q + eps
    dden = dq + U * den
    r = mn / den
    dr = (dm + np.abs(r) * dden) / (den - dden) + 2 * U * np.abs(r)
    w = step_size * r
    dw = step_size * dr + U * np.abs(w)
    pn = p1 - w
    dp = dp1 + dw + U * np.abs(pn)
    return pn, mn, vn, dp * SLACK, dm * SLACK, dv * SLACK


def _worst(p_in, g, m_in, v_in, pd, md, vd, scalars_of):
    """Largest error / bound over every tensor with a gradient (scalars_of(i): the kernel scalars of entry i); entries
    without one must be bit-identical to their inputs."""
    worst = np.zeros(3)
    p_out, m_out, v_out = _host(pd), _host(md), _host(vd)
    for i in range(len(p_in)):
        if g[i] is None:
            assert np.array_equal(p_out[i], p_in[i]) and np.array_equal(m_out[i], m_in[i]) and np.array_equal(v_out[i], v_in[i])
            continue
        pn, mn, vn, dp, dm, dv = _bounds(p_in[i], g[i], m_in[i], v_in[i], scalars_of(i))
        for k, (got, want, bnd) in enumerate(((p_out[i], pn, dp), (m_out[i], mn, dm), (v_out[i], vn, dv))):
            assert np.all(np.isfinite(got)), f"tensor {i}: {'pmv'[k]} is not finite"
            err = np.abs(got - want)
            assert np.all(err[bnd == 0] == 0)
            worst[k] = np.max([worst[k], np.max(err[bnd > 0] / bnd[bnd > 0], initial=0.0)])      # (np.max: a NaN would pass through)
    return worst


HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


# ------------------------------------------------------------------------------------------------ exact tier
@pytest.mark.parametrize("grad_scale", [1.0, 1024.0])
def test_adamw_first_step_exact(grad_scale):
    from dg_tta_amd import ops
    rng = np.random.RandomState(3)
    p0, g = _ints(rng, -2, 2), _with_none(_ints(rng, -4, 4, nonzero=True))
    zeros = [np.zeros(n) for n in _shapes()]
    pd, md, vd = _upload(p0), _upload(zeros), _upload(zeros)
    gd = _upload([None if a is None else a * grad_scale for a in g])
    hyper = dict(lr=2.0 ** -6, betas=(0.5, 0.75), eps=0.0, weight_decay=2.0 ** -4)
    ops.adamw_step(pd, gd, md, vd, 1, grad_scale=grad_scale, **hyper)
    rp, rm, rv = adamw_ref.adamw_step(p0, g, zeros, zeros, 1, hyper["lr"], hyper["betas"], 0.0, hyper["weight_decay"])
    _bits_equal(pd, rp, "p")
    _bits_equal(md, rm, "m")
    _bits_equal(vd, rv, "v")
    for i in NONE_AT:
        assert not md[i].any() and not vd[i].any() and np.array_equal(rp[i], p0[i])
    assert any(not np.array_equal(a, b) for a, b in zip(rp, p0))


# ------------------------------------------------------------------------------------------------ tolerance tier
@pytest.mark.parametrize("grad_scale", [1.0, 1024.0])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adamw_step_within_the_derived_bound(step, grad_scale):
    """Step 1 from zero state, steps 2 and 1000 (bias corrections 0.19 / 0.002 and 1 - 4e-46 / 0.63) from a given one."""
    from dg_tta_amd import ops
    rng = np.random.RandomState(10 + step)
    p = _normals(rng)
    g = _with_none(_normals(rng, grad_scale))
    if step == 1:
        m, v = [np.zeros(n) for n in _shapes()], [np.zeros(n) for n in _shapes()]
    else:
        m, v = _normals(rng, 0.3), [(a * a).astype(np.float32).astype(np.float64) for a in _normals(rng, 0.5)]
    pd, md, vd, gd = _upload(p), _upload(m), _upload(v), _upload(g)
    outside = [torch.full((4097,), 1.25, device=DEV), torch.full((300,), -7.0, device=DEV)]      # not in the table
    ops.adamw_step(pd, gd, md, vd, step, grad_scale=grad_scale, **HYPER)
    sc = adamw_ref.kernel_scalars(step, HYPER["lr"], *HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], grad_scale)
    assert sc[6] * grad_scale == 1.0                                   # a power of two: dividing it out is exact
    wp, wm, wv = _worst(p, g, m, v, pd, md, vd, lambda i: sc)
    print(f"\nstep {step} scale {grad_scale:g}: error / bound p {wp:.3f}, m {wm:.3f}, v {wv:.3f}")
    assert wp <= 1.0 and wm <= 1.0 and wv <= 1.0
    assert (outside[0] == 1.25).all() and (outside[1] == -7.0).all()
    # the reference with the kernel's scalars is the one that counts: it moved the parameters by about lr
    rp, _, _ = adamw_ref.adamw_step(p, g, m, v, step, grad_scale=grad_scale, **{k: HYPER[k] for k in ("lr", "betas", "eps")},
                                    weight_decay=HYPER["weight_decay"])
    moved = max(float(np.abs(a - b).max()) for a, b, gi in zip(rp, p, g) if gi is not None)
    assert moved > 1e-4


# ------------------------------------------------------------------------------------------------ the overflow guard
def _nonfinite(gd, flag):
    """dgtta_grads_nonfinite through the C ABI: None entries stay in the table as NULL pointers."""
    from dg_tta_amd import _lib
    lib = _lib.load()
    n = len(gd)
    hg = (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in gd])
    hn = (ctypes.c_int64 * n)(*[0 if t is None else t.numel() for t in gd])
    flag.zero_()
    _lib.check(lib.dgtta_grads_nonfinite(hg, hn, n, flag.data_ptr(), _lib.stream_of(flag.device)), "dgtta_grads_nonfinite")
    return int(flag.item())


def test_grads_nonfinite_every_value_and_position_and_the_skipped_step():
    from dg_tta_amd import ops
    rng = np.random.RandomState(40)
    g = _with_none(_normals(rng))
    big, tiny = 3.4028234e38, 1e-42                          # FLT_MAX and a subnormal: finite
    g[0][0], g[7][70000], g[7][4096], g[38][1] = big, -big, tiny, -tiny
    g[33][:4] = [big, -big, tiny, -tiny]                     # (the scalar path's tensor)
    gd = _upload(g)
    assert float(gd[0][0]) == float(np.float32(big)) and float(gd[7][4096]) == float(np.float32(tiny)) != 0.0
    assert np.isfinite(np.float32(big)) and np.float32(tiny) < np.finfo(np.float32).tiny
    flag = torch.zeros((), dtype=torch.int32, device=DEV)
    assert _nonfinite(gd, flag) == 0                         # FLT_MAX, subnormals and NULL entries are not flagged
    assert _nonfinite([None, None], flag) == 0
    # (entry, element): element 0 of the table; the last element of a ragged last chunk; the first element of a tensor's
    # second workgroup; a tensor of the second launch (its own last element: 4097 = one full workgroup + 1)
    places = [(0, 0), (7, 70000), (7, 4096), (35, 4096), (36, 70000)]
    assert _shapes()[35] == 4097 and _shapes()[0] == 1 and min(i for i, _ in places[3:]) >= 34
    for bad in (float("inf"), float("-inf"), float("nan")):
        for i, e in places:
            keep = float(gd[i][e])
            gd[i][e] = bad
            assert _nonfinite(gd, flag) == 1, (bad, i, e)
            gd[i][e] = keep
            assert _nonfinite(gd, flag) == 0, (bad, i, e)
    # a set flag skips the whole step, both launches: p, m, v bit-identical; a clear one lets it through
    p, m, v = _normals(rng), _normals(rng, 0.3), _normals(rng, 0.5, positive=True)
    pd, md, vd = _upload(p), _upload(m), _upload(v)
    before = [[_bits(t).copy() for t in ts] for ts in (pd, md, vd)]
    gd[35][4096] = float("inf")
    assert _nonfinite(gd, flag) == 1
    ops.adamw_step(pd, gd, md, vd, 5, grad_scale=2.0, skip_flag=flag, **HYPER)
    for ts, bs in zip((pd, md, vd), before):
        assert all(np.array_equal(_bits(t), b) for t, b in zip(ts, bs))
    gd[35][4096] = 1.0
    assert _nonfinite(gd, flag) == 0
    ops.adamw_step(pd, gd, md, vd, 5, grad_scale=2.0, skip_flag=flag, **HYPER)
    changed = [not np.array_equal(_bits(t), b) for t, b in zip(pd, before[0])]
    assert changed == [i not in NONE_AT for i in range(N)]


# ------------------------------------------------------------------------------------------------ the optimiser
def _params(arrays):
    return [torch.nn.Parameter(t) for t in _upload(arrays)]


def _set_grads(params, arrays):
    for p, g in zip(params, _upload(arrays)):
        p.grad = g


def test_hip_adamw_parameters_at_different_steps_match_the_reference():
    """Entries 20 and 31 get no gradient on the first step: on the second their counter is 1, the others' 2, and the optimiser
    sends them out as separate launches with their own bias corrections."""
    from dg_tta_amd.optim import HipAdamW
    rng = np.random.RandomState(50)
    p0 = _normals(rng)
    params = _params(p0)
    opt = HipAdamW(params, **HYPER)
    steps = [0] * N
    for it, g in enumerate((_with_none(_normals(rng)), _normals(rng))):
        p_in = _host([p.data for p in params])
        m_in = [np.zeros(n) if "exp_avg" not in opt.state[p] else opt.state[p]["exp_avg"].cpu().numpy().astype(np.float64)
                for p, n in zip(params, _shapes())]
        v_in = [np.zeros(n) if "exp_avg_sq" not in opt.state[p] else opt.state[p]["exp_avg_sq"].cpu().numpy().astype(np.float64)
                for p, n in zip(params, _shapes())]
        _set_grads(params, g)
        opt.step()
        opt.zero_grad(set_to_none=True)
        steps = [s + (gi is not None) for s, gi in zip(steps, g)]
        assert [int(opt.state[p]["step"]) if opt.state[p] else 0 for p in params] == steps
        have = [i for i in range(N) if steps[i] > 0]
        md = [opt.state[params[i]]["exp_avg"] for i in have]
        vd = [opt.state[params[i]]["exp_avg_sq"] for i in have]
        sel = lambda xs: [xs[i] for i in have]
        scal = {s: adamw_ref.kernel_scalars(s, HYPER["lr"], *HYPER["betas"], HYPER["eps"], HYPER["weight_decay"]) for s in (1, 2)}
        wp, wm, wv = _worst(sel(p_in), sel(g), sel(m_in), sel(v_in), [params[i].data for i in have], md, vd,
                            lambda k: scal[steps[have[k]]])
        print(f"\nHipAdamW step {it + 1}: error / bound p {wp:.3f}, m {wm:.3f}, v {wv:.3f}")
        assert wp <= 1.0 and wm <= 1.0 and wv <= 1.0
        for i in range(N):
            if g[i] is None:
                assert np.array_equal(params[i].detach().cpu().numpy(), p_in[i].astype(np.float32)) and not opt.state[params[i]]
    assert steps == [1 if i in NONE_AT else 2 for i in range(N)]
    assert scal[1] != scal[2]


def test_hip_adamw_state_dict_interchanges_with_torch_adamw():
    from dg_tta_amd.optim import HipAdamW
    rng = np.random.RandomState(60)
    take = [0, 1, 2, 5, 7, 33]                                            # 1, 255, 256, 4097, 70 001, 8192 (misaligned) elements
    sub = lambda arrs: [arrs[i] for i in take]
    p0 = sub(_normals(rng))
    g1, g2, g3 = (sub(_normals(rng, 0.1)) for _ in range(3))
    g1[2] = None                                                          # its counter stays one behind
    params = _params(p0)
    hip = HipAdamW(params, **HYPER)
    for g in (g1, g2):
        _set_grads(params, g)
        hip.step()
        hip.zero_grad(set_to_none=True)
    sd = hip.state_dict()
    assert set(sd["state"]) == set(range(6)) and all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    assert [int(sd["state"][i]["step"]) for i in range(6)] == [2, 2, 1, 2, 2, 2]
    # -> torch.optim.AdamW on the CPU: same state, and its next step is the reference's
    tparams = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    tadam = torch.optim.AdamW(tparams, lr=0.5)
    tadam.load_state_dict(copy.deepcopy(sd))
    grp = tadam.param_groups[0]
    assert (grp["lr"], tuple(grp["betas"]), grp["eps"], grp["weight_decay"]) == (1e-3, (0.9, 0.999), 1e-8, 1e-2)
    for i in range(6):
        assert torch.equal(tadam.state[tparams[i]]["exp_avg"], hip.state[params[i]]["exp_avg"].cpu())
        assert torch.equal(tadam.state[tparams[i]]["exp_avg_sq"], hip.state[params[i]]["exp_avg_sq"].cpu())
    for t, g in zip(tparams, g3):
        t.grad = torch.from_numpy(g.astype(np.float32))
    tadam.step()
    for i in range(6):
        (rp,), _, _ = adamw_ref.adamw_step(_host([params[i].data]), [g3[i]], _host([hip.state[params[i]]["exp_avg"]]),
                                           _host([hip.state[params[i]]["exp_avg_sq"]]), 2 if i == 2 else 3, **HYPER)
        np.testing.assert_allclose(tparams[i].detach().numpy(), rp, rtol=1e-5, atol=1e-6)
    # ... and back: a HipAdamW that loads torch's state continues exactly as the one that never stopped
    back_params = [torch.nn.Parameter(_upload([p.detach().cpu().numpy()])[0]) for p in params]
    pre = torch.optim.AdamW([torch.nn.Parameter(p.detach().cpu().clone()) for p in params], **HYPER)
    pre.load_state_dict(copy.deepcopy(sd))
    back = HipAdamW(back_params, lr=0.5)
    back.load_state_dict(copy.deepcopy(pre.state_dict()))
    _set_grads(params, g3)
    _set_grads(back_params, g3)
    hip.step()
    back.step()
    for a, b in zip(params, back_params):
        assert torch.equal(a.detach(), b.detach())
        assert int(hip.state[a]["step"]) == int(back.state[b]["step"])
        assert torch.equal(hip.state[a]["exp_avg"], back.state[b]["exp_avg"])
        assert torch.equal(hip.state[a]["exp_avg_sq"], back.state[b]["exp_avg_sq"])
