"""Host test of tests/conv_ref.py, the float64 restatement the exact GPU tests of the conv kernels are measured against.
(a) its operators against torch.nn.functional + autograd in float64 on real data; (b) the magnitude conditions under which
integer operands make every kernel exact, for every case tests/test_gpu_conv_exact.py runs (conditions, not measurements:
a case that breaks one gets another seed or density, never another limit); (c) the exact compare is sensitive - the typical
kernel mistakes (mirrored taps, a dropped tap at a border voxel, swapped channels, the ragged last column taken for padding,
a skipped stride-2 parity class), applied to the reference, change at least one output integer on those operands."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as cr

REL = 1e-12


def _close(got, ref, what):
    err = float((got - ref).abs().max())
    lim = REL * float(ref.abs().max())
    assert got.shape == ref.shape and err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e}"


def _cl(t):          # NCDHW -> channels last
    return t.detach().permute(0, 2, 3, 4, 1).contiguous()


# ------------------------------------------------------------------------------------------------ (a) autograd
@pytest.mark.parametrize("case", [(2, 5, 7, 6, 5, 9, 1), (1, 4, 3, 6, 8, 10, 2), (2, 3, 6, 7, 5, 9, 2), (1, 6, 4, 1, 1, 1, 1)])
def test_conv3_matches_autograd_in_float64(case):
    B, cin, cout, D, H, W, s = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, cin, D, H, W, generator=g, dtype=torch.float64).requires_grad_()
    w = torch.randn(cout, cin, 3, 3, 3, generator=g, dtype=torch.float64).requires_grad_()
    b = torch.randn(cout, generator=g, dtype=torch.float64).requires_grad_()
    y = F.conv3d(x, w, b, stride=s, padding=1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    _close(cr.conv3_fwd(_cl(x), w.detach(), b.detach(), s), _cl(y), "y")
    _close(cr.conv3_dgrad(_cl(dy), w.detach(), (D, H, W), s), _cl(x.grad), "dx")
    _close(cr.conv3_wgrad(_cl(x), _cl(dy), s), w.grad, "dw")
    _close(cr.conv3_dbias(_cl(dy)), b.grad, "db")
    # abs_bound: the same operator on magnitudes = sum |a b|, an upper bound of |result| element by element
    bound = cr.abs_bound(cr.conv3_fwd, _cl(x), w.detach(), b.detach(), stride=s)
    assert bool((bound >= _cl(y).abs() * (1 - REL)).all())
    _close(bound, _cl(F.conv3d(x.detach().abs(), w.detach().abs(), b.detach().abs(), stride=s, padding=1)), "abs bound")


@pytest.mark.parametrize("case", [(2, 5, 7, 3, 4, 5), (1, 8, 3, 1, 2, 6)])
def test_convT_matches_autograd_in_float64(case):
    B, cin, cout, D, H, W = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, cin, D, H, W, generator=g, dtype=torch.float64).requires_grad_()
    w = torch.randn(cin, cout, 2, 2, 2, generator=g, dtype=torch.float64).requires_grad_()
    b = torch.randn(cout, generator=g, dtype=torch.float64).requires_grad_()
    out = F.conv_transpose3d(x, w, b, stride=2)
    dout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(dout)
    _close(cr.convT_fwd(_cl(x), w.detach(), b.detach()), _cl(out), "out")
    _close(cr.convT_dgrad(_cl(dout), w.detach()), _cl(x.grad), "dx")
    _close(cr.convT_wgrad(_cl(x), _cl(dout)), w.grad, "dw")
    _close(cr.conv3_dbias(_cl(dout)), b.grad, "db")


def test_gstats_sums_match_instnorm_ref():
    """(sum da, sum da y) against instnorm_ref.backward's S0 and S1 = (sum da y - mean sum da) rstd."""
    import instnorm_ref as iref
    B, V, C = 2, 45, 6
    g = torch.Generator().manual_seed(5)
    y = torch.randn(B, V, C, generator=g, dtype=torch.float64) * 1.5 + 0.3
    gz = torch.randn(B, V, C, generator=g, dtype=torch.float64)
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    mean, rstd = iref.stats(y, 1e-5)
    _, _, _, S0, S1 = iref.backward(gz, y, mean, rstd, gamma, beta, 0.01)
    s0, s1 = cr.gstats_sums(gz, y, mean, rstd, gamma, beta, 0.01)
    _close(s0, S0, "S0")
    assert float(((s1 - mean * s0) * rstd - S1).abs().max()) <= 1e-10 * float((gz * y).abs().sum(dim=1).max())


def test_ternary_draw():
    g = torch.Generator().manual_seed(1)
    t = cr.ternary((200, 300), 2.0 / 3, g)
    assert set(t.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert abs(float((t != 0).double().mean()) - 2.0 / 3) < 0.01 and abs(float(t.mean())) < 0.01
    d = cr.densities(320, 16)
    assert d["w_fwd"] == 0.1 and d["w_dgrad"] == 2.0 / 3 and d["x"] == d["dy"] == 2.0 / 3


# ------------------------------------------------------------------------------------------------ (b) preconditions
def _is_integer(t):
    return bool((t == t.round()).all())


@pytest.mark.parametrize("case,stride", cr.fwd_dgrad_cases())
def test_preconditions_forward_and_data_gradient(case, stride):
    p = cr.conv_problem(case, stride)
    B, cin, cout = case[:3]
    assert _is_integer(p["y"]) and _is_integer(p["dx"])
    assert float(p["y"].abs().max()) <= cr.LIMIT_16BIT                               # y with bias, as stored
    assert float(p["dx"].abs().max()) <= cr.LIMIT_16BIT
    assert float((p["dx"] + p["base"]).abs().max()) <= cr.LIMIT_16BIT                # after the accumulate base
    assert float((p["y"] ** 2).reshape(B, -1, cout).sum(dim=1).max()) < cr.LIMIT_F32        # fused statistics, whole sample
    # every fp32 partial sum is an integer of magnitude <= sum |a b| (+ |bias|), far below 2^24
    assert float(cr.abs_bound(cr.conv3_fwd, p["x"], p["w"], p["bias"], stride=stride).max()) < cr.LIMIT_F32
    assert p["y"].unique().numel() >= 30 and p["dx"].unique().numel() >= 30          # (not a degenerate draw)


@pytest.mark.parametrize("case,stride", [(c, 1) for c in cr.WGRAD_CASES] + [(c, 2) for c in cr.WGRAD_S2_CASES])
def test_preconditions_weight_gradient(case, stride):
    p = cr.wgrad_problem(case, stride)
    assert _is_integer(p["dw"]) and _is_integer(p["db"])
    assert float(cr.abs_bound(cr.conv3_wgrad, p["x"], p["dy"], stride=stride).max()) + cr.BASE_RANGE < cr.LIMIT_F32
    assert float(p["dy"].abs().sum(dim=(0, 1, 2, 3)).max()) + cr.BASE_RANGE < cr.LIMIT_F32
    assert p["dw"].abs().max() > 0 or case[3:] == (1, 1, 1)


@pytest.mark.parametrize("case", cr.CONVT_CASES)
def test_preconditions_transposed_conv(case):
    p = cr.convT_problem(case)
    for k in ("out", "dx", "dw", "db"):
        assert _is_integer(p[k])
    assert float(p["out"].abs().max()) <= cr.LIMIT_16BIT and float(p["dx"].abs().max()) <= cr.LIMIT_16BIT
    assert float(cr.abs_bound(cr.convT_wgrad, p["x"], p["dcat"][..., :case[2]]).max()) + cr.BASE_RANGE < cr.LIMIT_F32
    assert float(p["dcat"].abs().sum(dim=(0, 1, 2, 3)).max()) + cr.BASE_RANGE < cr.LIMIT_F32


@pytest.mark.parametrize("case", cr.GSTATS_RING_CASES + cr.GSTATS_ROWS_CASES)
def test_preconditions_fused_dgrad_sums(case):
    p = cr.gstats_problem(case)
    B, cin = case[:2]
    assert _is_integer(p["dx"]) and float(p["dx"].abs().max()) <= cr.LIMIT_16BIT
    a = p["gamma"] * (p["y_prev"] - 0.5)
    assert bool((a != 0).all()) and _is_integer(2 * a)                              # the pre-activation: exact, never 0
    assert set(p["gamma"].abs().unique().tolist()) <= {1.0, 2.0}
    # da is a multiple of 1/4: the sums in units of 1/4 are integers below 2^24 in any order of summation
    da_abs = p["dx"].abs().reshape(B, -1, cin)
    assert float((4 * da_abs * p["y_prev"].abs().reshape(B, -1, cin)).sum(dim=1).max()) < cr.LIMIT_F32
    assert float((4 * da_abs).sum(dim=1).max()) < cr.LIMIT_F32
    assert _is_integer(4 * p["s0"]) and _is_integer(4 * p["s1"])
    assert bool((p["s0"] != 0).any()) and bool((p["s1"] != 0).any())


# ------------------------------------------------------------------------------------------------ (c) sensitivity
@pytest.mark.parametrize("case,stride", cr.fwd_dgrad_cases())
def test_exact_compare_is_sensitive(case, stride):
    p = cr.conv_problem(case, stride)
    B, cin, cout, D, H, W = case
    x, w, bias, dy, wd = p["x"], p["w"], p["bias"], p["dy"], p["wd"]
    # the taps mirrored (forward weights used as the data gradient's, or the reverse)
    assert not torch.equal(cr.conv3_fwd(x, w.flip(2, 3, 4), bias, stride), p["y"])
    assert not torch.equal(cr.conv3_dgrad(dy, wd.flip(2, 3, 4), (D, H, W), stride), p["dx"])
    # two input channels swapped (forward), two output channels swapped (data gradient: its K dimension)
    perm = list(range(cin))
    perm[0], perm[1] = perm[1], perm[0]
    assert not torch.equal(cr.conv3_fwd(x[..., perm], w, bias, stride), p["y"])
    permo = list(range(cout))
    permo[-1], permo[-2] = permo[-2], permo[-1]
    assert not torch.equal(cr.conv3_dgrad(dy[..., permo], wd, (D, H, W), stride), p["dx"])
    # one tap dropped at one border voxel: the output voxel (0, 0, last) loses the tap that reads its left neighbour
    od = p["od"]
    if W > 1:
        vw = od[2] - 1
        src_w = stride * vw - 1                                          # tap (1, 1, 0) reads x[0, 0, s vw - 1]
        lost = x[:, 0, 0, src_w] @ w[:, :, 1, 1, 0].t()
        assert bool((lost != 0).any()), "the dropped tap contributes nothing here: pick another seed"
        lost_g = dy[:, 0, 0, vw] @ wd[:, :, 1, 1, 0]                    # the same tap in the data gradient: dx[0, 0, s vw - 1]
        assert bool((lost_g != 0).any())
    # the last (ragged) column treated as padding
    x_cut = x.clone()
    x_cut[:, :, :, W - 1] = 0
    if W > 1 and (stride == 1 or (W - 1) <= stride * (od[2] - 1) + 1):
        assert not torch.equal(cr.conv3_fwd(x_cut, w, bias, stride), p["y"])
    assert bool((p["dx"][:, :, :, W - 1] != 0).any())                    # a data gradient that skips it is wrong somewhere
    # a stride-2 parity class skipped: every one of the 8 classes of dx holds a nonzero integer
    if stride == 2:
        for pd in range(2):
            for ph in range(2):
                for pw in range(2):
                    assert bool((p["dx"][:, pd::2, ph::2, pw::2] != 0).any())


@pytest.mark.parametrize("case", cr.CONVT_CASES)
def test_exact_compare_is_sensitive_transposed(case):
    p = cr.convT_problem(case)
    cout = case[2]
    assert not torch.equal(cr.convT_fwd(p["x"], p["w"].flip(2, 3, 4), p["bias"]), p["out"])
    assert not torch.equal(cr.convT_dgrad(p["dcat"][..., :cout], p["wd"].flip(4)), p["dx"])
    assert not torch.equal(cr.convT_dgrad(p["dcat"][..., cout:], p["wd"]), p["dx"])      # the skip half read instead
    ref_nobias = p["out"] - p["bias"]
    for od in range(2):
        for oh in range(2):
            for ow in range(2):
                assert bool((ref_nobias[:, od::2, oh::2, ow::2] != 0).any())
