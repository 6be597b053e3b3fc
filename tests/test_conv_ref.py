"""Host test of tests/conv_ref.py, the float64 restatement the exact GPU tests of the conv kernels are measured against.
(a) its operators against torch.nn.functional + autograd in float64 on real data; (b) the magnitude conditions under which
integer operands make every kernel exact, for every case tests/test_gpu_conv_exact.py runs (conditions, not measurements:
a case that breaks one gets another seed or density, never another limit); (c) the exact compare is sensitive - the typical
kernel mistakes (mirrored taps, a dropped tap at a border voxel, swapped channels, the ragged last column taken for padding,
a skipped stride-2 parity class), applied to the reference, change at least one output integer on those operands.
The same three sections for the anisotropic operators (conva_*, convTa_*) and the cases tests/test_gpu_aniso_exact.py runs, with the
mistakes of their own: taps mirrored along one axis, the taps of two parity classes exchanged, D padding on a kd = 1 layer, the H and
W strides exchanged, the tap-less class of kd = 1 with sd = 2; and that the case list reaches every tile shape of dispatch_conva."""
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


# (B, Cin, Cout, D, H, W, kd, stride): both kd, every stride combination once, odd extents along strided axes, a single voxel
ANISO_AUTOGRAD = [(2, 5, 7, 6, 5, 9, 1, (1, 1, 1)), (1, 4, 3, 6, 8, 10, 3, (1, 2, 2)), (2, 3, 6, 7, 5, 9, 1, (2, 2, 2)),
                  (1, 4, 5, 5, 7, 6, 3, (2, 1, 2)), (1, 3, 4, 4, 9, 7, 1, (1, 1, 2)), (2, 2, 3, 7, 6, 5, 3, (2, 2, 1)),
                  (1, 5, 2, 3, 4, 11, 1, (2, 1, 1)), (1, 3, 3, 5, 5, 5, 3, (1, 2, 1)), (1, 6, 4, 1, 1, 1, 3, (2, 2, 2)),
                  (1, 6, 4, 1, 1, 1, 1, (1, 1, 1)), (2, 4, 4, 8, 7, 9, 3, (1, 1, 1))]


@pytest.mark.parametrize("case", ANISO_AUTOGRAD)
def test_conva_matches_autograd_in_float64(case):
    B, cin, cout, D, H, W, kd, s = case
    g = torch.Generator().manual_seed(sum(case[:7]) + sum(s))
    x = torch.randn(B, cin, D, H, W, generator=g, dtype=torch.float64).requires_grad_()
    w = torch.randn(cout, cin, kd, 3, 3, generator=g, dtype=torch.float64).requires_grad_()
    b = torch.randn(cout, generator=g, dtype=torch.float64).requires_grad_()
    y = F.conv3d(x, w, b, stride=s, padding=(kd // 2, 1, 1))
    assert tuple(y.shape[2:]) == cr.aniso_out_dims((D, H, W), kd, s)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    _close(cr.conva_fwd(_cl(x), w.detach(), b.detach(), s), _cl(y), "y")
    _close(cr.conva_dgrad(_cl(dy), w.detach(), (D, H, W), s), _cl(x.grad), "dx")
    _close(cr.conva_wgrad(_cl(x), _cl(dy), kd, s), w.grad, "dw")
    _close(cr.conva_dbias(_cl(dy)), b.grad, "db")
    bound = cr.abs_bound(cr.conva_fwd, _cl(x), w.detach(), b.detach(), stride=s)
    assert bool((bound >= _cl(y).abs() * (1 - REL)).all())
    _close(bound, _cl(F.conv3d(x.detach().abs(), w.detach().abs(), b.detach().abs(), stride=s, padding=(kd // 2, 1, 1))), "abs bound")
    _close(cr.abs_bound(cr.conva_wgrad, _cl(x), _cl(dy), kd, stride=s), cr.conva_wgrad(_cl(x).abs(), _cl(dy).abs(), kd, s), "abs bound dw")
    if kd == 3 and s[0] == s[1] == s[2]:                 # where both exist the new operators restate the old ones
        assert torch.equal(cr.conva_fwd(_cl(x), w.detach(), b.detach(), s), cr.conv3_fwd(_cl(x), w.detach(), b.detach(), s[0]))
        assert torch.equal(cr.conva_dgrad(_cl(dy), w.detach(), (D, H, W), s), cr.conv3_dgrad(_cl(dy), w.detach(), (D, H, W), s[0]))
        assert torch.equal(cr.conva_wgrad(_cl(x), _cl(dy), kd, s), cr.conv3_wgrad(_cl(x), _cl(dy), s[0]))


@pytest.mark.parametrize("stride", cr.ANISO_CONVT_STRIDES)
@pytest.mark.parametrize("case", [(2, 5, 7, 3, 4, 5), (1, 8, 3, 1, 2, 6)])
def test_convTa_matches_autograd_in_float64(case, stride):
    B, cin, cout, D, H, W = case
    g = torch.Generator().manual_seed(sum(case) + sum(stride))
    x = torch.randn(B, cin, D, H, W, generator=g, dtype=torch.float64).requires_grad_()
    w = torch.randn(cin, cout, *stride, generator=g, dtype=torch.float64).requires_grad_()
    b = torch.randn(cout, generator=g, dtype=torch.float64).requires_grad_()
    out = F.conv_transpose3d(x, w, b, stride=stride)
    dout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(dout)
    _close(cr.convTa_fwd(_cl(x), w.detach(), b.detach()), _cl(out), "out")
    _close(cr.convTa_dgrad(_cl(dout), w.detach()), _cl(x.grad), "dx")
    _close(cr.convTa_wgrad(_cl(x), _cl(dout), stride), w.grad, "dw")
    _close(cr.conv3_dbias(_cl(dout)), b.grad, "db")
    _close(cr.abs_bound(cr.convTa_fwd, _cl(x), w.detach(), b.detach()), cr.convTa_fwd(_cl(x).abs(), w.detach().abs(), b.detach().abs()),
           "abs bound")


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


ANISO_GRID = [(c, kd, s) for c in cr.ANISO_CONV_CASES for kd in cr.ANISO_KDS for s in cr.ANISO_STRIDES]
ANISO_GRAD_GRID = [(c, kd, s) for c, kd, s in ANISO_GRID if cr.aniso_grads_defined(c, s)]
ANISO_CONVT_GRID = [(c, s) for c in cr.ANISO_CONVT_CASES for s in cr.ANISO_CONVT_STRIDES]


def _both_signs_many_values(t):
    """Not a degenerate draw: both signs and more distinct integers than a handful of ternary products could give."""
    return bool((t > 0).any()) and bool((t < 0).any()) and t.unique().numel() >= 9


@pytest.mark.parametrize("case,kd,stride", ANISO_GRID)
def test_preconditions_aniso_forward_and_data_gradient(case, kd, stride):
    p = cr.aniso_conv_problem(case, kd, stride)
    B, cin, cout = case[:3]
    assert _is_integer(p["y"]) and float(p["y"].abs().max()) <= cr.LIMIT_16BIT
    assert float((p["y"] ** 2).reshape(B, -1, cout).sum(dim=1).max()) < cr.LIMIT_F32
    assert float(cr.abs_bound(cr.conva_fwd, p["x"], p["w"], p["bias"], stride=stride).max()) < cr.LIMIT_F32
    assert _both_signs_many_values(p["y"])
    assert (p["dx"] is not None) == cr.aniso_grads_defined(case, stride)
    if p["dx"] is not None:
        assert _is_integer(p["dx"]) and float(p["dx"].abs().max()) <= cr.LIMIT_16BIT
        assert float((p["dx"] + p["base"]).abs().max()) <= cr.LIMIT_16BIT
        assert float(cr.abs_bound(cr.conva_dgrad, p["dy"], p["wd"], case[3:], stride=stride).max()) + cr.BASE_RANGE < cr.LIMIT_F32
        assert _both_signs_many_values(p["dx"])


@pytest.mark.parametrize("case,kd,stride", ANISO_GRAD_GRID)
def test_preconditions_aniso_weight_gradient(case, kd, stride):
    p = cr.aniso_wgrad_problem(case, kd, stride)
    assert _is_integer(p["dw"]) and _is_integer(p["db"])
    assert float(cr.abs_bound(cr.conva_wgrad, p["x"], p["dy"], kd, stride=stride).max()) + cr.BASE_RANGE < cr.LIMIT_F32
    assert float(p["dy"].abs().sum(dim=(0, 1, 2, 3)).max()) + cr.BASE_RANGE < cr.LIMIT_F32
    assert _both_signs_many_values(p["dw"]) and bool((p["db"] != 0).any())
    for t in range(kd * 9):                                                          # every tap's slice of dw carries something
        assert bool((p["dw"].reshape(*p["dw"].shape[:2], -1)[..., t] != 0).any())


def test_aniso_grad_grid_is_what_the_table_says():
    """The odd case runs its gradients at stride (1, 1, 1) only, every other case everywhere."""
    odd = cr.ANISO_CONV_CASES[3]
    assert [s for c, kd, s in ANISO_GRAD_GRID if c == odd and kd == 1] == [(1, 1, 1)]
    assert len(ANISO_GRAD_GRID) == 4 * 2 * 8 + 2 and len(ANISO_GRID) == 5 * 2 * 8


@pytest.mark.parametrize("case,stride", ANISO_CONVT_GRID)
def test_preconditions_aniso_transposed_conv(case, stride):
    p = cr.aniso_convT_problem(case, stride)
    cout = case[2]
    for k in ("out", "dx", "dw", "db"):
        assert _is_integer(p[k])
    assert float(p["out"].abs().max()) <= cr.LIMIT_16BIT and float(p["dx"].abs().max()) <= cr.LIMIT_16BIT
    assert float(cr.abs_bound(cr.convTa_fwd, p["x"], p["w"], p["bias"]).max()) < cr.LIMIT_F32
    assert float(cr.abs_bound(cr.convTa_dgrad, p["dcat"][..., :cout], p["wd"]).max()) < cr.LIMIT_F32
    assert float(cr.abs_bound(cr.convTa_wgrad, p["x"], p["dcat"][..., :cout], stride).max()) + cr.BASE_RANGE < cr.LIMIT_F32
    assert float(p["dcat"].abs().sum(dim=(0, 1, 2, 3)).max()) + cr.BASE_RANGE < cr.LIMIT_F32
    assert _both_signs_many_values(p["out"]) and _both_signs_many_values(p["dx"]) and _both_signs_many_values(p["dw"])


def test_aniso_convT_cases_are_what_the_issue_asks():
    assert len(cr.ANISO_CONVT_STRIDES) == 7 and (1, 1, 1) not in cr.ANISO_CONVT_STRIDES
    assert any(c[0] == 2 and c[1] % 32 for c in cr.ANISO_CONVT_CASES)


def _aniso_tile(wo, sd):
    """dispatch_conva of conv_aniso.hip restated: the output tile (TD, TH, TW) from the output row length and the D stride."""
    if sd == 1 and wo >= 32:
        return 4, 4, 32
    return (4, 4, 16) if wo >= 16 else (4, 8, 8)


def _aniso_tiles(case, kd, stride):
    """(tile width, workgroups along x of the forward launch)."""
    od = cr.aniso_out_dims(case[3:], kd, stride)
    t = _aniso_tile(od[2], stride[0])
    return t[2], case[0] * -(-od[0] // t[0]) * -(-od[1] // t[1]) * -(-od[2] // t[2])


def test_aniso_cases_reach_every_tile():
    """The case list reaches what its table claims: each tile width under each D stride that has it, both branches of the XCD
    swizzle (tile count a multiple of 8 or not), under both kd."""
    for kd in cr.ANISO_KDS:
        seen = {(s[0], _aniso_tiles(c, kd, s)[0]) for c, k, s in ANISO_GRID if k == kd}
        assert seen == {(1, 32), (1, 16), (1, 8), (2, 16), (2, 8)}
        counts = [_aniso_tiles(c, kd, s)[1] for c, k, s in ANISO_GRID if k == kd]
        assert any(n % 8 == 0 for n in counts) and any(n % 8 for n in counts)
        # and every tile width under every stride that has it: all conva_mfma_kernel<T, tile, KD, SD, SH, SW> the library instantiates
        reached = {(s, _aniso_tiles(c, kd, s)[0]) for c, k, s in ANISO_GRID if k == kd}
        assert reached == {(s, t) for s in cr.ANISO_STRIDES for t in (32, 16, 8) if t < 32 or s[0] == 1}
    assert _aniso_tiles(cr.ANISO_CONV_CASES[0], 3, (1, 1, 1)) == (32, 18)
    assert _aniso_tiles(cr.ANISO_CONV_CASES[1], 3, (1, 1, 1)) == (16, 40)
    assert _aniso_tiles(cr.ANISO_CONV_CASES[1], 1, (1, 1, 2)) == (8, 24)                   # Wo = 14
    assert _aniso_tiles(cr.ANISO_CONV_CASES[2], 1, (1, 1, 1))[0] == 8 and cr.ANISO_CONV_CASES[2][3] <= 4      # the 8-wide tile at sw = 1


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


def _parities(stride):
    return [(pd, ph, pw) for pd in range(stride[0]) for ph in range(stride[1]) for pw in range(stride[2])]


def _class_has_tap(par, kd, stride):
    """Does the parity class `par` of dx receive a tap?  Per axis, input index i = s vo + t - pad: t = i + pad (mod s) has a solution
    in [0, k) unless k = 1 and the parity is odd."""
    return all(any((t - k // 2 - p) % s == 0 for t in range(k)) for p, k, s in zip(par, (kd, 3, 3), stride))


@pytest.mark.parametrize("case,kd,stride", ANISO_GRID)
def test_exact_compare_is_sensitive_aniso(case, kd, stride):
    """The mistakes an anisotropic kernel can make, applied to the reference: each changes at least one output integer."""
    p = cr.aniso_conv_problem(case, kd, stride)
    B, cin, cout, D, H, W = case
    dims, od, pd = (D, H, W), p["od"], kd // 2
    x, w, bias, dy, wd, y, dx = p["x"], p["w"], p["bias"], p["dy"], p["wd"], p["y"], p["dx"]
    grads = dx is not None
    # the taps mirrored along ONE axis (kd = 1 has nothing to mirror along D)
    for ax in ((2, 3, 4) if kd == 3 else (3, 4)):
        assert not torch.equal(cr.conva_fwd(x, w.flip(ax), bias, stride), y), f"axis {ax}"
        if grads:
            assert not torch.equal(cr.conva_dgrad(dy, wd.flip(ax), dims, stride), dx), f"axis {ax}"
    # two input channels swapped (forward), two output channels swapped (the data gradient's K dimension)
    perm = list(range(cin))
    perm[0], perm[1] = perm[1], perm[0]
    assert not torch.equal(cr.conva_fwd(x[..., perm], w, bias, stride), y)
    permo = list(range(cout))
    permo[-1], permo[-2] = permo[-2], permo[-1]
    if grads:
        assert not torch.equal(cr.conva_dgrad(dy[..., permo], wd, dims, stride), dx)
    # one tap dropped at one border voxel: output voxel (0, 0, last) loses the tap that reads its left neighbour
    vw = od[2] - 1
    src_w = stride[2] * vw - 1
    assert bool((x[:, 0, 0, src_w] @ w[:, :, pd, 1, 0].t() != 0).any()), "the dropped tap contributes nothing here: pick another seed"
    if grads:
        assert bool((dy[:, 0, 0, vw] @ wd[:, :, pd, 1, 0] != 0).any())
    # the last (ragged) column taken for padding: some tap reads it whatever the stride (sw (Wo - 1) + 1 >= W - 1)
    assert stride[2] * vw + 1 >= W - 1
    x_cut = x.clone()
    x_cut[:, :, :, W - 1] = 0
    assert not torch.equal(cr.conva_fwd(x_cut, w, bias, stride), y)
    if grads:
        assert bool((dx[:, :, :, W - 1] != 0).any())
    # D padding applied to a kd = 1 layer: every output plane reads one plane too low
    if kd == 1:
        x_low = torch.cat([torch.zeros_like(x[:, :1]), x[:, :-1]], dim=1)
        assert not torch.equal(cr.conva_fwd(x_low, w, bias, stride), y)
    # the H and W strides exchanged (output extents as given, reads beyond the volume zero): the same rule on a volume with zeros behind it
    if stride[1] != stride[2]:
        x_big = torch.zeros(B, D, 2 * H + 2, 2 * W + 2, cin, dtype=x.dtype)
        x_big[:, :, :H, :W] = x
        y_ex = cr.conva_fwd(x_big, w, bias, (stride[0], stride[2], stride[1]))[:, :, :od[1], :od[2]]
        assert y_ex.shape == y.shape and not torch.equal(y_ex, y)
    if not grads:
        return
    # a parity class skipped: every class of dx that carries a tap holds a nonzero value; one without a tap (kd = 1, sd = 2, odd
    # planes) is exactly zero
    for par in _parities(stride):
        part = dx[:, par[0]::stride[0], par[1]::stride[1], par[2]::stride[2]]
        assert bool((part != 0).any()) == _class_has_tap(par, kd, stride), par
    if kd == 1 and stride[0] == 2:
        assert not bool(dx[:, 1::2].any()) and bool(dx[:, 0::2].any())
    # the weight taps of two parity classes exchanged: along a strided axis the even class takes tap 1, the odd one taps 0 and 2
    q = cr.aniso_wgrad_problem(case, kd, stride)
    for ax, s in zip((2, 3, 4), stride):
        if s == 2 and wd.shape[ax] == 3:
            swap = torch.tensor([1, 0, 2])
            assert not torch.equal(cr.conva_dgrad(dy, wd.index_select(ax, swap), dims, stride), dx), f"axis {ax}"
            assert not torch.equal(q["dw"].index_select(ax, swap), q["dw"]), f"axis {ax}"
            assert not torch.equal(q["dw"].flip(ax), q["dw"]), f"axis {ax}"


@pytest.mark.parametrize("case,stride", ANISO_CONVT_GRID)
def test_exact_compare_is_sensitive_aniso_transposed(case, stride):
    p = cr.aniso_convT_problem(case, stride)
    cin, cout = case[1:3]
    dout = p["dcat"][..., :cout]
    for ax, s in zip((2, 3, 4), stride):
        if s == 2:                                                                   # the offsets mirrored along one axis
            assert not torch.equal(cr.convTa_fwd(p["x"], p["w"].flip(ax), p["bias"]), p["out"])
            assert not torch.equal(cr.convTa_dgrad(dout, p["wd"].flip(ax)), p["dx"])
            assert not torch.equal(p["dw"].flip(ax), p["dw"])
    assert not torch.equal(cr.convTa_dgrad(p["dcat"][..., cout:], p["wd"]), p["dx"])        # the skip half read instead
    perm = list(range(cin))
    perm[0], perm[1] = perm[1], perm[0]
    assert not torch.equal(cr.convTa_fwd(p["x"][..., perm], p["w"], p["bias"]), p["out"])
    ref_nobias = p["out"] - p["bias"]
    for od, oh, ow in _parities(stride):                                             # an output offset skipped
        assert bool((ref_nobias[:, od::stride[0], oh::stride[1], ow::stride[2]] != 0).any())
        assert bool((p["dw"][:, :, od, oh, ow] != 0).any())
    if stride[1] != stride[2]:                                                       # the H and W strides exchanged: another shape altogether
        assert cr.convTa_fwd(p["x"], p["w"].transpose(3, 4), p["bias"]).shape != p["out"].shape
