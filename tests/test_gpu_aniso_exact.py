"""GPU: the anisotropic conv kernels (dg_tta_amd/csrc/conv_aniso.hip and the class-masked weight-gradient and transposed-conv
paths it drives) bit for bit against float64 (tests/conv_ref.py), through the C ABI.

The method is tests/test_gpu_conv_exact.py's: operands from {-1, 0, 1} (bias, accumulate bases: small integers) make every product
and every fp32 partial sum an exact integer whatever the order, tile shape or slab reduction, and every output an integer its
storage format holds (test_conv_ref.py checks those conditions for the cases used here, on the CPU, and that the typical mistakes
- a mirrored axis, exchanged parity classes, a dropped border tap, D padding on a kd = 1 layer, exchanged strides - move some
integer).  So every integer-operand comparison below is torch.equal against float64.  Output buffers start as NaN (overwrite) or
as the integer base (accumulate); what a kernel must not write holds a sentinel and is compared bit for bit; operands are read
from channel slices of wider buffers whose other channels hold 5.0.

Every conv case runs with kd = 1 and 3 and all eight strides, which reaches every conva_mfma_kernel<T, tile, KD, SD, SH, SW> the
library instantiates (test_conv_ref.py, test_aniso_cases_reach_every_tile): the forward takes (KD, SD, SH, SW) as given with the
32-wide tile (SD = 1 only), the 16-wide and the 8-wide one under each of them; the data gradient runs <KD, 1, 1, 1> with each of
the three tiles, once per parity class (1 to 8 classes, blockIdx.z).

| entry point                | test                             | switches (DGTTA_*)                                 | dtypes         | cases (conv_ref.py)                                |
|----------------------------|----------------------------------|----------------------------------------------------|----------------|----------------------------------------------------|
| conv3d_fwd (+ fused stats) | test_forward                     | none                                               | fp32 bf16 fp16 | ANISO_CONV_CASES x kd x 8 strides                  |
|                            | test_forward_plain               | none (stats = NULL, bias = NULL)                   | fp32 bf16 fp16 | first case x kd, stride (2, 1, 2)                  |
| conv3d_dgrad               | test_data_gradient               | none                                               | fp32 bf16 fp16 | the same grid where strided extents are even       |
| conv3d_wgrad (+ db)        | test_weight_gradient             | WGRAD_TR=0, WGRAD_XCD=0, WGRAD_REDUCE_TAPS=0,      | fp32 bf16 fp16 | the same grid                                      |
|                            |                                  | WGRAD_TR8=0, WGRAD_UPW=1/2; kd 3 at stride (1,1,1) |                |                                                    |
|                            |                                  | also WGRAD_RING=0, WGRAD_FLAT=0 and both           |                |                                                    |
|                            | test_weight_gradient_no_db       | none (db = NULL)                                   | fp32 bf16 fp16 | second case, kd 1, stride (1, 2, 2)                |
| convT3d_s_fwd / _bwd       | test_transposed                  | bwd: WGRAD_TR=0, WGRAD_XCD=0                       | fp32 bf16 fp16 | ANISO_CONVT_CASES x 7 strides                      |
|                            | test_transposed_optional_outputs | none (dx = NULL; dw_t = db = NULL)                 | fp32 bf16 fp16 | first case, strides (1,2,2) and (2,1,2)            |
| all five                   | test_refusals_*                  | none                                               | fp32 bf16 fp16 | odd strided extents, Cout % 8 or 4, workspace - 1, |
|                            |                                  |                                                    |                | kd = 5, transposed stride (1, 1, 1)                |
| fwd / dgrad, real operands | test_real_operands               | none                                               | fp32 bf16 fp16 | first case x kd, strides (1,2,2) and (2,1,2)       |
| convT fwd / dx, real       | test_real_operands_transposed    | none                                               | fp32 bf16 fp16 | first transposed case, stride (1, 2, 2)            |
"""
import functools

import pytest
import torch

import conv_ref as cr
from conftest import reload_kernel_switches
from test_gpu_conv_exact import (DEV, DTYPES, SENTINEL, _back, _dev, _lib, _nan_stats, _ndiff, _p, _same, _st, _stats_sums, _untouched,
                                 _up, _within)

pytestmark = pytest.mark.gpu
UNSUPPORTED, WORKSPACE = -2, -3                  # DGTTA_ERR_UNSUPPORTED, DGTTA_ERR_WORKSPACE
FILL = 5.0                          # what the channels beside an operand's slice hold (a kernel that reads them is off)
SWITCHES = ["WGRAD_RING", "WGRAD_FLAT", "WGRAD_TR", "WGRAD_TR8", "WGRAD_UPW", "WGRAD_XCD", "WGRAD_REDUCE_TAPS", "WGRAD_F32_SPLIT",
            "CONVT_GEMM", "CONVT_WGRAD_ONEPASS", "CONV_ROWS", "CONV_RING", "CONV_S2", "DGRAD_S2_ALLCLS"]

GRID = [(c, kd, s) for c in cr.ANISO_CONV_CASES for kd in cr.ANISO_KDS for s in cr.ANISO_STRIDES]
GRAD_GRID = [g for g in GRID if cr.aniso_grads_defined(g[0], g[2])]
CONVT_GRID = [(c, s) for c in cr.ANISO_CONVT_CASES for s in cr.ANISO_CONVT_STRIDES]


def _id(g):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else f"k{v}" for v in g)


@pytest.fixture
def switches(monkeypatch):
    """set_(NAME=value, ...): exactly these DGTTA_* kernel switches, the rest of this file's unset; the library takes a fresh
    snapshot.  Teardown restores the environment and reloads, so no test leaves a switch behind."""
    def set_(**kw):
        for name in SWITCHES:
            monkeypatch.delenv("DGTTA_" + name, raising=False)
        for name, value in kw.items():
            assert name in SWITCHES
            monkeypatch.setenv("DGTTA_" + name, str(value))
        reload_kernel_switches()
    set_()
    yield set_
    monkeypatch.undo()
    reload_kernel_switches()


def _check(rc, what):
    from dg_tta_amd._lib import check
    check(rc, what)


def _kpack(w64, dts):
    """The [kd, 3, 3] weight images of dgtta_conv3d_kpack_weights (forward image | data-gradient image)."""
    dt, tdt, gran = DTYPES[dts]
    lib = _lib()
    cout, cin, kd = w64.shape[:3]
    cinp, coutp = _up(cin, gran), _up(cout, gran)
    nb = lib.dgtta_conv3d_kpacked_bytes(kd, cinp, coutp, dt)
    assert nb > 0
    wpack = torch.empty(nb, dtype=torch.uint8, device=DEV)
    w = _dev(w64, torch.float32).contiguous()
    _check(lib.dgtta_conv3d_kpack_weights(_p(w), _p(wpack), kd, 3, 3, cin, cout, cinp, coutp, dt, _st()), "kpack")
    return wpack, cinp, coutp


def _sliced(t64, dts, fill=FILL):
    """t64 [..., C] as the channel slice [g, g + C) of a buffer of g + up(C, g) + g channels (g: the channel granule, 32 bytes),
    every other channel - the pad channels up to the next 16 bytes included - holding `fill`.  Returns (buffer, slice, row length)."""
    _, tdt, gran = DTYPES[dts]
    C = t64.shape[-1]
    ld = gran + _up(C, gran) + gran
    buf = torch.full((*t64.shape[:-1], ld), fill, dtype=tdt, device=DEV)
    buf[..., gran:gran + C] = _dev(t64, tdt)
    return buf, buf[..., gran:gran + C], ld


def _upper_half(t64, dts, fill=FILL):
    """t64 [..., C] as the upper half of a [..., 2 C] buffer whose lower half holds `fill`."""
    tdt = DTYPES[dts][1]
    C = t64.shape[-1]
    buf = torch.full((*t64.shape[:-1], 2 * C), fill, dtype=tdt, device=DEV)
    buf[..., C:] = _dev(t64, tdt)
    return buf, buf[..., C:], 2 * C


def _fwd(x, ldx, wpack, bias, y, ldy, stats, case, chans, kd, stride, dt):
    B, cin, cout, D, H, W = case
    return _lib().dgtta_conv3d_fwd(_p(x), ldx, _p(wpack), _p(bias), _p(y), ldy, _p(stats), B, cin, cout, *chans, D, H, W, kd, *stride, dt,
                                   _st())


def _dgrad(dy, lddy, wpack, dx, lddx, case, chans, kd, stride, acc, dt):
    B, cin, cout, D, H, W = case
    return _lib().dgtta_conv3d_dgrad(_p(dy), lddy, _p(wpack), _p(dx), lddx, B, cin, cout, *chans, D, H, W, kd, *stride, acc, dt, _st())


def _wgrad(x, ldx, dy, lddy, dw, db, ws, nb, case, kd, stride, acc, dt, cout=None):
    B, cin, c_out, D, H, W = case
    return _lib().dgtta_conv3d_wgrad(_p(x), ldx, _p(dy), lddy, _p(dw), _p(db), _p(ws), nb, B, cin, cout or c_out, D, H, W, kd, *stride,
                                     acc, dt, _st())


def _wgrad_ws(case, kd, stride):
    nb = _lib().dgtta_conv3d_kwgrad_ws_bytes(*case, kd, *stride)
    assert nb > 0
    return torch.empty(nb, dtype=torch.uint8, device=DEV), nb


def _sums(y64, B, C):
    return y64.reshape(B, -1, C).sum(dim=1), (y64 ** 2).reshape(B, -1, C).sum(dim=1)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("case,kd,stride", GRID, ids=[_id(g) for g in GRID])
def test_forward(case, kd, stride, dts):
    """dgtta_conv3d_fwd with bias and fused InstanceNorm statistics, twice: y exact in the upper half of a [..., 2 Cout] buffer whose
    lower half keeps its sentinel; the per-tile partial sums, added up per (sample, channel), equal sum y and sum y^2 exactly (an
    unwritten or doubly indexed tile slot leaves a NaN in them); both runs equal."""
    dt, tdt, gran = DTYPES[dts]
    lib = _lib()
    B, cin, cout, D, H, W = case
    p = cr.aniso_conv_problem(case, kd, stride)
    od = p["od"]
    _, x, ldx = _sliced(p["x"], dts)
    bias = _dev(p["bias"], torch.float32)
    wpack, cinp, coutp = _kpack(p["w"], dts)
    ref0, ref1 = _sums(p["y"], B, cout)
    nstat = lib.dgtta_conv3d_stats_bytes(B, cout, *od)
    got = []
    for _ in range(2):
        ybuf = torch.full((B, *od, 2 * cout), SENTINEL, dtype=tdt, device=DEV)
        ybuf[..., cout:] = float("nan")
        stats = _nan_stats(nstat)
        _check(_fwd(x, ldx, wpack, bias, ybuf[..., cout:], 2 * cout, stats, case, (cinp, coutp), kd, stride, dt), f"fwd {case} k{kd} {stride}")
        assert _same(ybuf[..., cout:], p["y"]), f"forward: {_ndiff(ybuf[..., cout:], p['y'])}"
        assert _untouched(ybuf[..., :cout]), "the lower half of the output rows was written"
        s0, s1 = _stats_sums(stats, B, cout)
        assert torch.equal(s0, ref0), "fused statistics: sum y"
        assert torch.equal(s1, ref1), "fused statistics: sum y^2"
        # the header: tiles per sample; a tile holds at most 16 M-blocks of 32 voxels and at least one voxel
        nblk = int(_back(stats)[:1].view(torch.int64)[0])
        assert od[0] * od[1] * od[2] <= nblk * 512 and nblk <= od[0] * od[1] * od[2], f"tiles per sample: {nblk}"
        got.append((ybuf, stats))
    assert torch.equal(got[1][0], got[0][0]), "forward: run to run"
    n = 32 + B * nblk * cout * 2                                                    # header + the written partial sums
    assert torch.equal(got[1][1][:n].view(torch.int64), got[0][1][:n].view(torch.int64)), "fused statistics: run to run"


@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("kd", cr.ANISO_KDS)
def test_forward_plain(kd, dts):
    """stats = NULL and bias = NULL: the same kernels without the epilogue's extras, x and y dense."""
    dt, tdt, gran = DTYPES[dts]
    case, stride = cr.ANISO_CONV_CASES[0], (2, 1, 2)
    B, cin, cout, D, H, W = case
    p = cr.aniso_conv_problem(case, kd, stride)
    x = _dev(p["x"], tdt)
    wpack, cinp, coutp = _kpack(p["w"], dts)
    y = torch.full((B, *p["od"], cout), float("nan"), dtype=tdt, device=DEV)
    _check(_fwd(x, cin, wpack, None, y, cout, None, case, (cinp, coutp), kd, stride, dt), "fwd")
    ref = p["y"] - p["bias"]
    assert _same(y, ref), _ndiff(y, ref)


# ------------------------------------------------------------------------------------------------ data gradient
@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("case,kd,stride", GRAD_GRID, ids=[_id(g) for g in GRAD_GRID])
def test_data_gradient(case, kd, stride, dts):
    """dgtta_conv3d_dgrad, overwrite onto NaN and accumulate onto the integer base: dy read from the upper half of a wider buffer,
    dx written into a channel slice with sentinels on both sides.  The class without a tap (kd = 1, sd = 2: the odd planes) writes
    zeros in overwrite mode and leaves the base alone when accumulating."""
    dt, tdt, gran = DTYPES[dts]
    B, cin, cout, D, H, W = case
    p = cr.aniso_conv_problem(case, kd, stride)
    _, dy, lddy = _upper_half(p["dy"], dts)
    wdpack, cinp, coutp = _kpack(p["wd"], dts)
    for acc, ref in ((0, p["dx"]), (1, p["dx"] + p["base"])):
        start = p["base"] if acc else torch.full_like(p["base"], float("nan"))
        dxbuf, dx, lddx = _sliced(start, dts, fill=SENTINEL)
        _check(_dgrad(dy, lddy, wdpack, dx, lddx, case, (cinp, coutp), kd, stride, acc, dt), f"dgrad {case} k{kd} {stride} acc {acc}")
        assert _same(dx, ref), f"data gradient, accumulate {acc}: {_ndiff(dx, ref)}"
        assert _untouched(dxbuf[..., :gran]) and _untouched(dxbuf[..., gran + cin:]), "channels beside the slice were written"
        if kd == 1 and stride[0] == 2:
            odd = dx[:, 1::2].double()
            want = _dev(p["base"], torch.float64)[:, 1::2] if acc else torch.zeros_like(odd)
            assert torch.equal(odd, want), f"odd planes of a kd = 1, sd = 2 layer, accumulate {acc}"


# ------------------------------------------------------------------------------------------------ weight and bias gradient
def _wgrad_configs(kd, stride):
    """Every switch wgrad_launch_classes, the class-masked kernels (conv_wgrad_rows.hip) and the slab reduction read.  kd = 3 at
    stride (1, 1, 1) is the plain 27-tap problem, which also has the ring sweep and the flat kernel in front of them."""
    cfgs = [{}, dict(WGRAD_TR="0"), dict(WGRAD_XCD="0"), dict(WGRAD_REDUCE_TAPS="0"), dict(WGRAD_TR8="0"), dict(WGRAD_UPW="1"),
            dict(WGRAD_UPW="2"), dict(WGRAD_TR="0", WGRAD_XCD="0")]
    if kd == 3 and stride == (1, 1, 1):
        cfgs += [dict(WGRAD_RING="0"), dict(WGRAD_FLAT="0"), dict(WGRAD_RING="0", WGRAD_FLAT="0"),
                 dict(WGRAD_RING="0", WGRAD_FLAT="0", WGRAD_XCD="0"), dict(WGRAD_RING="0", WGRAD_FLAT="0", WGRAD_UPW="2"),
                 dict(WGRAD_RING="0", WGRAD_FLAT="0", WGRAD_REDUCE_TAPS="0")]
    return cfgs


@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("case,kd,stride", GRAD_GRID, ids=[_id(g) for g in GRAD_GRID])
def test_weight_gradient(case, kd, stride, dts, switches):
    """dgtta_conv3d_wgrad with db under every weight-gradient switch: overwrite onto NaN, accumulate onto the integer base.  x is a
    channel slice of a wider buffer (its pad channels are somebody else's data)."""
    dt, tdt, gran = DTYPES[dts]
    B, cin, cout, D, H, W = case
    p = cr.aniso_wgrad_problem(case, kd, stride)
    _, x, ldx = _sliced(p["x"], dts)
    dy = _dev(p["dy"], tdt)
    ref_w = [p["dw"].to(DEV), (p["dw"] + p["base_w"]).to(DEV)]
    ref_b = [p["db"].to(DEV), (p["db"] + p["base_b"]).to(DEV)]
    base_w, base_b = _dev(p["base_w"], torch.float32), _dev(p["base_b"], torch.float32)
    ws, nb = _wgrad_ws(case, kd, stride)
    bad = []
    for cfg in _wgrad_configs(kd, stride):
        switches(**cfg)
        for acc in (0, 1):
            dw = base_w.clone() if acc else torch.full((cout, cin, kd, 3, 3), float("nan"), device=DEV)
            db = base_b.clone() if acc else torch.full((cout,), float("nan"), device=DEV)
            _check(_wgrad(x, ldx, dy, cout, dw, db, ws, nb, case, kd, stride, acc, dt), f"wgrad {case} k{kd} {stride} {dts} {cfg}")
            if not _same(dw, ref_w[acc]):
                bad.append(f"dw {cfg} accumulate {acc}: {_ndiff(dw, ref_w[acc])}")
            if not _same(db, ref_b[acc]):
                bad.append(f"db {cfg} accumulate {acc}: {_ndiff(db, ref_b[acc])}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dts", list(DTYPES))
def test_weight_gradient_no_db(dts):
    dt, tdt, gran = DTYPES[dts]
    case, kd, stride = cr.ANISO_CONV_CASES[1], 1, (1, 2, 2)
    B, cin, cout, D, H, W = case
    p = cr.aniso_wgrad_problem(case, kd, stride)
    _, x, ldx = _sliced(p["x"], dts)
    dy = _dev(p["dy"], tdt)
    ws, nb = _wgrad_ws(case, kd, stride)
    dw = torch.full((cout, cin, kd, 3, 3), float("nan"), device=DEV)
    _check(_wgrad(x, ldx, dy, cout, dw, None, ws, nb, case, kd, stride, 0, dt), "wgrad, db = NULL")
    assert _same(dw, p["dw"]), _ndiff(dw, p["dw"])


# ------------------------------------------------------------------------------------------------ transposed conv, kernel = stride
def _convT_fwd(x, ldx, w, bias, out, ldo, case, stride, dt, ws=None, nb=None):
    lib = _lib()
    B, cin, cout, D, H, W = case
    if ws is None:
        nb = lib.dgtta_convT3d_s_fwd_ws_bytes(cin, cout, *stride, dt)
        assert nb > 0
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    return lib.dgtta_convT3d_s_fwd(_p(x), ldx, _p(w), _p(bias), _p(out), ldo, _p(ws), nb, B, cin, cout, D, H, W, *stride, dt, _st())


def _convT_bwd(x, ldx, dcat, lddo, w, dx, lddx, dw, db, ws, nb, case, stride, acc, dt):
    B, cin, cout, D, H, W = case
    return _lib().dgtta_convT3d_s_bwd(_p(x), ldx, _p(dcat), lddo, _p(w), _p(dx), lddx, _p(dw), _p(db), _p(ws), nb, B, cin, cout, D, H, W,
                                      *stride, acc, dt, _st())


def _convT_bwd_ws(case, stride):
    nb = _lib().dgtta_convT3d_s_bwd_ws_bytes(*case, *stride)
    assert nb > 0
    return torch.empty(nb, dtype=torch.uint8, device=DEV), nb


@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("case,stride", CONVT_GRID, ids=[_id(g) for g in CONVT_GRID])
def test_transposed(case, stride, dts, switches):
    """Forward into the first half of a concat buffer (the skip half untouched); dx, dw and db from the concat buffer's gradient,
    overwrite and accumulate (dx is overwritten in both), under the switches of the class-masked weight gradient."""
    dt, tdt, gran = DTYPES[dts]
    B, cin, cout, D, H, W = case
    sd, sh, sw = stride
    p = cr.aniso_convT_problem(case, stride)
    x, dcat = _dev(p["x"], tdt), _dev(p["dcat"], tdt)
    w, wd, bias = _dev(p["w"], torch.float32), _dev(p["wd"], torch.float32), _dev(p["bias"], torch.float32)
    cat = torch.full((B, sd * D, sh * H, sw * W, 2 * cout), SENTINEL, dtype=tdt, device=DEV)
    cat[..., :cout] = float("nan")
    _check(_convT_fwd(x, cin, w, bias, cat, 2 * cout, case, stride, dt), f"convT fwd {case} {stride} {dts}")
    assert _same(cat[..., :cout], p["out"]), f"out: {_ndiff(cat[..., :cout], p['out'])}"
    assert _untouched(cat[..., cout:]), "skip half touched"
    ws, nb = _convT_bwd_ws(case, stride)
    bad = []
    for cfg in ({}, dict(WGRAD_TR="0"), dict(WGRAD_XCD="0")):
        switches(**cfg)
        for acc in (0, 1):
            dx = torch.full((B, D, H, W, cin), float("nan"), dtype=tdt, device=DEV)
            dw = _dev(p["base_w"], torch.float32) if acc else torch.full((cin, cout, sd, sh, sw), float("nan"), device=DEV)
            db = _dev(p["base_b"], torch.float32) if acc else torch.full((cout,), float("nan"), device=DEV)
            # (dx uses wd, dw does not read the weights: one call serves both)
            _check(_convT_bwd(x, cin, dcat, 2 * cout, wd, dx, cin, dw, db, ws, nb, case, stride, acc, dt), f"convT bwd {case} {stride} {dts}")
            ref_w, ref_b = (p["dw"] + p["base_w"], p["db"] + p["base_b"]) if acc else (p["dw"], p["db"])
            for name, got, ref in (("dx", dx, p["dx"]), ("dw", dw, ref_w), ("db", db, ref_b)):
                if not _same(got, ref):
                    bad.append(f"{name} {cfg} accumulate {acc}: {_ndiff(got, ref)}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("stride", [(1, 2, 2), (2, 1, 2)])
def test_transposed_optional_outputs(stride, dts):
    """dx = NULL: dw and db alone; dw_t = NULL and db = NULL: dx alone.  What is asked for is exact either way."""
    dt, tdt, gran = DTYPES[dts]
    case = cr.ANISO_CONVT_CASES[0]
    B, cin, cout, D, H, W = case
    p = cr.aniso_convT_problem(case, stride)
    x, dcat, wd = _dev(p["x"], tdt), _dev(p["dcat"], tdt), _dev(p["wd"], torch.float32)
    ws, nb = _convT_bwd_ws(case, stride)
    dw = torch.full((cin, cout, *stride), float("nan"), device=DEV)
    db = torch.full((cout,), float("nan"), device=DEV)
    _check(_convT_bwd(x, cin, dcat, 2 * cout, wd, None, cin, dw, db, ws, nb, case, stride, 0, dt), "convT bwd, dx = NULL")
    assert _same(dw, p["dw"]) and _same(db, p["db"])
    dx = torch.full((B, D, H, W, cin), float("nan"), dtype=tdt, device=DEV)
    _check(_convT_bwd(x, cin, dcat, 2 * cout, wd, dx, cin, None, None, ws, nb, case, stride, 0, dt), "convT bwd, dw_t = db = NULL")
    assert _same(dx, p["dx"]), _ndiff(dx, p["dx"])


# ------------------------------------------------------------------------------------------------ refusals
def _marked(shape, tdt):
    """An output buffer with a pattern of its own (not one value: a partial write of the same value would hide) and its copy."""
    n = 1
    for s in shape:
        n *= s
    t = (torch.arange(n, device=DEV) % 13 - 6).to(tdt).reshape(shape)
    return t, t.clone()


def _refused(rc, code, outputs, what):
    torch.cuda.synchronize()
    assert rc == code, f"{what}: returned {rc}, expected {code} ({_lib().dgtta_last_error().decode(errors='replace')})"
    for name, (buf, before) in outputs.items():
        assert torch.equal(buf.view(torch.uint8), before.view(torch.uint8)), f"{what}: {name} was written by a refused call"


ODD = cr.ANISO_CONV_CASES[3]
ODD_REFUSED = [(kd, s) for kd in cr.ANISO_KDS for s in cr.ANISO_STRIDES if not cr.aniso_grads_defined(ODD, s)]


@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("kd,stride", ODD_REFUSED, ids=[_id(g) for g in ODD_REFUSED])
def test_refusals_odd_strided_extent(kd, stride, dts):
    """Data and weight gradient refuse an odd extent along a strided axis (the forward of the same layer runs: test_forward)."""
    dt, tdt, gran = DTYPES[dts]
    B, cin, cout, D, H, W = ODD
    p = cr.aniso_conv_problem(ODD, kd, stride)
    assert p["dx"] is None and len(ODD_REFUSED) == 14
    dy, x = _dev(p["dy"], tdt), _dev(p["x"], tdt)
    wdpack, cinp, coutp = _kpack(p["wd"], dts)
    for acc in (0, 1):
        out = dict(dx=_marked((B, D, H, W, cin), tdt))
        _refused(_dgrad(dy, cout, wdpack, out["dx"][0], cin, ODD, (cinp, coutp), kd, stride, acc, dt), UNSUPPORTED, out, f"dgrad acc {acc}")
        assert b"even input extents" in _lib().dgtta_last_error()
        out = dict(dw=_marked((cout, cin, kd, 3, 3), torch.float32), db=_marked((cout,), torch.float32))
        ws, nb = _wgrad_ws(ODD, kd, stride)
        _refused(_wgrad(x, cin, dy, cout, out["dw"][0], out["db"][0], ws, nb, ODD, kd, stride, acc, dt), UNSUPPORTED, out, f"wgrad acc {acc}")
        assert b"even input extents" in _lib().dgtta_last_error()


@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("kd,stride", [(1, (1, 1, 1)), (3, (1, 2, 2)), (3, (1, 1, 1))], ids=["k1-1x1x1", "k3-1x2x2", "k3-1x1x1"])
def test_refusals_wgrad_cout_and_workspace(kd, stride, dts):
    """The weight gradient reads dy in whole 16-byte groups: Cout not a multiple of 8 (16-bit storage) / 4 (fp32) is refused; a
    workspace one byte short is DGTTA_ERR_WORKSPACE.  Neither writes dw or db."""
    dt, tdt, gran = DTYPES[dts]
    case = cr.ANISO_CONV_CASES[2]
    B, cin, cout, D, H, W = case
    p = cr.aniso_wgrad_problem(case, kd, stride)
    x, dy = _dev(p["x"], tdt), _dev(p["dy"], tdt)
    short = 6 if dts == "fp32" else 4                                                  # the first Cout channels of rows of 8
    assert short % (4 if dts == "fp32" else 8) and cout == 8
    ws, nb = _wgrad_ws(case, kd, stride)
    for acc in (0, 1):
        out = dict(dw=_marked((short, cin, kd, 3, 3), torch.float32), db=_marked((short,), torch.float32))
        _refused(_wgrad(x, cin, dy, cout, out["dw"][0], out["db"][0], ws, nb, case, kd, stride, acc, dt, cout=short), UNSUPPORTED, out,
                 f"wgrad Cout {short} acc {acc}")
        out = dict(dw=_marked((cout, cin, kd, 3, 3), torch.float32), db=_marked((cout,), torch.float32))
        _refused(_wgrad(x, cin, dy, cout, out["dw"][0], out["db"][0], ws, nb - 1, case, kd, stride, acc, dt), WORKSPACE, out,
                 f"wgrad workspace - 1 acc {acc}")
    # the same operands with the whole workspace are taken
    dw, db = torch.full((cout, cin, kd, 3, 3), float("nan"), device=DEV), torch.full((cout,), float("nan"), device=DEV)
    _check(_wgrad(x, cin, dy, cout, dw, db, ws, nb, case, kd, stride, 0, dt), "wgrad")
    assert _same(dw, p["dw"]) and _same(db, p["db"])


@pytest.mark.parametrize("dts", list(DTYPES))
def test_refusals_kernel_depth_5(dts):
    """kd = 5 is no layer of these kernels: forward, data gradient, weight gradient and the weight pack refuse it."""
    dt, tdt, gran = DTYPES[dts]
    lib = _lib()
    case, stride = cr.ANISO_CONV_CASES[2], (1, 1, 1)
    B, cin, cout, D, H, W = case
    p = cr.aniso_conv_problem(case, 3, stride)
    x, dy = _dev(p["x"], tdt), _dev(p["dy"], tdt)
    wpack, cinp, coutp = _kpack(p["w"], dts)
    assert lib.dgtta_conv3d_kpacked_bytes(5, cinp, coutp, dt) == 0 and lib.dgtta_conv3d_kwgrad_ws_bytes(*case, 5, *stride) == 0
    out = dict(y=_marked((B, D, H, W, cout), tdt), stats=_marked((lib.dgtta_conv3d_stats_bytes(B, cout, D, H, W) // 8,), torch.float64))
    _refused(_fwd(x, cin, wpack, None, out["y"][0], cout, out["stats"][0], case, (cinp, coutp), 5, stride, dt), UNSUPPORTED, out, "fwd kd 5")
    assert b"not supported" in lib.dgtta_last_error()
    out = dict(dx=_marked((B, D, H, W, cin), tdt))
    _refused(_dgrad(dy, cout, wpack, out["dx"][0], cin, case, (cinp, coutp), 5, stride, 0, dt), UNSUPPORTED, out, "dgrad kd 5")
    ws, nb = _wgrad_ws(case, 3, stride)
    out = dict(dw=_marked((cout, cin, 5, 3, 3), torch.float32), db=_marked((cout,), torch.float32))
    _refused(_wgrad(x, cin, dy, cout, out["dw"][0], out["db"][0], ws, nb, case, 5, stride, 0, dt), UNSUPPORTED, out, "wgrad kd 5")
    w5 = torch.zeros(cout, cin, 5, 3, 3, device=DEV)
    out = dict(wpack=_marked((wpack.numel(),), torch.uint8))
    _refused(lib.dgtta_conv3d_kpack_weights(_p(w5), _p(out["wpack"][0]), 5, 3, 3, cin, cout, cinp, coutp, dt, _st()), UNSUPPORTED, out,
             "kpack kd 5")


@pytest.mark.parametrize("dts", list(DTYPES))
def test_refusals_transposed(dts):
    """A transposed conv with stride (1, 1, 1) is no layer of a plan; a workspace one byte short is DGTTA_ERR_WORKSPACE."""
    dt, tdt, gran = DTYPES[dts]
    lib = _lib()
    case = cr.ANISO_CONVT_CASES[0]
    B, cin, cout, D, H, W = case
    p = cr.aniso_convT_problem(case, (1, 2, 2))
    x, wd = _dev(p["x"], tdt), _dev(p["wd"], torch.float32)
    assert lib.dgtta_convT3d_s_fwd_ws_bytes(cin, cout, 1, 1, 1, dt) == 0 and lib.dgtta_convT3d_s_bwd_ws_bytes(*case, 1, 1, 1) == 0
    ws, nb = _convT_bwd_ws(case, (2, 2, 2))                                          # room enough for anything below

    def outs(stride):
        return dict(dx=_marked((B, D, H, W, cin), tdt), dw=_marked((cin, cout, *stride), torch.float32), db=_marked((cout,), torch.float32))

    one = (1, 1, 1)
    out = dict(cat=_marked((B, D, H, W, 2 * cout), tdt))
    _refused(_convT_fwd(x, cin, wd, None, out["cat"][0], 2 * cout, case, one, dt, ws, nb), UNSUPPORTED, out, "convT fwd (1,1,1)")
    dcat1 = torch.zeros((B, D, H, W, 2 * cout), dtype=tdt, device=DEV)
    out = outs(one)
    _refused(_convT_bwd(x, cin, dcat1, 2 * cout, wd, out["dx"][0], cin, out["dw"][0], out["db"][0], ws, nb, case, one, 0, dt), UNSUPPORTED,
             out, "convT bwd (1,1,1)")
    s = (1, 2, 2)
    dcat = _dev(p["dcat"], tdt)
    nf = lib.dgtta_convT3d_s_fwd_ws_bytes(cin, cout, *s, dt)
    out = dict(cat=_marked((B, D, 2 * H, 2 * W, 2 * cout), tdt))
    _refused(_convT_fwd(x, cin, wd, None, out["cat"][0], 2 * cout, case, s, dt, ws, nf - 1), WORKSPACE, out, "convT fwd workspace - 1")
    nbw = lib.dgtta_convT3d_s_bwd_ws_bytes(*case, *s)
    out = outs(s)
    _refused(_convT_bwd(x, cin, dcat, 2 * cout, wd, out["dx"][0], cin, out["dw"][0], out["db"][0], ws, nbw - 1, case, s, 0, dt), WORKSPACE,
             out, "convT bwd workspace - 1")


# ------------------------------------------------------------------------------------------------ real-valued operands
@functools.lru_cache(maxsize=None)
def _real_problem(case, kd, stride, dts):
    """randn operands rounded to the storage type, their float64 results, sum |a b| and the number of products per output element
    (the operator applied to all-ones operands: the largest count over the elements)."""
    tdt = DTYPES[dts][1]
    B, cin, cout, D, H, W = case
    g = torch.Generator().manual_seed(sum(case) + 10 * kd + cr._stride_code(stride))
    od = cr.aniso_out_dims((D, H, W), kd, stride)
    rnd = lambda t: t.to(tdt).double()                                            # noqa: E731  (what the kernels store)
    x = rnd(torch.randn(B, D, H, W, cin, generator=g))
    w = rnd(torch.randn(cout, cin, kd, 3, 3, generator=g) / (9 * kd * cin) ** 0.5)
    bias = torch.randn(cout, generator=g).double()
    dy = rnd(torch.randn(B, *od, cout, generator=g))
    base = rnd(torch.randn(B, D, H, W, cin, generator=g))
    n_fwd = int(cr.conva_fwd(torch.ones_like(x), torch.ones_like(w), None, stride).max())
    n_dgrad = int(cr.conva_dgrad(torch.ones_like(dy), torch.ones_like(w), (D, H, W), stride).max())
    return dict(x=x, w=w, bias=bias, dy=dy, base=base, od=od, n_fwd=n_fwd, n_dgrad=n_dgrad, y=cr.conva_fwd(x, w, bias, stride),
                y_abs=cr.abs_bound(cr.conva_fwd, x, w, bias, stride=stride), dx=cr.conva_dgrad(dy, w, (D, H, W), stride),
                dx_abs=cr.abs_bound(cr.conva_dgrad, dy, w, (D, H, W), stride=stride))


@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("stride", [(1, 2, 2), (2, 1, 2)], ids=["1x2x2", "2x1x2"])
@pytest.mark.parametrize("kd", cr.ANISO_KDS)
def test_real_operands(kd, stride, dts):
    """randn operands rounded to the storage type: forward and data gradient, element by element, within the derived worst-case
    bound of fp32 summation against float64 (test_gpu_conv_exact._within, no added factor)."""
    dt, tdt, gran = DTYPES[dts]
    case = cr.ANISO_CONV_CASES[0]
    B, cin, cout, D, H, W = case
    p = _real_problem(case, kd, stride, dts)
    assert p["n_fwd"] == 9 * kd * cin and cout <= p["n_dgrad"] <= 9 * kd * cout
    xd, dyd, biasd = _dev(p["x"], tdt), _dev(p["dy"], tdt), _dev(p["bias"], torch.float32)
    wpack, cinp, coutp = _kpack(p["w"], dts)
    y = torch.full((B, *p["od"], cout), float("nan"), dtype=tdt, device=DEV)
    _check(_fwd(xd, cin, wpack, biasd, y, cout, None, case, (cinp, coutp), kd, stride, dt), "fwd")
    _within(_back(y), p["y"], p["y_abs"], p["n_fwd"], dts, f"aniso k{kd} s{stride} {dts} forward")
    for acc in (0, 1):
        dx = _dev(p["base"], tdt) if acc else torch.full((B, D, H, W, cin), float("nan"), dtype=tdt, device=DEV)
        _check(_dgrad(dyd, cout, wpack, dx, cin, case, (cinp, coutp), kd, stride, acc, dt), "dgrad")
        _within(_back(dx), p["dx"] + p["base"] * acc, p["dx_abs"] + p["base"].abs() * acc, p["n_dgrad"] + acc, dts,
                f"aniso k{kd} s{stride} {dts} dgrad acc {acc}")


@pytest.mark.parametrize("dts", list(DTYPES))
def test_real_operands_transposed(dts):
    """The same bound for the transposed conv's forward (Cin products and the bias) and data gradient (sd sh sw Cout products), read
    from / written into the concat buffer's first half."""
    dt, tdt, gran = DTYPES[dts]
    case, stride = cr.ANISO_CONVT_CASES[0], (1, 2, 2)
    B, cin, cout, D, H, W = case
    sd, sh, sw = stride
    g = torch.Generator().manual_seed(sum(case) + 1)
    rnd = lambda t: t.to(tdt).double()                                            # noqa: E731
    x = rnd(torch.randn(B, D, H, W, cin, generator=g))
    w = rnd(torch.randn(cin, cout, *stride, generator=g) / cin ** 0.5)
    bias = torch.randn(cout, generator=g).double()
    dcat = rnd(torch.randn(B, sd * D, sh * H, sw * W, 2 * cout, generator=g))
    dout = dcat[..., :cout]
    out_ref, out_abs = cr.convTa_fwd(x, w, bias), cr.abs_bound(cr.convTa_fwd, x, w, bias)
    dx_ref, dx_abs = cr.convTa_dgrad(dout, w), cr.abs_bound(cr.convTa_dgrad, dout, w)
    n_fwd = int(cr.convTa_fwd(torch.ones_like(x), torch.ones_like(w)).max())
    n_dgrad = int(cr.convTa_dgrad(torch.ones_like(dout), torch.ones_like(w)).max())
    assert n_fwd == cin and n_dgrad == sd * sh * sw * cout
    xd, dcatd, wd, biasd = _dev(x, tdt), _dev(dcat, tdt), _dev(w, torch.float32), _dev(bias, torch.float32)
    cat = torch.full((B, sd * D, sh * H, sw * W, 2 * cout), SENTINEL, dtype=tdt, device=DEV)
    _check(_convT_fwd(xd, cin, wd, biasd, cat, 2 * cout, case, stride, dt), "convT fwd")
    _within(_back(cat)[..., :cout], out_ref, out_abs, n_fwd, dts, f"aniso convT s{stride} {dts} forward")
    assert _untouched(cat[..., cout:])
    dx = torch.full((B, D, H, W, cin), float("nan"), dtype=tdt, device=DEV)
    ws, nb = _convT_bwd_ws(case, stride)
    _check(_convT_bwd(xd, cin, dcatd, 2 * cout, wd, dx, cin, None, None, ws, nb, case, stride, 0, dt), "convT bwd")
    _within(_back(dx), dx_ref, dx_abs, n_dgrad, dts, f"aniso convT s{stride} {dts} dgrad")
