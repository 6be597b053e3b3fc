"""GPU: the 3x3x3 and 2x2x2 conv kernels bit for bit against float64 (tests/conv_ref.py), through the C ABI.

Operands from {-1, 0, 1} (bias, accumulate bases: small integers) make every product and every fp32 partial sum an exact
integer whatever the order, MFMA shape or slab reduction, and every output an integer its storage format holds
(test_conv_ref.py checks those conditions for the cases used here, on the CPU).  So every kernel - fp32 VALU, fp32 MFMA,
the six-product bf16 split, every 16-bit kernel - must EQUAL the float64 reference: all integer-operand comparisons below
are torch.equal.  A wrong tap, channel, halo voxel, tile edge, parity class, slab or accumulate path moves some integer
by at least 1 (test_conv_ref.py, "sensitive").  The data gradients meet a reference here that never went through
dgtta_conv3d_pack_weights.  The last two tests use real-valued operands with the worst-case bound of fp32 summation per element.

What the exact suite covers (register a new kernel or switch value here and in the matching list):

| entry point                 | test                            | switches (DGTTA_*)                                        | dtypes x impl             | cases (conv_ref.py)  |
|-----------------------------|---------------------------------|-----------------------------------------------------------|---------------------------|----------------------|
| conv3d_k3_fwd / _dgrad      | test_generic_tiles              | none (32x4x4, 16x4x4, 8x2x2 k1/k2, 8x2x8 tiles, VALU)     | fp32 bf16 fp16 x 1 2 0    | GENERIC_CASES        |
|                             | test_rows_kernel                | CONV_ROWS=1 CONV_RING=0, ROWS_ORDER=0/1                   | fp32 bf16 fp16 x 1 2 0    | ROWS_CASES           |
|                             | test_ring_kernel                | CONV_RING=1                                               | fp32 bf16 fp16 x 1 2 0    | RING_CASES           |
|                             | test_stride2                    | CONV_S2 unset/1/4; DGRAD_S2_ALLCLS=0/1 (even extents)     | fp32 bf16 fp16 x 1 2 0    | S2_CASES             |
|                             | test_stride2_odd_extent_dgrad   | none                                                      | fp32 bf16 fp16 x 0        | S2_ODD_DGRAD_CASE    |
|                             | test_strided_rows               | per group as above                                        | fp32 bf16 fp16 x 0        | first of each group  |
| conv3d_k3_wgrad (+ db)      | test_wgrad_stride1              | WGRAD_RING=0/1/4/6 (5: Cin <= 16), WGRAD_FLAT=0/1,        | fp32 (plain + split ws)   | WGRAD_CASES          |
|                             |                                 | WGRAD_TR=0/1, WGRAD_UPW=1/2/3                             | bf16 fp16 x 1 2 0         |                      |
|                             | test_wgrad_stride2              | WGRAD_S2_ONEPASS=0/1                                      | same                      | WGRAD_S2_CASES       |
| convT3d_k2s2_fwd / _bwd     | test_convT                      | CONVT_GEMM=0/1 x CONVT_WGRAD_ONEPASS=0/1                  | same                      | CONVT_CASES          |
| conv3d_k3_dgrad_gstats      | test_dgrad_gstats               | CONV_RING=1 | CONV_ROWS=1; IN_GSTATS=0; generic forced     | bf16 fp16 x 0             | GSTATS_*_CASES       |
| fwd / dgrad, real operands  | test_real_operands_within_bound | per group as above                                        | fp32 bf16 fp16 x 0 1 2    | first of each group  |
| convT fwd / dgrad, real     | test_real_operands_convT        | CONVT_GEMM=0/1                                            | fp32 bf16 fp16 x 0 1 2    | CONVT_CASES[0]       |
"""
import ctypes
import functools

import pytest
import torch

import conv_ref as cr
import instnorm_ref as iref
from conftest import reload_kernel_switches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNSUPPORTED = -2
SENTINEL = -7.0                     # fills what a kernel must not write (exact in every storage type)
DTYPES = {"fp32": (0, torch.float32, 8), "bf16": (1, torch.bfloat16, 16), "fp16": (2, torch.float16, 16)}      # code, type, channel granule
IMPLS = [1, 2, 0]                   # VALU, MFMA, the product's own choice
SWITCHES = ["CONV_ROWS", "CONV_RING", "ROWS_ORDER", "CONV_S2", "DGRAD_S2_ALLCLS", "WGRAD_RING", "WGRAD_FLAT", "WGRAD_TR", "WGRAD_UPW",
            "WGRAD_S2_ONEPASS", "WGRAD_F32_SPLIT", "WGRAD_REDUCE_TAPS", "CONVT_GEMM", "CONVT_WGRAD_ONEPASS", "IN_GSTATS"]


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


def _lib():
    from dg_tta_amd import _lib
    return _lib.load()


def _ok(rc, impl, what):
    """impl 2 may refuse a shape (that parameter is skipped, with the library's reason); anything else is an error."""
    from dg_tta_amd._lib import check
    if rc == UNSUPPORTED and impl == 2:
        pytest.skip(f"impl 2 refuses {what}: {_lib().dgtta_last_error().decode(errors='replace')}")
    check(rc, what)


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream(DEV).cuda_stream


def _up(c, g):
    return (c + g - 1) // g * g


def _dev(t64, tdt):
    return t64.to(tdt).to(DEV)


def _back(t):
    torch.cuda.synchronize()
    return t.detach().cpu().double()


def _same(got, ref64):
    """Bit equality with the float64 reference (every storage type widens exactly), compared on the device."""
    return torch.equal(got.double(), ref64.to(got.device))


def _ndiff(got, ref64):
    return f"{int((got.double() != ref64.to(got.device)).sum())} of {ref64.numel()} elements differ"


def _untouched(part):
    return bool((part == SENTINEL).all())


def _pack(w64, dts):
    dt, tdt, gran = DTYPES[dts]
    lib = _lib()
    cout, cin = w64.shape[:2]
    cinp, coutp = _up(cin, gran), _up(cout, gran)
    w = _dev(w64, torch.float32)
    wpack = torch.empty(lib.dgtta_conv3d_packed_bytes(cinp, coutp, dt) // (4 if dt == 0 else 2), dtype=tdt, device=DEV)
    from dg_tta_amd._lib import check
    check(lib.dgtta_conv3d_pack_weights(_p(w), _p(wpack), cin, cout, cinp, coutp, dt, _st()), "pack")
    return wpack, cinp, coutp


def _fwd(x, ldx, wpack, bias, y, ldy, stats, dims, chans, stride, dt, impl):
    B, D, H, W = dims
    cin, cout, cinp, coutp = chans
    return _lib().dgtta_conv3d_k3_fwd(_p(x), ldx, _p(wpack), _p(bias), _p(y), ldy, _p(stats), B, cin, cout, cinp, coutp, D, H, W,
                                      stride, dt, impl, _st())


def _dgrad(dy, lddy, wpack, dx, lddx, dims, chans, stride, acc, dt, impl):
    B, D, H, W = dims
    cin, cout, cinp, coutp = chans
    return _lib().dgtta_conv3d_k3_dgrad(_p(dy), lddy, _p(wpack), _p(dx), lddx, B, cin, cout, cinp, coutp, D, H, W, stride, acc, dt,
                                        impl, _st())


def _stats_sums(stats, B, C):
    """(sum over tiles of the first, of the second partial), each [B, C] float64, read with instnorm_ref.unpack_partials."""
    buf = _back(stats)
    nblk = int(buf[:iref.HEADER_DOUBLES].view(torch.int64)[0])
    assert 1 <= nblk and iref.HEADER_DOUBLES + B * nblk * C * 2 <= buf.numel(), f"tiles per sample: {nblk}"
    n, body = iref.unpack_partials(buf[:iref.HEADER_DOUBLES + B * nblk * C * 2], B, C)
    assert n == nblk
    return body[..., 0].sum(dim=1), body[..., 1].sum(dim=1)


def _nan_stats(nbytes):
    return torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=DEV)


def _exact_fwd_dgrad(case, stride, dts, impl, switches, fwd_env=None, dgrad_variants=((),)):
    """Forward with bias and fused statistics, data gradient with and without accumulation, each twice: bit equal to float64
    and run to run.  dgrad_variants: switch settings under which the data gradient is repeated (fwd_env + variant)."""
    dt, tdt, gran = DTYPES[dts]
    lib = _lib()
    B, cin, cout, D, H, W = case
    p = cr.conv_problem(case, stride)
    od = p["od"]
    fwd_env = fwd_env or {}
    switches(**fwd_env)
    x, bias = _dev(p["x"], tdt), _dev(p["bias"], torch.float32)
    wpack, cinp, coutp = _pack(p["w"], dts)
    chans = (cin, cout, cinp, coutp)
    ys = []
    for _ in range(2):
        y = torch.full((B, *od, cout), float("nan"), dtype=tdt, device=DEV)
        stats = _nan_stats(lib.dgtta_conv3d_stats_bytes(B, cout, *od))
        _ok(_fwd(x, cin, wpack, bias, y, cout, stats, (B, D, H, W), chans, stride, dt, impl), impl, f"fwd {case} s{stride} {dts}")
        ys.append(y)
        s0, s1 = _stats_sums(stats, B, cout)
        assert torch.equal(s0, p["y"].reshape(B, -1, cout).sum(dim=1)), "fused statistics: sum y"
        assert torch.equal(s1, (p["y"] ** 2).reshape(B, -1, cout).sum(dim=1)), "fused statistics: sum y^2"
    assert _same(ys[0], p["y"]), f"forward: {_ndiff(ys[0], p['y'])}"
    assert torch.equal(ys[1], ys[0]), "forward: run to run"

    dy = _dev(p["dy"], tdt)
    wdpack, _, _ = _pack(p["wd"], dts)
    for variant in dgrad_variants:
        switches(**{**fwd_env, **dict(variant)})
        for acc, ref in ((0, p["dx"]), (1, p["dx"] + p["base"])):
            got = []
            for _ in range(2):
                dx = _dev(p["base"], tdt) if acc else torch.full((B, D, H, W, cin), float("nan"), dtype=tdt, device=DEV)
                _ok(_dgrad(dy, cout, wdpack, dx, cin, (B, D, H, W), chans, stride, acc, dt, impl), impl,
                    f"dgrad {case} s{stride} {dts} acc {acc}")
                got.append(dx)
            what = f"data gradient, accumulate {acc}, {dict(variant)}"
            assert _same(got[0], ref), f"{what}: {_ndiff(got[0], ref)}"
            assert torch.equal(got[1], got[0]), f"{what}: run to run"


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("case", cr.GENERIC_CASES)
def test_generic_tiles(case, dts, impl, switches):
    """The generic MFMA tiles (32-wide ragged in all axes, 16-wide, 8x2x2 with one and two k-steps, 8x2x8) and the VALU kernels."""
    _exact_fwd_dgrad(case, 1, dts, impl, switches)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("order", ["0", "1"])
@pytest.mark.parametrize("case", cr.ROWS_CASES)
def test_rows_kernel(case, order, dts, impl, switches):
    """The persistent row-reuse kernel forced on (16-bit storage, impl 2 / 0; the other parameters run what the dispatch then picks)."""
    _exact_fwd_dgrad(case, 1, dts, impl, switches, dict(CONV_ROWS=1, CONV_RING=0, ROWS_ORDER=order))


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("case", cr.RING_CASES)
def test_ring_kernel(case, dts, impl, switches):
    """The D-ring kernel forced on: 32 and 64 input channels, ragged edges, batch > 1, more column jobs than CUs."""
    _exact_fwd_dgrad(case, 1, dts, impl, switches, dict(CONV_RING=1))


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("s2", [None, "1", "4"])
@pytest.mark.parametrize("case", cr.S2_CASES)
def test_stride2(case, s2, dts, impl, switches):
    """Stride 2: the register-operand kernel, the generic 8-wave and former 4-wave tiles; the data gradient as 8 parity-class
    launches and as the single all-classes pass."""
    env = {} if s2 is None else dict(CONV_S2=s2)
    _exact_fwd_dgrad(case, 2, dts, impl, switches, env,
                     dgrad_variants=((("DGRAD_S2_ALLCLS", "0"),), (("DGRAD_S2_ALLCLS", "1"),)))


@pytest.mark.parametrize("dts", list(DTYPES))
def test_stride2_odd_extent_dgrad(dts, switches):
    _exact_fwd_dgrad(cr.S2_ODD_DGRAD_CASE, 2, dts, 0, switches)


GROUP_FIRST = [("generic", cr.GENERIC_CASES[0], 1, {}), ("rows", cr.ROWS_CASES[0], 1, dict(CONV_ROWS=1, CONV_RING=0)),
               ("ring", cr.RING_CASES[0], 1, dict(CONV_RING=1)), ("stride2", cr.S2_CASES[0], 2, {})]


@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("group", GROUP_FIRST, ids=[g[0] for g in GROUP_FIRST])
def test_strided_rows(group, dts, switches):
    """Row strides wider than the channel count, as the U-Net's concat buffers have them: x is read from the upper half of a
    [..., 2 Cin] buffer, y written into the upper half of a [..., 2 Cout] buffer (and dy read from there), dx written into
    channels [CP, CP + Cin) of a wider buffer.  The rest of every row keeps its sentinel bit for bit; the written part is exact."""
    _, case, stride, env = group
    dt, tdt, gran = DTYPES[dts]
    B, cin, cout, D, H, W = case
    p = cr.conv_problem(case, stride)
    od = p["od"]
    switches(**env)
    lib = _lib()
    xbuf = torch.full((B, D, H, W, 2 * cin), 5.0, dtype=tdt, device=DEV)            # (a kernel that reads the wrong half is off)
    xbuf[..., cin:] = _dev(p["x"], tdt)
    wpack, cinp, coutp = _pack(p["w"], dts)
    chans = (cin, cout, cinp, coutp)
    bias = _dev(p["bias"], torch.float32)
    ybuf = torch.full((B, *od, 2 * cout), SENTINEL, dtype=tdt, device=DEV)
    stats = _nan_stats(lib.dgtta_conv3d_stats_bytes(B, cout, *od))
    _ok(_fwd(xbuf[..., cin:], 2 * cin, wpack, bias, ybuf[..., cout:], 2 * cout, stats, (B, D, H, W), chans, stride, dt, 0), 0, "fwd")
    assert _same(ybuf[..., cout:], p["y"]), _ndiff(ybuf[..., cout:], p["y"])
    assert _untouched(ybuf[..., :cout])
    s0, s1 = _stats_sums(stats, B, cout)
    assert torch.equal(s0, p["y"].reshape(B, -1, cout).sum(dim=1)) and torch.equal(s1, (p["y"] ** 2).reshape(B, -1, cout).sum(dim=1))

    CP, tail = 16, 8
    dybuf = torch.full((B, *od, 2 * cout), 5.0, dtype=tdt, device=DEV)
    dybuf[..., cout:] = _dev(p["dy"], tdt)
    wdpack, _, _ = _pack(p["wd"], dts)
    for acc, ref in ((0, p["dx"]), (1, p["dx"] + p["base"])):
        dxbuf = torch.full((B, D, H, W, CP + cin + tail), SENTINEL, dtype=tdt, device=DEV)
        if acc:
            dxbuf[..., CP:CP + cin] = _dev(p["base"], tdt)
        _ok(_dgrad(dybuf[..., cout:], 2 * cout, wdpack, dxbuf[..., CP:], CP + cin + tail, (B, D, H, W), chans, stride, acc, dt, 0), 0,
            "dgrad")
        assert _same(dxbuf[..., CP:CP + cin], ref), f"accumulate {acc}: {_ndiff(dxbuf[..., CP:CP + cin], ref)}"
        assert _untouched(dxbuf[..., :CP]) and _untouched(dxbuf[..., CP + cin:])


# ------------------------------------------------------------------------------------------------ weight and bias gradient
def _wgrad(x, ldx, dy, lddy, dw, db, dims, cin, cout, stride, acc, dt, impl, split):
    lib = _lib()
    B, D, H, W = dims
    od = [cr.out_extent(n, stride) for n in (D, H, W)]
    plain = lib.dgtta_conv3d_wgrad_ws_bytes(B, cin, cout, *od)
    nb = lib.dgtta_conv3d_wgrad_split_ws_bytes(B, cin, cout, *od, stride) if split else plain
    assert nb >= plain and (not split or nb > plain)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    return lib.dgtta_conv3d_k3_wgrad(_p(x), ldx, _p(dy), lddy, _p(dw), _p(db), _p(ws), nb, B, cin, cout, D, H, W, stride, acc, dt,
                                     impl, _st())


# (dtype, impl, split workspace): fp32 VALU / MFMA / the six-product bf16 split / auto (with the split workspace, as the U-Net offers it)
WGRAD_MODES = [("fp32", 1, False), ("fp32", 2, False), ("fp32", 2, True), ("fp32", 0, True), ("bf16", 1, False), ("bf16", 2, False),
               ("bf16", 0, False), ("fp16", 1, False), ("fp16", 2, False), ("fp16", 0, False)]
WGRAD_MODE_IDS = [f"{d}-impl{i}{'-split' if s else ''}" for d, i, s in WGRAD_MODES]


def _exact_wgrad(case, stride, mode, configs, switches):
    dts, impl, split = mode
    dt, tdt, gran = DTYPES[dts]
    B, cin, cout, D, H, W = case
    p = cr.wgrad_problem(case, stride)
    ld = _up(cin, 8)
    x = torch.full((B, D, H, W, ld), 3.0, dtype=tdt, device=DEV)                    # the pad channels of a row are somebody else's data
    x[..., :cin] = _dev(p["x"], tdt)
    dy = _dev(p["dy"], tdt)
    ref_w = [p["dw"].to(DEV), (p["dw"] + p["base_w"]).to(DEV)]                      # overwrite, accumulate
    ref_b = [p["db"].to(DEV), (p["db"] + p["base_b"]).to(DEV)]
    base_w, base_b = _dev(p["base_w"], torch.float32), _dev(p["base_b"], torch.float32)
    bad = []
    for cfg in (configs if impl != 1 else configs[:1]):                             # (the VALU kernel knows no switch)
        switches(**cfg)
        for acc in (0, 1):
            dw = base_w.clone() if acc else torch.full((cout, cin, 3, 3, 3), float("nan"), device=DEV)
            db = base_b.clone() if acc else torch.full((cout,), float("nan"), device=DEV)
            _ok(_wgrad(x, ld, dy, cout, dw, db, (B, D, H, W), cin, cout, stride, acc, dt, impl, split), impl,
                f"wgrad {case} s{stride} {dts} {cfg}")
            if not _same(dw, ref_w[acc]):
                bad.append(f"dw {cfg} accumulate {acc}: {_ndiff(dw, ref_w[acc])}")
            if not _same(db, ref_b[acc]):                                           # db against dy.sum in float64
                bad.append(f"db {cfg} accumulate {acc}: {_ndiff(db, ref_b[acc])}")
    assert not bad, "\n".join(bad)


def _wgrad_configs(cin):
    ring = ["0", "1", "4", "6"] + (["5"] if cin <= 16 else [])
    cfgs = [{}] + [dict(WGRAD_RING=r) for r in ring] + [dict(WGRAD_FLAT=f) for f in "01"] + [dict(WGRAD_TR=t) for t in "01"]
    cfgs += [dict(WGRAD_UPW=u) for u in "123"]
    # the predecessors below the ring sweep, each on its own: row kernels with and without the transposed read, several units per workgroup
    cfgs += [dict(WGRAD_RING="0", WGRAD_TR="0"), dict(WGRAD_RING="0", WGRAD_UPW="3"), dict(WGRAD_RING="0", WGRAD_TR="0", WGRAD_UPW="2"),
             dict(WGRAD_RING="0", WGRAD_FLAT="0"), dict(WGRAD_F32_SPLIT="0"), dict(WGRAD_REDUCE_TAPS="0")]
    return cfgs


@pytest.mark.parametrize("mode", WGRAD_MODES, ids=WGRAD_MODE_IDS)
@pytest.mark.parametrize("case", cr.WGRAD_CASES)
def test_wgrad_stride1(case, mode, switches):
    """dw and db of the stride-1 conv under every weight-gradient switch, overwrite and accumulate onto an integer base."""
    _exact_wgrad(case, 1, mode, _wgrad_configs(case[1]), switches)


@pytest.mark.parametrize("mode", WGRAD_MODES, ids=WGRAD_MODE_IDS)
@pytest.mark.parametrize("case", cr.WGRAD_S2_CASES)
def test_wgrad_stride2(case, mode, switches):
    _exact_wgrad(case, 2, mode, [{}, dict(WGRAD_S2_ONEPASS="0"), dict(WGRAD_S2_ONEPASS="1"), dict(WGRAD_F32_SPLIT="0")], switches)


# ------------------------------------------------------------------------------------------------ transposed conv (k2 s2)
@pytest.mark.parametrize("mode", WGRAD_MODES, ids=WGRAD_MODE_IDS)
@pytest.mark.parametrize("case", cr.CONVT_CASES)
def test_convT(case, mode, switches):
    """Forward into the first half of a concat buffer (the skip half untouched); dx, dw and db from the concat buffer's gradient."""
    dts, impl, split = mode
    dt, tdt, gran = DTYPES[dts]
    lib = _lib()
    B, cin, cout, D, H, W = case
    p = cr.convT_problem(case)
    x, dcat = _dev(p["x"], tdt), _dev(p["dcat"], tdt)
    w, wd, bias = _dev(p["w"], torch.float32), _dev(p["wd"], torch.float32), _dev(p["bias"], torch.float32)
    bad = []
    cfgs = [dict(CONVT_GEMM=g, CONVT_WGRAD_ONEPASS=o) for g in "01" for o in "01"] + [{}]
    for cfg in (cfgs if impl != 1 else cfgs[-1:]):
        switches(**cfg)
        cat = torch.full((B, 2 * D, 2 * H, 2 * W, 2 * cout), SENTINEL, dtype=tdt, device=DEV)
        nb = lib.dgtta_convT3d_fwd_ws_bytes(cin, cout, dt)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        _ok(lib.dgtta_convT3d_k2s2_fwd(_p(x), cin, _p(w), _p(bias), _p(cat), 2 * cout, _p(ws), nb, B, cin, cout, D, H, W, dt, impl, _st()),
            impl, f"convT fwd {case} {dts}")
        if not _same(cat[..., :cout], p["out"]):
            bad.append(f"out {cfg}: {_ndiff(cat[..., :cout], p['out'])}")
        if not _untouched(cat[..., cout:]):
            bad.append(f"skip half touched {cfg}")
        nb = (lib.dgtta_convT3d_bwd_split_ws_bytes if split else lib.dgtta_convT3d_bwd_ws_bytes)(B, cin, cout, D, H, W)
        ws2 = torch.empty(nb, dtype=torch.uint8, device=DEV)
        for acc in (0, 1):
            dx = torch.full((B, D, H, W, cin), float("nan"), dtype=tdt, device=DEV)                 # (overwritten in both modes)
            dw = _dev(p["base_w"], torch.float32) if acc else torch.full((cin, cout, 2, 2, 2), float("nan"), device=DEV)
            db = _dev(p["base_b"], torch.float32) if acc else torch.full((cout,), float("nan"), device=DEV)
            # (dx uses wd, dw does not read the weights: one call serves both)
            _ok(lib.dgtta_convT3d_k2s2_bwd(_p(x), cin, _p(dcat), 2 * cout, _p(wd), _p(dx), cin, _p(dw), _p(db), _p(ws2), nb, B, cin, cout,
                                           D, H, W, acc, dt, impl, _st()), impl, f"convT bwd {case} {dts}")
            ref_w, ref_b = (p["dw"] + p["base_w"], p["db"] + p["base_b"]) if acc else (p["dw"], p["db"])
            for name, got, ref in (("dx", dx, p["dx"]), ("dw", dw, ref_w), ("db", db, ref_b)):
                if not _same(got, ref):
                    bad.append(f"{name} {cfg} accumulate {acc}: {_ndiff(got, ref)}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ fused dgrad sums
GSTATS = [("ring", c, dict(CONV_RING=1)) for c in cr.GSTATS_RING_CASES] + [("rows", c, dict(CONV_ROWS=1)) for c in cr.GSTATS_ROWS_CASES]


@pytest.mark.parametrize("dts", ["bf16", "fp16"])
@pytest.mark.parametrize("kern,case,env", GSTATS, ids=[f"{k}-{'x'.join(map(str, c))}" for k, c, _ in GSTATS])
def test_dgrad_gstats(kern, case, env, dts, switches):
    """dgtta_conv3d_k3_dgrad_gstats: what the producer writes.  dx exact; the per-tile sums of g' and g' y_prev, added up per
    (sample, channel), equal conv_ref.gstats_sums exactly (a voxel beyond a ragged W contributes nothing).  Switched off, or on
    the generic kernel, nothing is produced, the buffer keeps its fill and dx is the same."""
    dt, tdt, gran = DTYPES[dts]
    lib = _lib()
    B, cin, cout, D, H, W = case
    p = cr.gstats_problem(case)
    dy, y_prev = _dev(p["dy"], tdt), _dev(p["y_prev"], tdt)
    wpack, cinp, coutp = _pack(p["w"], dts)
    mr = torch.stack((p["mean"], p["rstd"]), dim=-1).float().contiguous().to(DEV)              # [B][Cin][2]
    gamma, beta = _dev(p["gamma"], torch.float32), _dev(p["beta"], torch.float32)
    gbytes = lib.dgtta_conv3d_stats_bytes(B, cin, D, H, W)

    def run(**cfg):
        switches(**cfg)
        dx = torch.full((B, D, H, W, cin), float("nan"), dtype=tdt, device=DEV)
        gst = _nan_stats(gbytes)
        produced = ctypes.c_int(-1)
        _ok(lib.dgtta_conv3d_k3_dgrad_gstats(_p(dy), cout, _p(wpack), _p(dx), cin, B, cin, cout, cinp, coutp, D, H, W, _p(y_prev), cin,
                                             _p(mr), _p(gamma), _p(beta), cr.GSTATS_SLOPE, _p(gst), gbytes, ctypes.byref(produced), dt, 0,
                                             _st()), 0, "dgrad_gstats")
        return dx, gst, produced.value

    dx, gst, produced = run(**env)
    assert produced == 1, "the fused kernel did not take the launch"
    assert _same(dx, p["dx"]), _ndiff(dx, p["dx"])
    s0, s1 = _stats_sums(gst, B, cin)
    assert torch.equal(s0, p["s0"]), "sum of g'"
    assert torch.equal(s1, p["s1"]), "sum of g' y_prev"
    dx2, gst2, produced2 = run(**env)
    assert produced2 == 1 and torch.equal(dx2, dx) and torch.equal(_back(gst2).view(torch.int64), _back(gst).view(torch.int64))
    fill = _back(_nan_stats(gbytes)).view(torch.int64)
    for cfg in ({**env, "IN_GSTATS": "0"}, dict(CONV_RING="0", CONV_ROWS="0")):
        dx0, gst0, produced0 = run(**cfg)
        assert produced0 == 0, cfg
        assert torch.equal(_back(gst0).view(torch.int64), fill), f"{cfg}: the statistics buffer was written"
        assert torch.equal(dx0, dx), cfg


# ------------------------------------------------------------------------------------------------ real-valued operands
MANT = {"bf16": 7, "fp16": 10}


def _spacing(v, dts):
    """Spacing of the output format at magnitude v (float64 tensor): 2^(floor(log2 v) - mantissa bits); fp16 bottoms out at 2^-24."""
    _, e = torch.frexp(v.clamp_min(2.0 ** -126))               # v = m 2^e, m in [0.5, 1)
    sp = torch.ldexp(torch.ones_like(v), e - 1 - MANT[dts])
    return sp.clamp_min(2.0 ** -24) if dts == "fp16" else sp


def _within(got, ref, absb, nprod, dts, what):
    """|got - ref| <= 1/2 spacing_out(|ref| + E) + E, E = n 2^-24 sum |a b|, n = products + 1: the worst case of fp32 summation
    in any order (products of fp32 operands rounded once each) plus one rounding to the output format; no extra factor."""
    E = (nprod + 1) * 2.0 ** -24 * absb
    bound = E if dts == "fp32" else 0.5 * _spacing(ref.abs() + E, dts) + E
    err = (got - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    i = int(ratio.argmax())
    print(f"RATIO {what}: max err/bound {float(ratio.max()):.3f} (err {float(err.reshape(-1)[i]):.3e}, bound "
          f"{float(bound.reshape(-1)[i]):.3e}, ref {float(ref.reshape(-1)[i]):.4f}); max err {float(err.max()):.3e}")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements beyond the bound, worst ratio {float(ratio.max()):.3f}"


@functools.lru_cache(maxsize=None)
def _real_problem(case, stride, dts):
    """randn operands rounded to the storage type, their float64 results and sum |a b| (once per process: the row-reuse and
    the ring group share their first case)."""
    tdt = DTYPES[dts][1]
    B, cin, cout, D, H, W = case
    g = torch.Generator().manual_seed(sum(case) + stride)
    od = tuple(cr.out_extent(n, stride) for n in (D, H, W))
    rnd = lambda t: t.to(tdt).double()                                            # noqa: E731  (what the kernels store)
    x = rnd(torch.randn(B, D, H, W, cin, generator=g))
    w = rnd(torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5)
    bias = torch.randn(cout, generator=g).double()
    dy = rnd(torch.randn(B, *od, cout, generator=g))
    base = rnd(torch.randn(B, D, H, W, cin, generator=g))
    return dict(x=x, w=w, bias=bias, dy=dy, base=base, od=od, y=cr.conv3_fwd(x, w, bias, stride),
                y_abs=cr.abs_bound(cr.conv3_fwd, x, w, bias, stride=stride), dx=cr.conv3_dgrad(dy, w, (D, H, W), stride),
                dx_abs=cr.abs_bound(cr.conv3_dgrad, dy, w, (D, H, W), stride=stride))


@pytest.mark.parametrize("dts", list(DTYPES))
@pytest.mark.parametrize("group", GROUP_FIRST, ids=[g[0] for g in GROUP_FIRST])
def test_real_operands_within_bound(group, dts, switches):
    """randn operands rounded to the storage type: forward and data gradient, element by element, within the derived bound of
    fp32 accumulation against float64 - for dx the first reference that did not go through dgtta_conv3d_pack_weights."""
    name, case, stride, env = group
    dt, tdt, gran = DTYPES[dts]
    B, cin, cout, D, H, W = case
    p = _real_problem(case, stride, dts)
    x, w, bias, dy, base, od = p["x"], p["w"], p["bias"], p["dy"], p["base"], p["od"]
    y_ref, y_abs, dx_ref, dx_abs = p["y"], p["y_abs"], p["dx"], p["dx_abs"]
    ntap_dgrad = 27 if stride == 1 else 8                                         # taps that reach one input voxel
    switches(**env)
    xd, dyd, biasd = _dev(x, tdt), _dev(dy, tdt), _dev(bias, torch.float32)
    wpack, cinp, coutp = _pack(w, dts)
    chans = (cin, cout, cinp, coutp)
    for impl in (0, 1, 2):
        y = torch.full((B, *od, cout), float("nan"), dtype=tdt, device=DEV)
        rc = _fwd(xd, cin, wpack, biasd, y, cout, None, (B, D, H, W), chans, stride, dt, impl)
        if rc == UNSUPPORTED and impl == 2:
            print(f"RATIO {name} {dts} impl 2: refused")
            continue
        _ok(rc, impl, "fwd")
        _within(_back(y), y_ref, y_abs, 27 * cin, dts, f"{name} s{stride} {dts} impl {impl} forward")
        for acc in (0, 1):
            dx = _dev(base, tdt) if acc else torch.full((B, D, H, W, cin), float("nan"), dtype=tdt, device=DEV)
            _ok(_dgrad(dyd, cout, wpack, dx, cin, (B, D, H, W), chans, stride, acc, dt, impl), impl, "dgrad")
            _within(_back(dx), dx_ref + base * acc, dx_abs + base.abs() * acc, ntap_dgrad * cout + acc, dts,
                    f"{name} s{stride} {dts} impl {impl} dgrad acc {acc}")


@pytest.mark.parametrize("dts", list(DTYPES))
def test_real_operands_convT(dts, switches):
    """The same bound for the transposed conv's forward (Cin products and the bias) and data gradient (8 Cout products), read
    from / written into the concat buffer's first half."""
    dt, tdt, gran = DTYPES[dts]
    lib = _lib()
    case = cr.CONVT_CASES[0]
    B, cin, cout, D, H, W = case
    g = torch.Generator().manual_seed(sum(case))
    rnd = lambda t: t.to(tdt).double()                                            # noqa: E731
    x = rnd(torch.randn(B, D, H, W, cin, generator=g))
    w = rnd(torch.randn(cin, cout, 2, 2, 2, generator=g) / cin ** 0.5)
    bias = torch.randn(cout, generator=g).double()
    dcat = rnd(torch.randn(B, 2 * D, 2 * H, 2 * W, 2 * cout, generator=g))
    dout = dcat[..., :cout]
    out_ref, out_abs = cr.convT_fwd(x, w, bias), cr.abs_bound(cr.convT_fwd, x, w, bias)
    dx_ref, dx_abs = cr.convT_dgrad(dout, w), cr.abs_bound(cr.convT_dgrad, dout, w)
    xd, dcatd, wd, biasd = _dev(x, tdt), _dev(dcat, tdt), _dev(w, torch.float32), _dev(bias, torch.float32)
    for gemm in "10":
        switches(CONVT_GEMM=gemm)
        for impl in (0, 1, 2):
            cat = torch.full((B, 2 * D, 2 * H, 2 * W, 2 * cout), SENTINEL, dtype=tdt, device=DEV)
            nb = lib.dgtta_convT3d_fwd_ws_bytes(cin, cout, dt)
            ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
            rc = lib.dgtta_convT3d_k2s2_fwd(_p(xd), cin, _p(wd), _p(biasd), _p(cat), 2 * cout, _p(ws), nb, B, cin, cout, D, H, W, dt, impl,
                                            _st())
            if rc == UNSUPPORTED and impl == 2:
                print(f"RATIO convT {dts} impl 2 gemm {gemm}: refused")
                continue
            _ok(rc, impl, "convT fwd")
            _within(_back(cat)[..., :cout], out_ref, out_abs, cin, dts, f"convT {dts} impl {impl} gemm {gemm} forward")
            dx = torch.full((B, D, H, W, cin), float("nan"), dtype=tdt, device=DEV)
            nb = lib.dgtta_convT3d_bwd_ws_bytes(B, cin, cout, D, H, W)
            ws2 = torch.empty(nb, dtype=torch.uint8, device=DEV)
            _ok(lib.dgtta_convT3d_k2s2_bwd(_p(xd), cin, _p(dcatd), 2 * cout, _p(wd), _p(dx), cin, None, None, _p(ws2), nb, B, cin, cout, D, H,
                                           W, 0, dt, impl, _st()), impl, "convT bwd")
            _within(_back(dx), dx_ref, dx_abs, 8 * cout, dts, f"convT {dts} impl {impl} gemm {gemm} dgrad")
