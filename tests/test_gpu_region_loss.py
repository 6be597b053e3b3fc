"""GPU: the region loss kernels of csrc/region_loss.hip (DC+BCE of R sigmoid outputs against overlapping regions of an integer
label map; plain, batch Dice and strided labels) through the C ABI, against the float64 restatement of tests/region_ref.py
(licensed by tests/test_region_ref.py).

INPUTS.  Logits N(0, 3^2) rounded to fp32.  Regions are nested, region r = labels {r + 1 .. R} (region R - 1 is the single label R),
so the table has L = R + 1 entries; labels are uniform in [0, L) with ignored values -1, L, 255 (outside every table here) and
-2^40 sprinkled in, label R removed from sample 0 (a region absent from a sample), and - where asked - a sample or the whole
batch ignored.  Input rows are padded with NaN up to ldc and lie between NaN guard zones: one read past a row's R outputs or past
the volume poisons the result.  Gradient rows are pre-filled with a sentinel and lie between sentinel guard zones; their padding
columns must come back untouched.

TOLERANCE: the project's rule for the transcendental loss kernels (tests/test_gpu_loss.py).  The yardstick of a case is the error
of a float32 CPU evaluation of THE REFERENCE FORMULA on the same inputs against float64 (region_ref.region_loss(dtype=np.float32));
it never involves the kernel.  Per quantity: |loss| error, largest dice error, and for the gradient largest error per batch item.
The kernel is allowed 8 x the yardstick; the yardstick of the loss is not taken below 2^-24 * max(1, |loss|) (one fp32 number
cannot be closer to the float64 value than half an ulp, while the fp32 CPU evaluation may hit by luck).  Every kernel output must
be finite before it is judged.  loss[0] = loss[1] + loss[2] to three roundings.  Power-of-two scales: bit for bit.

MEASURED on an MI355X, largest kernel error / yardstick over all cases (allowed: 8):
  loss 2.05 (B = 3, R = 32, V = 1), dice 6.33 (B = 1, R = 3, V = 127), gradient 1.59 (the same case)
  without its fp32 floor the loss, one scalar, reaches 52 (B = 3, R = 3, V = 129, batch Dice: the fp32 CPU evaluation happens to
  round far closer to the float64 value than half an ulp)."""
import ctypes

import numpy as np
import pytest
import torch

import region_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
ALLOW = 8.0
SENT = -777.25
GUARD = 64


def f32(x):
    return ctypes.c_float(x).value


def _nested_table(R):
    from dg_tta_amd.labels import membership_table
    return membership_table(tuple(tuple(range(r + 1, R + 1)) for r in range(R)))


def _inputs(B, R, V, seed=0, ignore_sample=None, all_ignored=False):
    rng = np.random.RandomState(100 * R + B + seed + V % 997)
    table = _nested_table(R)
    L = table.size
    assert L == R + 1 and L < 255
    z = (rng.standard_normal((B, R, V)) * 3).astype(np.float32).astype(np.float64)
    y = rng.randint(0, L, size=(B, V)).astype(np.int64)
    if R >= 2:
        y[0][y[0] == R] = 0                                       # the innermost region is absent from sample 0
    if V >= 8:
        y[0, 1:V:31] = -1
        y[0, 2:V:31] = L
        y[B - 1, 3:V:31] = 255
        y[B - 1, 4:V:31] = -2 ** 40
    if ignore_sample is not None:
        y[ignore_sample] = -1
    if all_ignored:
        y[:] = L + 1
    return z, y, table


def _rows(B, V, ld, fill):
    n = B * V * ld
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _put(view, x, ld):
    B, R, V = x.shape
    h = np.full((B, V, ld), np.nan, np.float32)
    h[:, :, :R] = x.transpose(0, 2, 1)
    view.copy_(torch.from_numpy(h.reshape(-1)))


def _get(buf, B, R, V, ld, fill):
    h = buf.cpu().numpy()
    n = B * V * ld
    assert np.all(h[:GUARD] == fill) and np.all(h[GUARD + n:] == fill), "written outside [B][V][ld]"
    rows = h[GUARD:GUARD + n].reshape(B, V, ld)
    return np.ascontiguousarray(rows[:, :, :R].transpose(0, 2, 1)), rows[:, :, R:]


def _lib_and_stream():
    from dg_tta_amd import _lib
    return _lib.load(), _lib.check, _lib.stream_of(torch.device(DEV))


def _same_bits(x, y):
    return np.array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32))


def _abi(z, y, table, smooth=1e-5, batch_dice=None, ldc=None, ldg=None, scale_h=1.0, scale_dev=None, dims=None, strides=None):
    """dgtta_region_loss_fwd (batch_dice None) or _batch_fwd, + _bwd - or the _ds_ forms when dims = (d, h, w) and strides are
    given; y is then the full-resolution map - through the C ABI -> dict(loss [3], dice [B][R], g [B][R][V])."""
    lib, check, st = _lib_and_stream()
    B, R, V = z.shape
    ldc, ldg = R if ldc is None else ldc, R if ldg is None else ldg
    bz, vz = _rows(B, V, ldc, float("nan"))
    _put(vz, z, ldc)
    yd = torch.from_numpy(np.ascontiguousarray(y)).to(DEV)
    td = torch.from_numpy(table.view(np.int32).copy()).to(DEV)
    L = table.size
    small = torch.full((B * R + 7,), SENT, dtype=torch.float32, device=DEV)           # [guard][dice][guard][loss3][guard]
    dice, loss3 = small[1:1 + B * R], small[B * R + 2:B * R + 5]
    nbytes = lib.dgtta_region_loss_ws_bytes(B, R, V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    bg, vg = _rows(B, V, ldg, SENT)
    sd = None if scale_dev is None else torch.tensor([scale_dev], dtype=torch.float32, device=DEV)
    sdp = None if sd is None else sd.data_ptr()
    head = (vz.data_ptr(), ldc, yd.data_ptr(), td.data_ptr(), L)
    if strides is None:
        if batch_dice is None:
            check(lib.dgtta_region_loss_fwd(*head, loss3.data_ptr(), dice.data_ptr(), ws.data_ptr(), nbytes, B, R, V, smooth, st), "fwd")
        else:
            check(lib.dgtta_region_loss_batch_fwd(*head, loss3.data_ptr(), dice.data_ptr(), ws.data_ptr(), nbytes, B, R, V, smooth,
                                                  int(batch_dice), st), "batch_fwd")
        check(lib.dgtta_region_loss_bwd(*head, ws.data_ptr(), scale_h, sdp, vg.data_ptr(), ldg, B, R, V, st), "bwd")
    else:
        assert lib.dgtta_region_loss_ds_ws_bytes(B, R, *dims) == nbytes and dims[0] * dims[1] * dims[2] == V
        if batch_dice is None:
            check(lib.dgtta_region_loss_ds_fwd(*head, loss3.data_ptr(), dice.data_ptr(), ws.data_ptr(), nbytes, B, R, *dims, *strides,
                                               smooth, st), "ds_fwd")
        else:
            check(lib.dgtta_region_loss_ds_batch_fwd(*head, loss3.data_ptr(), dice.data_ptr(), ws.data_ptr(), nbytes, B, R, *dims,
                                                     *strides, smooth, int(batch_dice), st), "ds_batch_fwd")
        check(lib.dgtta_region_loss_ds_bwd(*head, ws.data_ptr(), scale_h, sdp, vg.data_ptr(), ldg, B, R, *dims, *strides, st), "ds_bwd")
    torch.cuda.synchronize()
    s = small.cpu().numpy()
    assert s[0] == SENT and s[B * R + 1] == SENT and s[B * R + 5] == SENT and s[B * R + 6] == SENT
    g, pad = _get(bg, B, R, V, ldg, SENT)
    assert np.all(pad == SENT), "the padding columns of the gradient rows were written (the kernel stores R columns per row)"
    return dict(loss=s[B * R + 2:B * R + 5].copy(), dice=s[1:1 + B * R].reshape(B, R).copy(), g=g)


WORST = {"loss": 0.0, "dice": 0.0, "grad": 0.0}


def _judge(name, got, ref64, ref32):
    """Kernel error / yardstick per quantity (module docstring); every ratio is printed, then asserted to be at most 8."""
    for k in ("loss", "dice", "g"):
        assert np.all(np.isfinite(got[k])), f"{name}: the kernel's {k} is not finite"

    def ratios(err_k, yard):                     # element-wise; no error at all is ratio 0 whatever the yardstick
        err_k, yard = np.asarray(err_k, np.float64), np.asarray(yard, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(err_k == 0, 0.0, err_k / yard)
    lk, l64, l32 = (np.asarray(x, np.float64) for x in (got["loss"], ref64[0], ref32[0]))
    raw_yard = np.abs(l32 - l64)
    out = {"loss": float(np.max(ratios(np.abs(lk - l64), np.maximum(raw_yard, U * np.maximum(1.0, np.abs(l64)))))),
           "loss (raw)": float(np.max(ratios(np.abs(lk - l64), raw_yard)))}
    d64 = ref64[1]
    out["dice"] = float(ratios(np.abs(got["dice"] - d64).max(), np.abs(ref32[1] - d64).max()))
    per_item = [0.0]
    g64, g32, gk = ref64[2], ref32[2], got["g"]
    for b in range(g64.shape[0]):
        if not g64[b].any():
            assert not gk[b].any(), f"{name}: g[{b}] must be exactly zero"
            continue
        per_item.append(float(ratios(np.abs(gk[b] - g64[b]).max(), np.abs(g32[b] - g64[b]).max())))
    out["grad"] = float(np.max(per_item))
    print(f"\n{name}: kernel error / yardstick  " + "  ".join(f"{q} {v:.2f}" for q, v in out.items()))
    for q in WORST:
        WORST[q] = max(WORST[q], out[q])
    print(f"largest so far: " + "  ".join(f"{q} {v:.2f}" for q, v in WORST.items()))
    for q in ("loss", "dice", "grad"):
        assert out[q] <= ALLOW, f"{name}: {q} error is {out[q]:.2f} x the yardstick"
    return out


def _case(name, z, y, table, smooth=1e-5, batch_dice=None, **abi):
    got = _abi(z, y, table, smooth, batch_dice, **abi)
    strides = abi.get("strides") or (1, 1, 1)
    zz = z if "dims" not in abi else z.reshape(*z.shape[:2], *abi["dims"])
    ref64 = region_ref.region_loss(zz, y, table, f32(smooth), bool(batch_dice), strides)
    ref32 = region_ref.region_loss(zz, y, table, f32(smooth), bool(batch_dice), strides, dtype=np.float32)
    flat = lambda r: (np.array(r[0], dtype=np.float64), r[1], r[2].reshape(z.shape))
    _judge(name, got, flat(ref64), flat(ref32))
    l0, l1, l2 = (float(x) for x in got["loss"])
    assert abs(l0 - (l1 + l2)) <= U * (abs(l0) + abs(l1) + abs(l2))              # three roundings of one double sum
    return got


# ================================================================================================ shapes, labels, switches
@pytest.mark.parametrize("batch_dice", [False, True])
@pytest.mark.parametrize("smooth", [1e-5, 0.0])
@pytest.mark.parametrize("B,R,V", [
    (3, 1, 129),          # a single region (pitch 1); one tile and one voxel
    (3, 2, 129),
    (3, 3, 129),          # the KiTS / BraTS head
    (1, 31, 129),         # odd pitch 31
    (8, 32, 129),         # every bit of the table, all 256 threads in the tile's region sums; the largest batch
])
def test_region_loss_shapes_labels_and_switches(B, R, V, smooth, batch_dice):
    """Labels: ignored values -1, L, 255, -2^40; the innermost region absent from sample 0; with B >= 3 sample 1 is ignored
    entirely (per-sample Dice: dice 1 with smooth = 1e-5, 0 / 1e-8 = 0 with smooth = 0; gradient 0 in either mode)."""
    z, y, table = _inputs(B, R, V, ignore_sample=1 if B >= 3 else None)
    got = _case(f"region_loss B {B} R {R} V {V} smooth {smooth:g} batch {batch_dice}", z, y, table, smooth, batch_dice)
    if B >= 3:
        assert not got["g"][1].any()
        if not batch_dice:
            assert np.all(got["dice"][1] == (1.0 if smooth else 0.0))
    if batch_dice:
        assert all(_same_bits(got["dice"][b], got["dice"][0]) for b in range(B))
    elif R >= 2 and smooth == 0.0:
        assert got["dice"][0, R - 1] == 0.0
    assert got["g"][0].any()
    if not batch_dice:                       # batch_dice = 0 of the _batch_ entry and the plain entry: the same bits
        plain = _abi(z, y, table, smooth, None)
        assert all(_same_bits(got[k], plain[k]) for k in ("loss", "dice", "g"))


def test_region_loss_batch_dice_differs_from_per_sample():
    z, y, table = _inputs(2, 3, 300, seed=4)
    a, b = _abi(z, y, table, 1e-5, False), _abi(z, y, table, 1e-5, True)
    assert a["loss"][1] == b["loss"][1] and a["loss"][2] != b["loss"][2] and not _same_bits(a["g"], b["g"])


@pytest.mark.parametrize("V", [1, 127, 128, 1000])
@pytest.mark.parametrize("B,R", [(1, 3), (3, 32)])
def test_region_loss_volume_sizes(B, R, V):
    """Around one 128-voxel tile; 1000 = eight tiles, the last of 104 voxels (the eight-deep load loop at a short tile)."""
    z, y, table = _inputs(B, R, V)
    _case(f"region_loss B {B} R {R} V {V}", z, y, table)


def test_region_loss_second_grid_stride_pass():
    """V = 262 144 + 128 + 37 at R = 2: above the forward cap (1024 workgroups x 128 voxels) and the backward cap (2048 x 128)."""
    z, y, table = _inputs(1, 2, 262144 + 128 + 37)
    _case("region_loss R 2 V 262309", z, y, table)


def test_region_loss_whole_batch_ignored():
    z, y, table = _inputs(3, 3, 200, all_ignored=True)
    for bd in (False, True):
        got = _abi(z, y, table, 1e-5, bd)
        assert got["loss"].tolist() == [-1.0, 0.0, -1.0] and np.all(got["dice"] == 1.0) and not got["g"].any()
        got = _abi(z, y, table, 0.0, bd)
        assert got["loss"].tolist() == [0.0, 0.0, 0.0] and np.all(got["dice"] == 0.0) and not got["g"].any()


def test_region_loss_large_logits_stay_finite():
    """+-80 in a few voxels, with either target: sigmoid, s (1 - s) and the softplus are formed from exp(-|z|)."""
    z, y, table = _inputs(2, 3, 300, seed=6)
    z[0, :, 5:300:37] = 80.0
    z[1, :, 6:300:37] = -80.0
    z[0, 1, 7:300:41] = -80.0
    got = _case("region_loss +-80", z, y, table)
    assert np.all(np.isfinite(got["g"])) and np.all(np.isfinite(got["loss"]))
    hot = np.abs(z) == 80.0
    assert hot.sum() > 20 and np.all(np.abs(got["g"][hot]) <= 1.0)


@pytest.mark.parametrize("R", [1, 3, 32])
@pytest.mark.parametrize("dc,dg", [(0, 0), (3, 0), (0, 1), (4, 4)])
def test_region_loss_row_pitch(R, dc, dg):
    """(ldc, ldg) = (R + dc, R + dg): the contiguous eight-deep load only at ldc == R, the strided load and store otherwise.
    Input padding NaN, gradient pre-filled with a sentinel: results bit-identical to dense rows, padding untouched."""
    ldc, ldg = R + dc, R + dg
    z, y, table = _inputs(2, R, 300, seed=1)
    got = _case(f"region_loss R {R} ldc {ldc} ldg {ldg}", z, y, table, ldc=ldc, ldg=ldg)
    if (dc, dg) != (0, 0):
        plain = _abi(z, y, table)
        assert all(_same_bits(got[k], plain[k]) for k in ("loss", "dice", "g"))


def test_region_loss_host_and_device_scale_and_reproducibility():
    z, y, table = _inputs(2, 3, 300, seed=2)
    one, again = _abi(z, y, table), _abi(z, y, table)
    assert all(_same_bits(one[k], again[k]) for k in ("loss", "dice", "g"))
    for kw in (dict(scale_h=1024.0), dict(scale_h=4096.0, scale_dev=0.25), dict(scale_h=1.0, scale_dev=1024.0)):
        big = _abi(z, y, table, **kw)
        normal = (np.abs(one["g"]) >= 2.0 ** -126) | (one["g"] == 0)
        assert normal.mean() >= 0.999 and _same_bits(one["loss"], big["loss"])
        assert _same_bits((one["g"] * np.float32(1024))[normal], big["g"][normal]) and np.abs(big["g"]).max() > 0


@pytest.mark.parametrize("batch_dice", [None, True])
@pytest.mark.parametrize("strides", [(2, 2, 2), (1, 2, 2), (1, 1, 1)])
def test_region_loss_strided_labels(strides, batch_dice):
    """The deep-supervision entry points at (4, 6, 8): low-resolution logits against the full-resolution label map read through
    (i sd + sd / 2, j sh + sh / 2, k sw + sw / 2); bit-equal to the dense entry on the sliced map - at strides (1, 1, 1) that is
    the dense entry on the same map."""
    from dg_tta_amd import ops
    B, R, dims = 2, 3, (4, 6, 8)
    V = dims[0] * dims[1] * dims[2]
    table = _nested_table(R)
    rng = np.random.RandomState(sum(strides) * 10 + V)
    z = (rng.standard_normal((B, R, V)) * 3).astype(np.float32).astype(np.float64)
    full = rng.randint(-1, table.size + 1, size=(B, *(d * s for d, s in zip(dims, strides)))).astype(np.int64)
    got = _case(f"region_loss strides {strides} batch {batch_dice}", z, full, table, batch_dice=batch_dice, dims=dims, strides=strides)
    low = np.ascontiguousarray(full[:, strides[0] // 2::strides[0], strides[1] // 2::strides[1], strides[2] // 2::strides[2]])
    plain = _abi(z, low.reshape(B, V), table, batch_dice=batch_dice)
    assert all(_same_bits(got[k], plain[k]) for k in ("loss", "dice", "g"))
    # the tensor wrappers reach the same kernels
    t = torch.from_numpy(z.astype(np.float32)).reshape(B, R, *dims).to(DEV).requires_grad_(True)
    loss, _ = ops.deep_supervision_region_loss([t], torch.from_numpy(full).to(DEV), table, weights=[1.0], batch_dice=bool(batch_dice))
    loss.backward()
    assert _same_bits(float(loss.detach()), got["loss"][0])
    assert _same_bits(t.grad.cpu().numpy().reshape(B, R, V), got["g"])
    t2 = torch.from_numpy(z.astype(np.float32)).reshape(B, R, *dims).to(DEV).requires_grad_(True)
    loss2, dice2, parts = ops.region_loss(t2, torch.from_numpy(low).to(DEV), table, batch_dice=bool(batch_dice))
    loss2.backward()
    assert _same_bits(float(loss2.detach()), got["loss"][0]) and _same_bits(dice2.cpu().numpy(), got["dice"])
    assert _same_bits(parts.detach().cpu().numpy(), got["loss"][1:]) and _same_bits(t2.grad.cpu().numpy().reshape(B, R, V), got["g"])


def test_region_loss_argument_checks():
    from dg_tta_amd._lib import DgttaError
    lib, check, st = _lib_and_stream()
    assert lib.dgtta_region_loss_ws_bytes(0, 3, 100) == 0 and lib.dgtta_region_loss_ws_bytes(2, 3, 0) == 0
    assert lib.dgtta_region_loss_ws_bytes(9, 3, 100) == 0 and lib.dgtta_region_loss_ws_bytes(2, 33, 100) == 0
    assert lib.dgtta_region_loss_ws_bytes(2, 0, 100) == 0 and lib.dgtta_region_loss_ds_ws_bytes(2, 3, 0, 4, 4) == 0
    assert lib.dgtta_region_loss_ws_bytes(8, 32, 1 << 40) > 0
    t = torch.zeros(8 * 32 * 4 * 2, dtype=torch.float32, device=DEV)
    lab = torch.zeros(8 * 64, dtype=torch.int64, device=DEV)
    tab = torch.zeros(1024, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.dgtta_region_loss_ws_bytes(8, 32, 4), dtype=torch.uint8, device=DEV)
    need = lib.dgtta_region_loss_ws_bytes(2, 3, 4)
    p, y, tb, w = t.data_ptr(), lab.data_ptr(), tab.data_ptr(), ws.data_ptr()

    def fwd(B=2, R=3, ldc=3, L=4, nbytes=None, batch=None):
        nb = ws.numel() if nbytes is None else nbytes
        if batch is None:
            check(lib.dgtta_region_loss_fwd(p, ldc, y, tb, L, p, p, w, nb, B, R, 4, 1e-5, st), "fwd")
        else:
            check(lib.dgtta_region_loss_batch_fwd(p, ldc, y, tb, L, p, p, w, nb, B, R, 4, 1e-5, batch, st), "batch_fwd")

    def bwd(B=2, R=3, ldc=3, ldg=3, L=4):
        check(lib.dgtta_region_loss_bwd(p, ldc, y, tb, L, w, 1.0, None, p, ldg, B, R, 4, st), "bwd")
    fwd()
    fwd(R=1, ldc=1)
    fwd(R=32, ldc=32, L=1024)
    for kw, code in ((dict(B=9), -1), (dict(B=0), -1), (dict(R=0, ldc=1), -1), (dict(R=33, ldc=33), -1), (dict(ldc=2), -1),
                     (dict(L=0), -1), (dict(L=1025), -1), (dict(batch=2), -1), (dict(batch=-1), -1), (dict(nbytes=need - 1), -3)):
        with pytest.raises(DgttaError, match=rf"code {code}\)"):
            fwd(**kw)
    for kw in (dict(B=9), dict(R=0), dict(R=33, ldc=33, ldg=33), dict(ldc=2), dict(ldg=2), dict(L=0), dict(L=1025)):
        with pytest.raises(DgttaError, match=r"code -1\)"):
            bwd(**kw)
    for dims in ((0, 2, 2, 1, 1, 1), (1, 2, 2, 0, 1, 1), (1, 2, 2, 1, 1, -1)):
        with pytest.raises(DgttaError, match=r"code -1\)"):
            check(lib.dgtta_region_loss_ds_fwd(p, 3, y, tb, 4, p, p, w, ws.numel(), 2, 3, *dims, 1e-5, st), "ds_fwd")
        with pytest.raises(DgttaError, match=r"code -1\)"):
            check(lib.dgtta_region_loss_ds_batch_fwd(p, 3, y, tb, 4, p, p, w, ws.numel(), 2, 3, *dims, 1e-5, 1, st), "ds_batch_fwd")
        with pytest.raises(DgttaError, match=r"code -1\)"):
            check(lib.dgtta_region_loss_ds_bwd(p, 3, y, tb, 4, w, 1.0, None, p, 3, 2, 3, *dims, st), "ds_bwd")
    with pytest.raises(DgttaError, match=r"code -1\)"):
        check(lib.dgtta_region_loss_fwd(None, 3, y, tb, 4, p, p, w, ws.numel(), 2, 3, 4, 1e-5, st), "fwd")
    torch.cuda.synchronize()
