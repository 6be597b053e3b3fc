"""GPU: the loss kernels of csrc/softdice.hip (masked-softmax soft-Dice consistency loss: generic LDS-tile kernels, the 16-class
DPP kernels, the stand-alone `probs` kernels) and csrc/dice_ce.hip (DC+CE, plain and strided labels) against the float64
restatements of tests/loss_ref.py (licensed by tests/test_loss_ref.py).  Cases the tensor wrappers of ops.py cannot reach (row
pitch ldc / ldg, guard_items, host and device scale, misaligned rows) go through the C ABI.

INPUTS OF THE MASKED LOSS.  The mask is a hard function of an fp32 class sum, so the logits are multiples of 2^-10 with
|x| < 32: a sum over at most 128 classes is a multiple of 2^-10 below 2^12 at every partial sum, i.e. exact in fp32 IN ANY ORDER
(22 bits) - the sequential sum of the generic kernel, the quad tree of the 16-class kernel and the float64 reference see the
same sign.  Both properties are asserted (_assert_exact_sums).  A positive bias keeps well over half the voxels unmasked; every
29th voxel is a row of exact zeros in both branches (the warp's border), the next has a negative sum in branch a only, the next
in branch b only.  Input rows are padded with NaN up to ldc and lie between NaN guard zones: one read past a row's C classes
or past the volume poisons the result.  Gradient buffers are pre-filled with a sentinel and lie between sentinel guard zones.

TOLERANCES.
  softmax kernels (expf / logf): the yardstick of a case is the error of a float32 CPU evaluation of THE REFERENCE FORMULA on
      the same inputs against float64 (loss_ref.*(dtype=np.float32)); it never involves the kernel.  Per quantity: |loss|
      error, largest dice error, and for the gradient largest error / largest reference value per batch item and branch.  The
      kernel is allowed 8 x the yardstick (summation order, device expf / logf against libm).  For dice and gradient that is
      the whole rule.  For the loss there is one addition, from the number format alone: the kernel's loss is ONE fp32 number,
      so even a kernel without any error of its own is off by up to u = 2^-24 relative (half an ulp) from the float64 value,
      while the fp32 CPU evaluation of one scalar is, by luck, often much closer than that (its single final rounding may
      hit).  The yardstick of the loss is therefore not taken below u * max(1, |loss|) (the loss is formed as 1 - x or ce + x
      with terms of order 1).  Every case prints the loss ratio with and without that floor ("loss (raw)").
      Every kernel output must be finite before it is judged: input padding and guard zones are NaN.
  probs kernels (no transcendental functions): derived, u = 2^-24, non-negative inputs.  A thread adds at most 64 products in
      fp32: nom (1 + u)^65 - 1, den (x + y rounded, squared, added) 67 u; the narrowing to fp32 before block_sum u; block_sum
      (six butterfly levels + four waves) 10 u; the mean is formed in double and rounded once, u: nom 77 u, den 79 u, and
      dice = nom / den 158 u relative (division: 2 u allowed).  Backward with the reference's P = 2 g / (V den) and
      Q = -g nom / (V den^2): the kernel's P carries 1 / (B C) (2 u), V den (80 u), its division (2 u), g B C (u) and the product
      (u): 86 u; Q 2 + 78 + 159 + 1 + 2 + 2 = 244 u; t = Q (x + y) 246 u, and |ga_k - ga| <= 87 u |P y| + 246 u |t| + u |ga|.
      The bounds are multiplied by 1 + 2^-16 for the second-order terms.
  power-of-two scales: bit for bit.

MEASURED on an MI355X, largest kernel error / yardstick over all cases (allowed: 8):
  soft Dice (generic and 16-class kernels)   loss 2.22, dice 4.63 (C = 5, V = 1), gradient 4.50 (C = 65, B = 8, V = 1)
  DC + CE                                    loss 1.42, dice 4.25, gradient 1.66
  without its fp32 floor the loss, one scalar, reaches 15 (soft Dice) and 966 (DC + CE, a case in which the fp32 CPU
  evaluation happens to round to within 1e-10 of the float64 value).
  probs kernels, error / derived bound (allowed: 1): dice 0.026, gradient 0.031 (the bounds are worst cases over up to 80
  roundings of one sign; rounding errors of random sign cancel)."""
import ctypes

import numpy as np
import pytest
import torch

import loss_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
ALLOW = 8.0
SENT = -777.25
GUARD = 64                       # floats of guard zone on either side of a row buffer


# ================================================================================================ helpers
def _assert_exact_sums(x):
    """x [B][C][V] float64: multiples of 2^-10 below 32, and the fp32 class sums equal the float64 one in three orders."""
    assert np.array_equal(np.round(x * 1024), x * 1024) and np.abs(x).max() < 32
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x)
    want = x.sum(axis=1)
    fwd, rev = x32[:, 0].copy(), x32[:, -1].copy()
    for c in range(1, x.shape[1]):
        fwd, rev = fwd + x32[:, c], rev + x32[:, -1 - c]
    assert fwd.dtype == np.float32 and np.array_equal(fwd, want) and np.array_equal(rev, want)
    assert np.array_equal(x32.sum(axis=1, dtype=np.float32), want)


_INPUTS = {}


def _inputs(B, C, V, seed=0, masked_items=()):
    """(la, lb) class-major float64 on the 2^-10 grid (see the module docstring); masked_items: batch items masked entirely."""
    key = (B, C, V, seed, tuple(masked_items))
    if key in _INPUTS:
        return _INPUTS[key]
    rng = np.random.RandomState(1000 * C + 7 * B + seed + V % 1000)
    bias = np.ceil(3.0 / np.sqrt(C) * 1024) / 1024
    la, lb = (np.clip(np.round(rng.standard_normal((B, C, V)) * 2048) / 1024 + bias, -31.0, 31.0) for _ in range(2))
    if V >= 3:
        la[:, :, 0::29] = 0.0
        lb[:, :, 0::29] = 0.0
        la[:, :, 1::29] = -np.abs(la[:, :, 1::29])
        lb[:, :, 2::29] = -np.abs(lb[:, :, 2::29])
    else:                                  # one or two voxels: unmasked (an item without any voxel has dice 0 / 0)
        la, lb = np.abs(la), np.abs(lb)
    for i in masked_items:
        la[i] = -np.abs(la[i])
    _assert_exact_sums(la)
    _assert_exact_sums(lb)
    if V >= 63 and not masked_items:
        unmasked = ((la.sum(1) > 0) & (lb.sum(1) > 0)).mean()
        assert 0.5 < unmasked < 0.95, unmasked
    if la.size <= 1 << 21:
        _INPUTS[key] = (la, lb)
    return la, lb


_REFS = {}


def _softdice_refs(la, lb, start_class, guard_items, key=None):
    """(float64 reference, float32 evaluation of the same formula), computed once per case."""
    if key is not None and key in _REFS:
        return _REFS[key]
    out = (loss_ref.softdice(la, lb, start_class, guard_items), loss_ref.softdice(la, lb, start_class, guard_items, dtype=np.float32))
    if key is not None and la.size <= 1 << 21:
        _REFS[key] = out
    return out


def _rows(B, V, ld, fill, misalign=False):
    """A row buffer [B][V][ld] between guard zones, everything pre-filled with `fill` -> (whole buffer, view, lead)."""
    n = B * V * ld
    lead = GUARD + (1 if misalign else 0)
    buf = torch.full((lead + n + GUARD,), fill, dtype=torch.float32, device=DEV)
    view = buf[lead:lead + n]
    assert view.data_ptr() % 16 == (4 if misalign else 0)
    return buf, view, lead


def _put(view, x, ld):
    """Class-major [B][C][V] -> voxel-major rows of pitch ld, padding columns NaN."""
    B, C, V = x.shape
    h = np.full((B, V, ld), np.nan, np.float32)
    h[:, :, :C] = x.transpose(0, 2, 1)
    view.copy_(torch.from_numpy(h.reshape(-1)))


def _get(buf, lead, B, C, V, ld, fill):
    """-> (class-major [B][C][V] fp32, padding columns [B][V][ld - C]); the guard zones must still hold `fill`."""
    h = buf.cpu().numpy()
    n = B * V * ld
    assert np.all(h[:lead] == fill) and np.all(h[lead + n:] == fill), "written outside [B][V][ld]"
    rows = h[lead:lead + n].reshape(B, V, ld)
    return np.ascontiguousarray(rows[:, :, :C].transpose(0, 2, 1)), rows[:, :, C:]


def _lib_and_stream():
    from dg_tta_amd import _lib
    return _lib.load(), _lib.check, _lib.stream_of(torch.device(DEV))


def _softdice_abi(la, lb, start_class=1, guard_items=None, ldc=None, misalign=False, scale_h=1.0, scale_dev=None):
    """dgtta_softdice_fwd + _bwd through the C ABI -> dict(loss, dice [B][C], ga, gb [B][C][V]) as fp32 numpy."""
    lib, check, st = _lib_and_stream()
    B, C, V = la.shape
    ldc = C if ldc is None else ldc
    nan = float("nan")
    (ba, va, _), (bb, vb, _) = _rows(B, V, ldc, nan, misalign), _rows(B, V, ldc, nan, misalign)
    _put(va, la, ldc)
    _put(vb, lb, ldc)
    small = torch.full((B * C + 4,), SENT, dtype=torch.float32, device=DEV)           # [guard][dice B*C][guard][loss][guard]
    dice, loss = small[1:1 + B * C], small[B * C + 2:B * C + 3]
    nbytes = lib.dgtta_softdice_ws_bytes(B, C, V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    check(lib.dgtta_softdice_fwd(va.data_ptr(), vb.data_ptr(), dice.data_ptr(), loss.data_ptr(), ws.data_ptr(), nbytes, B, C, V, ldc,
                                 start_class, guard_items or B, st), "dgtta_softdice_fwd")
    (bga, vga, lead), (bgb, vgb, _) = _rows(B, V, ldc, SENT, misalign), _rows(B, V, ldc, SENT, misalign)
    sd = None if scale_dev is None else torch.tensor([scale_dev], dtype=torch.float32, device=DEV)
    check(lib.dgtta_softdice_bwd(va.data_ptr(), vb.data_ptr(), vga.data_ptr(), vgb.data_ptr(), ws.data_ptr(), scale_h,
                                 None if sd is None else sd.data_ptr(), B, C, V, ldc, start_class, st), "dgtta_softdice_bwd")
    torch.cuda.synchronize()
    s = small.cpu().numpy()
    assert s[0] == SENT and s[B * C + 1] == SENT and s[B * C + 3] == SENT
    ga, pad_a = _get(bga, lead, B, C, V, ldc, SENT)
    gb, pad_b = _get(bgb, lead, B, C, V, ldc, SENT)
    assert not pad_a.any() and not pad_b.any(), "padding columns of the gradient rows are not zero"
    return dict(loss=s[B * C + 2], dice=s[1:1 + B * C].reshape(B, C).copy(), ga=ga, gb=gb)


def _same_bits(x, y):
    return np.array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32))


def _judge(name, got, ref64, ref32, grads=("ga", "gb")):
    """Kernel error / yardstick per quantity (module docstring): every kernel output must be finite, and every ratio at most 8
    (asserted after printing them).  The reductions are numpy maxima, which a NaN would pass through."""
    for k in ("loss", "dice", *grads):
        assert np.all(np.isfinite(got[k])), f"{name}: the kernel's {k} is not finite"

    def ratios(err_k, yard):                     # element-wise; no error at all is ratio 0 whatever the yardstick
        err_k, yard = np.asarray(err_k, np.float64), np.asarray(yard, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(err_k == 0, 0.0, err_k / yard)
    lk, l64, l32 = (np.atleast_1d(np.asarray(x, np.float64)) for x in (got["loss"], ref64[0], ref32[0]))
    raw_yard = np.abs(l32 - l64)
    out = {"loss": float(np.max(ratios(np.abs(lk - l64), np.maximum(raw_yard, U * np.maximum(1.0, np.abs(l64)))))),
           "loss (raw)": float(np.max(ratios(np.abs(lk - l64), raw_yard)))}
    d64 = ref64[1]
    out["dice"] = float(ratios(np.abs(got["dice"] - d64).max(), np.abs(ref32[1] - d64).max()))
    per_item = [0.0]
    for k, name_g in enumerate(grads):
        g64, g32, gk = ref64[2 + k], ref32[2 + k], got[name_g]
        for b in range(g64.shape[0]):
            if not g64[b].any():
                assert not gk[b].any(), f"{name}: {name_g}[{b}] must be exactly zero"
                continue
            per_item.append(float(ratios(np.abs(gk[b] - g64[b]).max(), np.abs(g32[b] - g64[b]).max())))   # (both over max |g64[b]|)
    out["grad"] = float(np.max(per_item))
    print(f"\n{name}: kernel error / yardstick  " + "  ".join(f"{q} {v:.2f}" for q, v in out.items()))
    for q in ("loss", "dice", "grad"):
        assert out[q] <= ALLOW, f"{name}: {q} error is {out[q]:.2f} x the yardstick"
    return out


def _softdice_case(la, lb, name, start_class=1, guard_items=None, key=None, **abi):
    got = _softdice_abi(la, lb, start_class, guard_items, **abi)
    ref64, ref32 = _softdice_refs(la, lb, start_class, guard_items, key)
    _judge(name, got, ref64, ref32)
    return got


def _waves(ldc):                  # waves_for(ldc) of softdice.hip: two [64][ldc | 1] fp32 tiles per wave in 96 KiB, at most 4
    return max(1, min(4, (96 * 1024) // (2 * 64 * (ldc | 1) * 4)))


def _set16(monkeypatch, on):
    from conftest import reload_kernel_switches
    monkeypatch.setenv("DGTTA_SOFTDICE16", "1" if on else "0")
    reload_kernel_switches()


# ================================================================================================ soft Dice: branches
def test_wave_counts_assumed_by_the_cases_below():
    """waves_for: 4 waves up to ldc 47, 3 at 48..63 (pitch 49..63), 2 at 64..95, 1 from 96."""
    assert [_waves(c) for c in (1, 5, 21, 33, 47, 48, 63, 64, 65, 68, 95, 96, 128)] == [4, 4, 4, 4, 4, 3, 3, 2, 2, 2, 2, 1, 1]


@pytest.mark.parametrize("C,way", [
    (1, "generic"),       # 64 voxel groups, start_class 0 (the only one a single class allows)
    (2, "generic"),       # 32 groups
    (5, "generic"),       # 12 groups, lanes 60..63 idle in the reduction
    (16, "generic"),      # DGTTA_SOFTDICE16=0: the LDS-tile kernels at 16 classes (4 groups)
    (16, "16"),           # the 16-class DPP kernels
    (21, "generic"),      # three voxel groups, one idle lane
    (33, "generic"),      # groups == 1, 31 idle lanes
    (48, "generic"),      # groups == 1, THREE waves per workgroup
    (64, "generic"),      # groups == 1, every lane busy, TWO waves
    (65, "generic"),      # NR == 2: the second accumulator holds one class; two waves
    (96, "generic"),      # NR == 2, ONE wave per workgroup
    (128, "generic"),     # NR == 2, both accumulators full, one wave
])
def test_softdice_every_class_count_branch(C, way, monkeypatch):
    """B = 2, V = 333: nblocks_for = 2 workgroups per batch item, which cover 512, 384, 256 or 128 voxels per pass with 4, 3, 2
    or 1 waves (so two passes at C >= 64, three at C >= 96), a ragged last tile of 13 voxels, waves without a tile."""
    _set16(monkeypatch, way == "16")
    la, lb = _inputs(2, C, 333)
    start = 0 if C == 1 else 1
    _softdice_case(la, lb, f"softdice C {C} ({way})", start, key=("C", C, start))


@pytest.mark.parametrize("V", [1, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize("C,way,B", [
    (5, "generic", 1),    # four waves: a workgroup pass is 256 voxels - below, at and above one tile and one pass
    (16, "16", 2),        # 64 voxels per workgroup pass, whole quads in or out
    (65, "generic", 8),   # two accumulators, two waves (128 voxels per pass), the largest batch
])
def test_softdice_volume_sizes(C, way, B, V, monkeypatch):
    _set16(monkeypatch, way == "16")
    la, lb = _inputs(B, C, V)
    _softdice_case(la, lb, f"softdice C {C} B {B} V {V}", key=("V", B, C, V))


def test_softdice_128_classes_four_grid_stride_passes():
    """C = 128: one wave per workgroup, nblocks_for(1000) = 4 workgroups of 64 voxels per pass: four passes, the last ragged."""
    la, lb = _inputs(1, 128, 1000)
    _softdice_case(la, lb, "softdice C 128 V 1000")


@pytest.mark.parametrize("C,way", [(2, "generic"), (16, "16")])
def test_softdice_second_grid_stride_pass_of_every_kernel(C, way, monkeypatch):
    """V = 524 288 + 64 + 37: above the forward cap (1024 workgroups x 256 voxels, 16-class: x 64) and the backward caps (2048 x
    256; 16-class 4096 x 64), so one workgroup of every kernel takes a second pass, with a ragged tile at the end."""
    _set16(monkeypatch, way == "16")
    la, lb = _inputs(1, C, 524288 + 64 + 37)
    _softdice_case(la, lb, f"softdice C {C} V 524389 ({way})")


# ================================================================================================ soft Dice: guard, start class
@pytest.mark.parametrize("C,way", [(5, "generic"), (16, "16")])
@pytest.mark.parametrize("guard_items", [1, 2, 4])
@pytest.mark.parametrize("start", ["0", "1", "C-1"])
def test_softdice_guard_groups_and_start_class(C, way, guard_items, start, monkeypatch):
    """B = 4; the LAST guard group is masked entirely (guard_items 1: item 3, next to three unguarded groups; 2: items 2 and 3;
    4: the whole call): its dice is exactly 1 and its gradient rows exactly 0, the other groups match the reference."""
    _set16(monkeypatch, way == "16")
    start_class = {"0": 0, "1": 1, "C-1": C - 1}[start]
    masked = tuple(range(4 - guard_items, 4))
    la, lb = _inputs(4, C, 150, seed=3, masked_items=masked)
    got = _softdice_case(la, lb, f"softdice C {C} guard {guard_items} start {start_class}", start_class, guard_items,
                         key=("guard", C, guard_items, start_class))
    for i in range(4):
        if i in masked:
            assert np.all(got["dice"][i] == 1.0) and not got["ga"][i].any() and not got["gb"][i].any()
        else:
            assert got["ga"][i, start_class:].any() and np.all(got["dice"][i] < 1.0)
    if guard_items == 4:
        assert got["loss"] == 0.0


# ================================================================================================ soft Dice: row pitch
@pytest.mark.parametrize("C,ldc,misalign", [
    (5, 5, False),        # odd pitch: scalar path
    (5, 6, False),        # one padding column, ldc % 4 != 0: scalar path
    (5, 8, False),        # three padding columns on the float4 path
    (8, 8, False),        # float4 path without padding
    (8, 8, True),         # the same rows 4 bytes into their allocations: the scalar path must be taken
    (8, 12, False),       # float4 path, a float4 of pure padding per row
    (65, 68, False),      # two accumulators with padding, float4 path
])
def test_softdice_row_pitch_and_alignment(C, ldc, misalign):
    """B = 2, V = 301 (ragged last tile).  Inputs: NaN padding columns and NaN guard zones; gradients: sentinel pre-fill and
    sentinel guard zones (checked inside _softdice_abi: padding columns come back zero, nothing outside [B][V][ldc] is written).
    The layout does not change the arithmetic: the results equal those of dense aligned rows bit for bit (same wave count)."""
    la, lb = _inputs(2, C, 301, seed=5)
    got = _softdice_case(la, lb, f"softdice C {C} ldc {ldc} misaligned {misalign}", key=("pitch", C), ldc=ldc, misalign=misalign)
    if (ldc != C or misalign) and _waves(ldc) == _waves(C):
        plain = _softdice_abi(la, lb)
        assert all(_same_bits(got[k], plain[k]) for k in ("loss", "dice", "ga", "gb"))


# ================================================================================================ soft Dice: scale, properties
@pytest.mark.parametrize("C,way", [(5, "generic"), (16, "16"), (65, "generic")])
def test_softdice_host_and_device_scale_are_exact_powers_of_two(C, way, monkeypatch):
    """grad_scale 4096 on the host x 0.25 on the device = 1024 x the scale-1 gradient, bit for bit (results that are subnormal at
    scale 1 excepted: at most 0.1 % of the elements)."""
    _set16(monkeypatch, way == "16")
    la, lb = _inputs(2, C, 301, seed=5)
    one = _softdice_abi(la, lb)
    big = _softdice_abi(la, lb, scale_h=4096.0, scale_dev=0.25)
    assert _same_bits(one["loss"], big["loss"]) and _same_bits(one["dice"], big["dice"])
    for k in ("ga", "gb"):
        normal = (np.abs(one[k]) >= 2.0 ** -126) | (one[k] == 0)
        assert normal.mean() >= 0.999
        assert _same_bits((one[k] * np.float32(1024))[normal], big[k][normal]) and np.abs(big[k]).max() > 0


@pytest.mark.parametrize("C", [5, 65])
def test_softdice_reproducible_and_symmetric_in_the_branches(C):
    """Two runs are bit-identical; 2ab and (a + b)^2 are symmetric in fp32, so swapping the branches gives the same loss and dice
    and the swapped gradients, bit for bit (generic kernels)."""
    la, lb = _inputs(2, C, 301, seed=5)
    r1, r2, sw = _softdice_abi(la, lb), _softdice_abi(la, lb), _softdice_abi(lb, la)
    assert all(_same_bits(r1[k], r2[k]) for k in ("loss", "dice", "ga", "gb"))
    assert _same_bits(r1["loss"], sw["loss"]) and _same_bits(r1["dice"], sw["dice"])
    assert _same_bits(r1["ga"], sw["gb"]) and _same_bits(r1["gb"], sw["ga"])
    assert not _same_bits(r1["ga"], r1["gb"])


def test_softdice_16_classes_both_ways_are_reproducible_and_different_kernels(monkeypatch):
    """DGTTA_SOFTDICE16 really switches: the quad-tree sums of the 16-class kernels and the sequential sums of the generic ones
    differ in the last bits somewhere (were the switch dead, both ways would run the same kernels and every 16-class case above
    would pass twice on one of them)."""
    la, lb = _inputs(2, 16, 301, seed=5)
    out = {}
    for way in ("generic", "16"):
        _set16(monkeypatch, way == "16")
        r1, r2 = _softdice_abi(la, lb), _softdice_abi(la, lb)
        assert all(_same_bits(r1[k], r2[k]) for k in ("loss", "dice", "ga", "gb"))
        out[way] = r1
    assert not all(_same_bits(out["generic"][k], out["16"][k]) for k in ("loss", "dice", "ga", "gb"))
    assert np.abs(out["generic"]["ga"] - out["16"]["ga"]).max() <= 1e-5 * np.abs(out["16"]["ga"]).max()


@pytest.mark.parametrize("C", [5, 33])
def test_consistency_loss_pair_form_equals_the_two_tensor_form(C):
    """ops.consistency_loss on the halves of one batched tensor (C != 16) against the two-tensor form: the same bits, and both
    within the yardstick of float64."""
    from dg_tta_amd import ops
    B, shp = 2, (5, 6, 9)
    la, lb = _inputs(B, C, 270, seed=9)
    ta, tb = (torch.from_numpy(x.astype(np.float32)).reshape(B, C, *shp) for x in (la, lb))
    da = ta.to(DEV).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    db = tb.to(DEV).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    loss, dice = ops.consistency_loss(da, db, 1)
    (loss * 0.5).backward()
    both = torch.cat([ta, tb]).to(DEV).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    pa, pb = both[:B], both[B:]
    pa._dgtta_pair = pb._dgtta_pair = both
    loss2, dice2 = ops.consistency_loss(pa, pb, 1)
    (loss2 * 0.5).backward()
    assert torch.equal(loss, loss2) and torch.equal(dice, dice2)
    assert torch.equal(both.grad[:B], da.grad) and torch.equal(both.grad[B:], db.grad)
    got = dict(loss=float(loss.detach()), dice=dice.cpu().numpy(), ga=da.grad.cpu().numpy().reshape(B, C, -1) * 2,
               gb=db.grad.cpu().numpy().reshape(B, C, -1) * 2)
    _judge(f"consistency_loss C {C}", got, *_softdice_refs(la, lb, 1, None))


# ================================================================================================ soft Dice: argument checks
def test_softdice_argument_checks():
    from dg_tta_amd._lib import DgttaError
    lib, check, st = _lib_and_stream()
    assert lib.dgtta_softdice_ws_bytes(0, 5, 100) == 0 and lib.dgtta_softdice_ws_bytes(2, 0, 100) == 0
    assert lib.dgtta_softdice_ws_bytes(2, 5, 0) == 0
    t = torch.zeros(9 * 129 * 4 * 2, dtype=torch.float32, device=DEV)
    need = lib.dgtta_softdice_ws_bytes(2, 5, 4)
    ws = torch.empty(lib.dgtta_softdice_ws_bytes(8, 128, 4), dtype=torch.uint8, device=DEV)
    p = t.data_ptr()

    def fwd(B=2, C=5, ldc=5, start=1, guard=2, nbytes=None):
        nb = lib.dgtta_softdice_ws_bytes(min(B, 8), min(C, 128), 4) if nbytes is None else nbytes
        check(lib.dgtta_softdice_fwd(p, p, p, p, ws.data_ptr(), nb, B, C, 4, ldc, start, guard, st), "dgtta_softdice_fwd")
    fwd()
    for kw, code in ((dict(B=9, guard=9), -1), (dict(C=129, ldc=129), -1), (dict(ldc=4), -1), (dict(start=5), -1),
                     (dict(start=-1), -1), (dict(B=4, guard=3), -1), (dict(guard=0), -1), (dict(nbytes=need - 1), -3)):
        with pytest.raises(DgttaError, match=rf"code {code}\)"):
            fwd(**kw)
    for B, C, ldc in ((9, 5, 5), (2, 129, 129), (2, 5, 4)):
        with pytest.raises(DgttaError, match=r"code -1\)"):
            check(lib.dgtta_softdice_bwd(p, p, p, p, ws.data_ptr(), 1.0, None, B, C, 4, ldc, 1, st), "dgtta_softdice_bwd")
    with pytest.raises(DgttaError, match=r"code -1\)"):
        check(lib.dgtta_softdice_probs_fwd(p, p, p, ws.data_ptr(), ws.numel(), 9, 5, 4, 20, 4, 1, st), "dgtta_softdice_probs_fwd")
    with pytest.raises(DgttaError, match=r"code -3\)"):
        check(lib.dgtta_softdice_probs_fwd(p, p, p, ws.data_ptr(), need - 1, 2, 5, 4, 20, 4, 1, st), "dgtta_softdice_probs_fwd")
    torch.cuda.synchronize()


# ================================================================================================ the probs kernels
P_SLACK = 1.0 + 2.0 ** -16


def _probs_check(name, a, b, gd, dice_k, ga_k, gb_k):
    """Derived bounds of the module docstring; a, b [B][C][V] float64 (fp32 values, non-negative)."""
    B, C, V = a.shape
    for what, x in (("dice", dice_k), ("grad_a", ga_k), ("grad_b", gb_k)):
        assert np.all(np.isfinite(x)), f"{name}: the kernel's {what} is not finite"
    d = loss_ref.softdice_probs(a, b)
    r_d = float(np.max(np.abs(dice_k - d) / (158 * U * P_SLACK * np.abs(d))))
    nom, den = (2 * a * b).mean(2), 0.5 * ((a + b) ** 2).mean(2)
    P, Q = (gd * 2 / (V * den))[:, :, None], (-gd * nom / (den * den * V))[:, :, None]
    t = Q * (a + b)
    ga, gb = loss_ref.softdice_probs_grad(a, b, gd)
    r_g = [0.0]
    for gk, g, other in ((ga_k, ga, b), (gb_k, gb, a)):
        bound = (87 * U * np.abs(P * other) + 246 * U * np.abs(t) + U * np.abs(g)) * P_SLACK
        err = np.abs(gk - g)
        assert np.all(err[bound == 0] == 0)
        r_g.append(float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
    r_g = float(np.max(r_g))
    print(f"\n{name}: error / bound  dice {r_d:.3f}  grad {r_g:.3f}")
    assert r_d <= 1.0 and r_g <= 1.0


def _probs_run(a, b, gd, channels_last):
    from dg_tta_amd import ops
    B, C, V = a.shape
    fmt = torch.channels_last_3d if channels_last else torch.contiguous_format
    ta, tb = (torch.from_numpy(x.astype(np.float32)).reshape(B, C, V, 1, 1).to(DEV).contiguous(memory_format=fmt).requires_grad_(True)
              for x in (a, b))
    if channels_last and C > 1 and V > 1:
        assert not ta.is_contiguous() and ta.stride(1) == 1
    dice = ops.soft_dice(ta, tb)
    (dice * torch.from_numpy(gd.astype(np.float32)).to(DEV)).sum().backward()
    return (dice.detach().cpu().numpy(), ta.grad.cpu().numpy().reshape(B, C, V), tb.grad.cpu().numpy().reshape(B, C, V))


# (with one class or one voxel channels-last and NCDHW are the same memory and ops.soft_dice takes the NCDHW strides: those cases
# are listed once)
@pytest.mark.parametrize("B,C,V,channels_last", [
    (2, 1, 1, False), (3, 5, 1, False),                               # one voxel
    (2, 5, 255, False), (2, 5, 255, True),                            # one short workgroup chunk
    (1, 128, 255, False), (1, 128, 255, True),
    (8, 5, 257, False), (8, 5, 257, True),                            # two workgroups (nblocks_for = 2), slices of 129 and 128
    (1, 128, 257, False), (1, 128, 257, True),
    (2, 5, 16385, False), (2, 5, 16385, True),                        # 65 workgroups of 253 voxels (the last one 193)
    (1, 1, 256 * 64 + 1, False),                                      # (the same volume in one plane)
    (1, 128, 16385, False), (1, 128, 16385, True),
])
def test_softdice_probs_against_the_derived_bound(B, C, V, channels_last):
    rng = np.random.RandomState(B * 31 + C + V)
    a, b = (rng.uniform(size=(B, C, V)).astype(np.float32).astype(np.float64) for _ in range(2))
    gd = rng.standard_normal((B, C)).astype(np.float32).astype(np.float64)
    out = _probs_run(a, b, gd, channels_last)
    _probs_check(f"probs B {B} C {C} V {V} channels_last {channels_last}", a, b, gd, *out)
    again, swapped = _probs_run(a, b, gd, channels_last), _probs_run(b, a, gd, channels_last)
    assert all(_same_bits(x, y) for x, y in zip(out, again))
    assert _same_bits(out[0], swapped[0]) and _same_bits(out[1], swapped[2]) and _same_bits(out[2], swapped[1])


@pytest.mark.parametrize("C,channels_last", [(1, False), (2, True)])
def test_softdice_probs_second_round_of_the_chunk_loop_and_of_the_slice(C, channels_last):
    """V = 256 * 64 * 1024 + 1: nblocks_for caps at 1024 workgroups, a workgroup's slice is 16 385 voxels - the inner 256 * 64
    chunk loop takes a second round (of one voxel) in every workgroup, the only volume at which it does; the backward's 512
    workgroups x 256 threads make 128 grid-stride rounds and one more.  Once with unit voxel stride (one class), once
    channels-last with two classes (voxel stride 2).  Each class plane is checked on its own to bound the host memory."""
    V = 256 * 64 * 1024 + 1
    rng = np.random.RandomState(77 + C)
    a, b = (rng.uniform(size=(1, C, V)).astype(np.float32).astype(np.float64) for _ in range(2))
    gd = np.array([[0.75, -1.5][:C]])
    dice, ga, gb = _probs_run(a, b, gd, channels_last)
    for c in range(C):
        k = slice(c, c + 1)
        _probs_check(f"probs V 16777217 class {c} of {C}", a[:, k], b[:, k], gd[:, k], dice[:, k], ga[:, k], gb[:, k])


def test_softdice_probs_all_zero_guard():
    z, gd = np.zeros((2, 5, 300)), np.ones((2, 5))
    for cl in (False, True):
        dice, ga, gb = _probs_run(z, z, gd, cl)
        assert np.all(dice == 1.0) and not ga.any() and not gb.any()
    one = z.copy()
    one[1, 3, 299] = 0.5                 # a single non-zero voxel anywhere in the call lifts the guard for every (b, c)
    dice, _, _ = _probs_run(one, one, gd, False)
    assert dice[1, 3] == 1.0 and np.isnan(dice[0, 0])


# ================================================================================================ DC + CE
def _dc_inputs(B, C, V, seed=0, ignore_sample=None, all_ignored=False):
    rng = np.random.RandomState(100 * C + B + seed + V % 997)
    z = (rng.standard_normal((B, C, V)) * 3).astype(np.float32).astype(np.float64)
    y = rng.randint(0, C, size=(B, V)).astype(np.int64)
    if C >= 3:
        y[0][y[0] == C - 1] = 0                                   # a class absent from sample 0
    if V >= 8:
        y[0, 1:V:31] = -1                                         # ignored values
        y[0, 2:V:31] = C
        y[B - 1, 3:V:31] = 255
        y[B - 1, 4:V:31] = -2 ** 40
    if ignore_sample is not None:
        y[ignore_sample] = -1
    if all_ignored:
        y[:] = C + 1
    return z, y


def _dice_ce_abi(z, y, smooth=1e-5, do_bg=False, ldc=None, ldg=None, scale_h=1.0, scale_dev=None, dims=None, strides=None):
    """dgtta_dice_ce_fwd + _bwd (or the _ds_ pair when dims = (d, h, w) and strides are given; y is then the full-resolution
    map) through the C ABI -> dict(loss [3], dice [B][C], g [B][C][V], pad)."""
    lib, check, st = _lib_and_stream()
    B, C, V = z.shape
    ldc, ldg = C if ldc is None else ldc, C if ldg is None else ldg
    bz, vz, _ = _rows(B, V, ldc, float("nan"))
    _put(vz, z, ldc)
    yd = torch.from_numpy(np.ascontiguousarray(y)).to(DEV)
    small = torch.full((B * C + 7,), SENT, dtype=torch.float32, device=DEV)           # [guard][dice][guard][loss3][guard]
    dice, loss3 = small[1:1 + B * C], small[B * C + 2:B * C + 5]
    nbytes = lib.dgtta_dice_ce_ws_bytes(B, C, V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    bg, vg, lead = _rows(B, V, ldg, SENT)
    sd = None if scale_dev is None else torch.tensor([scale_dev], dtype=torch.float32, device=DEV)
    sdp = None if sd is None else sd.data_ptr()
    if strides is None:
        check(lib.dgtta_dice_ce_fwd(vz.data_ptr(), ldc, yd.data_ptr(), loss3.data_ptr(), dice.data_ptr(), ws.data_ptr(), nbytes, B, C, V,
                                    smooth, int(do_bg), st), "dgtta_dice_ce_fwd")
        check(lib.dgtta_dice_ce_bwd(vz.data_ptr(), ldc, yd.data_ptr(), ws.data_ptr(), scale_h, sdp, vg.data_ptr(), ldg, B, C, V, st),
              "dgtta_dice_ce_bwd")
    else:
        assert lib.dgtta_dice_ce_ds_ws_bytes(B, C, *dims) == nbytes and dims[0] * dims[1] * dims[2] == V
        check(lib.dgtta_dice_ce_ds_fwd(vz.data_ptr(), ldc, yd.data_ptr(), loss3.data_ptr(), dice.data_ptr(), ws.data_ptr(), nbytes, B, C,
                                       *dims, *strides, smooth, int(do_bg), st), "dgtta_dice_ce_ds_fwd")
        check(lib.dgtta_dice_ce_ds_bwd(vz.data_ptr(), ldc, yd.data_ptr(), ws.data_ptr(), scale_h, sdp, vg.data_ptr(), ldg, B, C, *dims,
                                       *strides, st), "dgtta_dice_ce_ds_bwd")
    torch.cuda.synchronize()
    s = small.cpu().numpy()
    assert s[0] == SENT and s[B * C + 1] == SENT and s[B * C + 5] == SENT and s[B * C + 6] == SENT
    g, pad = _get(bg, lead, B, C, V, ldg, SENT)
    assert np.all(pad == SENT), "the padding columns of the gradient rows were written (the kernel stores C columns per row)"
    return dict(loss=s[B * C + 2:B * C + 5].copy(), dice=s[1:1 + B * C].reshape(B, C).copy(), g=g)


def _dice_ce_case(name, z, y, smooth=1e-5, do_bg=False, **abi):
    got = _dice_ce_abi(z, y, smooth, do_bg, **abi)
    strides = abi.get("strides") or (1, 1, 1)
    zz = z if "dims" not in abi else z.reshape(*z.shape[:2], *abi["dims"])
    ref64 = loss_ref.dice_ce(zz, y, f32(smooth), do_bg, strides)
    ref32 = loss_ref.dice_ce(zz, y, f32(smooth), do_bg, strides, dtype=np.float32)
    flat = lambda r: (np.array(r[0], dtype=np.float64), r[1], r[2].reshape(z.shape))
    _judge(name, got, flat(ref64), flat(ref32), grads=("g",))
    l0, l1, l2 = (float(x) for x in got["loss"])
    assert abs(l0 - (l1 + l2)) <= U * (abs(l0) + abs(l1) + abs(l2))              # three roundings of one double sum
    return got


def f32(x):
    return ctypes.c_float(x).value


@pytest.mark.parametrize("do_bg", [False, True])
@pytest.mark.parametrize("smooth", [1e-5, 0.0])
@pytest.mark.parametrize("B,C,V", [
    (3, 2, 129),          # two classes; one tile and one voxel
    (3, 3, 129),
    (1, 16, 129),
    (3, 105, 129),        # the class count of the full-body plan
    (1, 127, 129),        # odd pitch 127
    (8, 128, 129),        # the `t < C` reduction takes all 128 tile threads; the largest batch
])
def test_dice_ce_class_counts_labels_and_switches(B, C, V, smooth, do_bg):
    """Labels: ignored values -1, C, 255, -2^40; a class absent from sample 0 (dice 0 under smooth = 0); with B >= 3 sample 1 is
    ignored entirely (dice 1 with smooth = 1e-5, 0 / 1e-8 = 0 with smooth = 0 - the clamp of the denominator; gradient 0)."""
    z, y = _dc_inputs(B, C, V, ignore_sample=1 if B >= 3 else None)
    got = _dice_ce_case(f"dice_ce B {B} C {C} V {V} smooth {smooth:g} bg {do_bg}", z, y, smooth, do_bg)
    if B >= 3:
        assert not got["g"][1].any() and np.all(got["dice"][1] == (1.0 if smooth else 0.0))
    if C >= 3 and smooth == 0.0:
        assert got["dice"][0, C - 1] == 0.0
    assert got["g"][0].any()


@pytest.mark.parametrize("V", [1, 127, 128, 1000])
@pytest.mark.parametrize("B,C", [(1, 3), (3, 128)])
def test_dice_ce_volume_sizes(B, C, V):
    """Around one 128-voxel tile; 1000 = eight tiles, the last of 104 voxels (dc_tile_load's eight-deep loop at a short tile)."""
    z, y = _dc_inputs(B, C, V)
    _dice_ce_case(f"dice_ce B {B} C {C} V {V}", z, y)


def test_dice_ce_second_grid_stride_pass():
    """V = 262 144 + 128 + 37 at C = 2: above the forward cap (1024 workgroups x 128 voxels) and the backward cap (2048 x 128)."""
    z, y = _dc_inputs(1, 2, 262144 + 128 + 37)
    _dice_ce_case("dice_ce C 2 V 262309", z, y)


def test_dice_ce_whole_batch_ignored():
    z, y = _dc_inputs(3, 5, 200, all_ignored=True)
    got = _dice_ce_abi(z, y, 1e-5, False)
    assert got["loss"].tolist() == [-1.0, 0.0, -1.0] and np.all(got["dice"] == 1.0) and not got["g"].any()
    got = _dice_ce_abi(z, y, 0.0, True)
    assert got["loss"].tolist() == [0.0, 0.0, 0.0] and np.all(got["dice"] == 0.0) and not got["g"].any()


@pytest.mark.parametrize("C", [5, 16, 128])
@pytest.mark.parametrize("dc,dg", [(0, 0), (3, 0), (0, 1), (4, 4)])
def test_dice_ce_row_pitch(C, dc, dg):
    """(ldc, ldg) = (C + dc, C + dg): the contiguous eight-deep load only at ldc == C, the strided load and store otherwise.  Input padding NaN,
    gradient pre-filled with a sentinel: results bit-identical to dense rows, nothing written outside [B][V][ldg]."""
    ldc, ldg = C + dc, C + dg
    z, y = _dc_inputs(2, C, 300, seed=1)
    got = _dice_ce_case(f"dice_ce C {C} ldc {ldc} ldg {ldg}", z, y, ldc=ldc, ldg=ldg)
    if (dc, dg) != (0, 0):
        plain = _dice_ce_abi(z, y)
        assert all(_same_bits(got[k], plain[k]) for k in ("loss", "dice", "g"))


def test_dice_ce_host_and_device_scale_and_reproducibility():
    z, y = _dc_inputs(2, 16, 300, seed=2)
    one, again = _dice_ce_abi(z, y), _dice_ce_abi(z, y)
    assert all(_same_bits(one[k], again[k]) for k in ("loss", "dice", "g"))
    for kw in (dict(scale_h=1024.0), dict(scale_h=4096.0, scale_dev=0.25), dict(scale_h=1.0, scale_dev=1024.0)):
        big = _dice_ce_abi(z, y, **kw)
        normal = (np.abs(one["g"]) >= 2.0 ** -126) | (one["g"] == 0)
        assert normal.mean() >= 0.999 and _same_bits(one["loss"], big["loss"])
        assert _same_bits((one["g"] * np.float32(1024))[normal], big["g"][normal]) and np.abs(big["g"]).max() > 0


@pytest.mark.parametrize("strides,dims", [((1, 2, 4), (5, 4, 3)), ((3, 3, 3), (2, 5, 7)), ((2, 1, 2), (6, 3, 11)),
                                          ((1, 1, 1), (4, 5, 7))])
def test_dice_ce_strided_labels(strides, dims):
    """The deep-supervision entry points: low-resolution logits against the full-resolution label map read through
    (i sd + sd / 2, j sh + sh / 2, k sw + sw / 2).  Unit strides are the plain entry points bit for bit."""
    from dg_tta_amd import ops
    B, C = 2, 6
    V = dims[0] * dims[1] * dims[2]
    rng = np.random.RandomState(sum(strides) * 10 + V)
    z = (rng.standard_normal((B, C, V)) * 3).astype(np.float32).astype(np.float64)
    full = rng.randint(-1, C + 1, size=(B, *(d * s for d, s in zip(dims, strides)))).astype(np.int64)
    got = _dice_ce_case(f"dice_ce strides {strides}", z, full, dims=dims, strides=strides)
    low = np.ascontiguousarray(full[:, strides[0] // 2::strides[0], strides[1] // 2::strides[1], strides[2] // 2::strides[2]])
    plain = _dice_ce_abi(z, low.reshape(B, V))
    assert all(_same_bits(got[k], plain[k]) for k in ("loss", "dice", "g"))
    # the tensor wrapper reaches the same kernels
    t = torch.from_numpy(z.astype(np.float32)).reshape(B, C, *dims).to(DEV).requires_grad_(True)
    loss, _ = ops.deep_supervision_loss([t], torch.from_numpy(full).to(DEV), weights=[1.0])
    loss.backward()
    assert _same_bits(float(loss.detach()), got["loss"][0])
    assert _same_bits(t.grad.cpu().numpy().reshape(B, C, V), got["g"])


def test_dice_ce_argument_checks():
    from dg_tta_amd._lib import DgttaError
    lib, check, st = _lib_and_stream()
    assert lib.dgtta_dice_ce_ws_bytes(0, 5, 100) == 0 and lib.dgtta_dice_ce_ws_bytes(2, 5, 0) == 0
    assert lib.dgtta_dice_ce_ds_ws_bytes(2, 5, 0, 4, 4) == 0
    t = torch.zeros(8 * 128 * 4 * 2, dtype=torch.float32, device=DEV)
    lab = torch.zeros(8 * 64, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.dgtta_dice_ce_ws_bytes(8, 128, 4), dtype=torch.uint8, device=DEV)
    need = lib.dgtta_dice_ce_ws_bytes(2, 5, 4)
    p, y, w = t.data_ptr(), lab.data_ptr(), ws.data_ptr()

    def fwd(B=2, C=5, ldc=5, nbytes=None):
        check(lib.dgtta_dice_ce_fwd(p, ldc, y, p, p, w, ws.numel() if nbytes is None else nbytes, B, C, 4, 1e-5, 0, st), "fwd")

    def bwd(B=2, C=5, ldc=5, ldg=5):
        check(lib.dgtta_dice_ce_bwd(p, ldc, y, w, 1.0, None, p, ldg, B, C, 4, st), "bwd")
    fwd()
    for kw, code in ((dict(B=9), -1), (dict(B=0), -1), (dict(C=1, ldc=1), -1), (dict(C=129, ldc=129), -1), (dict(ldc=4), -1),
                     (dict(nbytes=need - 1), -3)):
        with pytest.raises(DgttaError, match=rf"code {code}\)"):
            fwd(**kw)
    for kw in (dict(B=9), dict(C=1, ldc=1, ldg=1), dict(C=129, ldc=129, ldg=129), dict(ldc=4), dict(ldg=4)):
        with pytest.raises(DgttaError, match=r"code -1\)"):
            bwd(**kw)
    for dims in ((0, 2, 2, 1, 1, 1), (1, 2, 2, 0, 1, 1), (1, 2, 2, 1, 1, -1)):
        with pytest.raises(DgttaError, match=r"code -1\)"):
            check(lib.dgtta_dice_ce_ds_fwd(p, 5, y, p, p, w, ws.numel(), 2, 5, *dims, 1e-5, 0, st), "ds_fwd")
        with pytest.raises(DgttaError, match=r"code -1\)"):
            check(lib.dgtta_dice_ce_ds_bwd(p, 5, y, w, 1.0, None, p, 5, 2, 5, *dims, st), "ds_bwd")
    torch.cuda.synchronize()

