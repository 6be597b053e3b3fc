"""GPU: dgtta_region_counts (csrc/region_map.hip; ops.region_counts) - TP / FP / FN per region of the hard prediction z > 0 over
the valid voxels - against tests/region_ref.py, bit-equal (integer sums).  The logits are exact binary fractions (multiples of
1/4) and include exact zeros: a zero is "not predicted".  Label edge cases as in tests/test_gpu_region_loss.py: -1, L, 255,
-2^40, a sample ignored entirely, a region absent from a sample, the whole batch ignored."""
import numpy as np
import pytest
import torch

import region_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _nested_table(R):
    from dg_tta_amd.labels import membership_table
    return membership_table(tuple(tuple(range(r + 1, R + 1)) for r in range(R)))


def _inputs(B, R, shape, seed=0, ignore_sample=None, all_ignored=False):
    rng = np.random.RandomState(7 * R + B + seed)
    table = _nested_table(R)
    L, V = table.size, int(np.prod(shape))
    z = np.clip(np.round(rng.standard_normal((B, R, V)) * 4) / 4, -8, 8)
    assert (z == 0).mean() > 0.02
    y = rng.randint(0, L, size=(B, V)).astype(np.int64)
    if R >= 2:
        y[0][y[0] == R] = 0
    if V >= 8:
        y[0, 1:V:31] = -1
        y[0, 2:V:31] = L
        y[B - 1, 3:V:31] = 255
        y[B - 1, 4:V:31] = -2 ** 40
    if ignore_sample is not None:
        y[ignore_sample] = -1
    if all_ignored:
        y[:] = L
    return z, y, table


def _run(z, y, table, shape):
    from dg_tta_amd import ops
    B, R = z.shape[:2]
    t = torch.from_numpy(z.astype(np.float32)).reshape(B, R, *shape).to(DEV)
    return ops.region_counts(t, torch.from_numpy(y).reshape(B, *shape).to(DEV), table).cpu().numpy()


@pytest.mark.parametrize("B,R,shape", [
    (1, 1, (1, 1, 1)),            # one voxel, one region
    (3, 1, (3, 5, 7)),            # less than one wave per sample
    (3, 3, (4, 8, 9)),            # 288 voxels per sample: more than one workgroup pass over the batch
    (2, 31, (5, 6, 11)),
    (8, 32, (3, 7, 13)),          # every bit of the table
    (1, 2, (8, 256, 257)),        # 526 336 voxels = 2048 workgroups x 256 and 2048 more: a second grid-stride pass for eight of them
])
def test_counts_equal_the_reference(B, R, shape):
    z, y, table = _inputs(B, R, shape, ignore_sample=1 if B >= 3 else None)
    got = _run(z, y, table, shape)
    want = region_ref.region_counts(z, y, table)
    assert got.dtype == np.int64 and got.shape == (3, R) and np.array_equal(got, want), (got, want)
    if np.prod(shape) >= 100:
        assert want[0].sum() > 0 and want[1].sum() > 0 and want[2].sum() > 0
    assert np.array_equal(_run(z, y, table, shape), got)


def test_an_exact_zero_is_not_predicted():
    table = _nested_table(2)
    z = np.zeros((1, 2, 64))
    y = np.full((1, 64), 2, dtype=np.int64)
    assert _run(z, y, table, (4, 4, 4)).tolist() == [[0, 0], [0, 0], [64, 64]]
    z[0, 0, :5] = 0.25
    z[0, 1, :3] = -0.0
    assert _run(z, y, table, (4, 4, 4)).tolist() == [[5, 0], [0, 0], [59, 64]]


def test_whole_batch_ignored_counts_nothing():
    z, y, table = _inputs(2, 3, (4, 5, 6), all_ignored=True)
    assert not _run(z, y, table, (4, 5, 6)).any()


def test_row_pitch_and_argument_checks():
    """ldc > R through the C ABI (NaN padding columns must not be read as outputs), and the argument checks."""
    from dg_tta_amd import _lib
    from dg_tta_amd._lib import DgttaError
    lib, st = _lib.load(), _lib.stream_of(torch.device(DEV))
    z, y, table = _inputs(2, 3, (300,), seed=3)
    rows = np.full((600, 5), np.nan, np.float32)
    rows[:, :3] = z.transpose(0, 2, 1).reshape(600, 3)
    zd, yd = torch.from_numpy(rows).to(DEV), torch.from_numpy(y.reshape(-1)).to(DEV)
    td = torch.from_numpy(table.view(np.int32).copy()).to(DEV)
    counts = torch.full((11,), -5, dtype=torch.int64, device=DEV)
    c = counts[1:10]

    def call(R=3, ldc=5, L=None, n=600, zp=zd.data_ptr()):
        _lib.check(lib.dgtta_region_counts(zp, ldc, R, yd.data_ptr(), td.data_ptr(), table.size if L is None else L, c.data_ptr(), n, st),
                   "dgtta_region_counts")
    call()
    torch.cuda.synchronize()
    assert counts[0] == -5 and counts[10] == -5
    assert np.array_equal(c.cpu().numpy().reshape(3, 3), region_ref.region_counts(z, y, table))
    for kw in (dict(R=0), dict(R=33, ldc=33), dict(ldc=2), dict(L=0), dict(L=1025), dict(n=0), dict(zp=None)):
        with pytest.raises(DgttaError, match=r"code -1\)"):
            call(**kw)
    torch.cuda.synchronize()
