"""Mirroring on the GPU: the gather / batch-flip kernels bit for bit against torch, every mirrored window accumulation against the
float64 restatement (tests/mirror_ref.py) and against its unmirrored entry, and sliding-window inference with mirror_axes against
the CPU restatement of nnU-Net's mirrored prediction."""
import functools

import pytest
import torch

import mirror_ref as mr

DEV = "cuda:0"
U = 2.0 ** -24                                  # unit roundoff of fp32
# window with odd and even extents, all distinct; ragged volume; three overlapping origins.  The second case has a last axis longer
# than the 64-voxel runs of the head kernels (a mirrored read crosses runs).
CASES = {"p568": ((5, 6, 8), (9, 8, 13), [(0, 0, 0), (2, 1, 3), (4, 2, 5)]),
         "p3x2x70": ((3, 2, 70), (5, 4, 75), [(0, 0, 0), (1, 2, 3), (2, 1, 5)])}
DTYPES = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
BADARG, UNSUPPORTED = -1, -2


def _lib():
    from dg_tta_amd import _lib as L
    return L.load()


def _reference(P, V, origins, mask, g, zs):
    """float64 accumulators of the three windows under `mask`: (acc, nsum, sum |g z|, contributions per voxel)."""
    C = zs[0].shape[-1]
    acc = torch.zeros(*V, C, dtype=torch.float64)
    absacc, nsum = torch.zeros_like(acc), torch.zeros(*V, dtype=torch.float64)
    counts = torch.zeros(*V, dtype=torch.int64)
    for o, z in zip(origins, zs):
        mr.accumulate(acc, nsum, absacc, counts, g.cpu(), z.cpu(), o, mask)
    return acc, nsum, absacc, counts


def _within(got, ref, absref, counts, extra=0):
    """|got - ref| <= (k + 1 + extra) * 2^-24 * sum_i |g_i z_i| on EVERY element: one rounding per product, one per addition (k
    contributions), `extra` roundings inside a contribution."""
    k = counts.double()
    while k.dim() < ref.dim():
        k = k[..., None]
    return bool(((got.cpu().double() - ref).abs() <= (k + 1 + extra) * U * absref).all())


# ------------------------------------------------------------------------------------------------ data movement
@pytest.mark.gpu
def test_window_gather_equals_torch_slicing_and_flip():
    from dg_tta_amd import ops
    P, V, origins = CASES["p568"]
    torch.manual_seed(0)
    vol = torch.randn(2, *V, device=DEV)
    for o in origins:
        got = ops.window_gather(vol, [o] * 8, list(range(8)), P)
        assert torch.equal(got.cpu(), mr.gather(vol.cpu(), [o] * 8, list(range(8)), P))
    # more windows than one launch takes (16), mixed origins and masks
    many = [origins[i % 3] for i in range(37)]
    masks = [(5 * i + 3) % 8 for i in range(37)]
    assert torch.equal(ops.window_gather(vol, many, masks, P).cpu(), mr.gather(vol.cpu(), many, masks, P))
    lib = _lib()
    import ctypes as C
    out = torch.empty(1, 2, *P, device=DEV)
    def rc(origin, mask):
        return lib.dgtta_window_gather(vol.data_ptr(), out.data_ptr(), (C.c_int * 3)(*origin), (C.c_int * 1)(mask), 1, 2, *P, *V, None)
    assert rc((4, 2, 5), 7) == 0
    assert rc((5, 2, 5), 0) == BADARG and rc((0, 3, 0), 0) == BADARG and rc((0, 0, 6), 0) == BADARG and rc((-1, 0, 0), 0) == BADARG
    assert rc((0, 0, 0), 8) == BADARG and rc((0, 0, 0), -1) == BADARG
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_mirror_batch_equals_torch_flip():
    from dg_tta_amd import ops
    torch.manual_seed(1)
    img = torch.randn(3, 2, 5, 6, 8, device=DEV)
    lab = torch.randint(0, 2 ** 40, (3, 5, 6, 8), device=DEV, dtype=torch.int64)       # (values beyond 32 bits)
    masks = [0, 5, 7]
    gi, gl = ops.mirror_batch(img, lab, masks)
    assert gi.data_ptr() != img.data_ptr() and gi.dtype == torch.float32 and gl.dtype == torch.int64
    for b, m in enumerate(masks):
        assert torch.equal(gi[b], mr.flip(img[b], m)) and torch.equal(gl[b], mr.flip(lab[b], m))
    # a batch larger than one launch's 16 items
    big_i, big_l = torch.randn(19, 1, 3, 4, 5, device=DEV), torch.randint(0, 9, (19, 3, 4, 5), device=DEV)
    bm = [(3 * i + 1) % 8 for i in range(19)]
    oi, ol = ops.mirror_batch(big_i, big_l, bm)
    assert all(torch.equal(oi[b], mr.flip(big_i[b], m)) and torch.equal(ol[b], mr.flip(big_l[b], m)) for b, m in enumerate(bm))
    with pytest.raises(ValueError):
        ops.mirror_batch(img, lab, [0, 8, 0])
    with pytest.raises(ValueError):
        ops.mirror_batch(img, lab.int(), masks)
    import ctypes as C
    lib = _lib()
    assert lib.dgtta_mirror_batch(img.data_ptr(), lab.data_ptr(), gi.data_ptr(), gl.data_ptr(), (C.c_int * 3)(0, 9, 0), 3, 2, 5, 6, 8,
                                  None) == BADARG
    assert lib.dgtta_mirror_batch(img.data_ptr(), lab.data_ptr(), img.data_ptr(), gl.data_ptr(), (C.c_int * 3)(0, 1, 0), 3, 2, 5, 6, 8,
                                  None) == BADARG


# ------------------------------------------------------------------------------------------------ mirrored accumulations
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dts", list(DTYPES))
def test_feature_window_accumulate_mirror(dts, case):
    """dgtta_feature_window_accumulate_mirror and its norm-folded form: mask 0 = the unmirrored entry's bits; masks 1..7 within the
    rounding bound of the float64 restatement, and the bits of the unmirrored entry fed the flipped source (the Gaussian stays)."""
    lib = _lib()
    dt, tdt = DTYPES[dts]
    P, V, origins = CASES[case]
    torch.manual_seed(2)
    g = torch.rand(*P, device=DEV) + 0.1                      # positive, no symmetry at all
    zs = [torch.randn(*P, 32, device=DEV).to(tdt) for _ in origins]
    ys = [torch.randn(*P, 32, device=DEV).to(tdt) for _ in origins]
    stats = [torch.stack([torch.randn(32, device=DEV), torch.rand(32, device=DEV) + 0.5], -1).contiguous() for _ in origins]
    gamma, beta = torch.randn(32, device=DEV), torch.randn(32, device=DEV)

    def plain(srcs, mask, entry):
        acc, n = torch.zeros(*V, 32, device=DEV), torch.zeros(*V, device=DEV)
        for o, z in zip(origins, srcs):
            if entry == "mirror":
                rc = lib.dgtta_feature_window_accumulate_mirror(z.data_ptr(), g.data_ptr(), acc.data_ptr(), n.data_ptr(), 32, *P, *V, *o, dt,
                                                                mask, None)
            else:
                rc = lib.dgtta_feature_window_accumulate(z.data_ptr(), g.data_ptr(), acc.data_ptr(), n.data_ptr(), 32, *P, *V, *o, dt, None)
            assert rc == 0
        return acc, n

    def norm(srcs, mask, entry):
        acc, n = torch.zeros(*V, 32, device=DEV), torch.zeros(*V, device=DEV)
        for o, y, s in zip(origins, srcs, stats):
            args = (y.data_ptr(), s.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 0.01, g.data_ptr(), acc.data_ptr(), n.data_ptr(), 32,
                    *P, *V, *o, dt)
            rc = lib.dgtta_feature_window_accumulate_norm_mirror(*args, mask, None) if entry == "mirror" else \
                lib.dgtta_feature_window_accumulate_norm(*args, None)
            assert rc == 0
        return acc, n

    for fn, srcs in ((norm, ys), (plain, zs)):
        a0, n0 = fn(srcs, 0, "mirror")
        a1, n1 = fn(srcs, 0, "plain")                          # (a1 is the unmirrored PLAIN accumulator after the loop)
        assert torch.equal(a0, a1) and torch.equal(n0, n1) and float(a0.abs().max()) > 0
    # the values the norm-folded form accumulates: round_T(lrelu(y * alpha + beta')) with the kernel's own fp32 arithmetic
    zn = []
    for y, s in zip(ys, stats):
        al = s[:, 1] * gamma
        v = y.float() * al + (beta - s[:, 0] * al)
        zn.append(torch.where(v > 0, v, v * 0.01).to(tdt))
    for mask in range(1, 8):
        acc, n = plain(zs, mask, "mirror")
        ref, ref_n, absref, counts = _reference(P, V, origins, mask, g, [z.float() for z in zs])
        assert int(counts.max()) >= 2
        assert _within(acc, ref, absref, counts) and _within(n, ref_n, ref_n, counts)
        flipped = plain([mr.flip(z, mask, first=0).contiguous() for z in zs], 0, "plain")
        assert torch.equal(acc, flipped[0]) and torch.equal(n, flipped[1])
        assert not torch.equal(acc, a1)                        # (it IS mirrored)
        # the norm-folded form against the mirrored plain form on the same values
        acc_n, n_n = norm(ys, mask, "mirror")
        acc_z, n_z = plain(zn, mask, "mirror")
        assert torch.equal(acc_n, acc_z) and torch.equal(n_n, n_z)
    torch.cuda.synchronize()
    # documented error codes
    a, n = torch.zeros(*V, 32, device=DEV), torch.zeros(*V, device=DEV)
    z = zs[0]
    def rc(cin, origin, mask):
        return lib.dgtta_feature_window_accumulate_mirror(z.data_ptr(), g.data_ptr(), a.data_ptr(), n.data_ptr(), cin, *P, *V, *origin, dt, mask,
                                                          None)
    far = (V[0] - P[0] + 1, 0, 0)
    assert rc(32, far, 1) == BADARG and rc(32, (0, 0, V[2] - P[2] + 1), 1) == BADARG and rc(32, (0, -1, 0), 1) == BADARG
    assert rc(32, (0, 0, 0), 8) == BADARG and rc(32, (0, 0, 0), -1) == BADARG and rc(16, (0, 0, 0), 1) == UNSUPPORTED
    args = (ys[0].data_ptr(), stats[0].data_ptr(), gamma.data_ptr(), beta.data_ptr(), 0.01, g.data_ptr(), a.data_ptr(), n.data_ptr())
    assert lib.dgtta_feature_window_accumulate_norm_mirror(*args, 32, *P, *V, *far, dt, 1, None) == BADARG
    assert lib.dgtta_feature_window_accumulate_norm_mirror(*args, 32, *P, *V, 0, 0, 0, dt, 8, None) == BADARG
    assert lib.dgtta_feature_window_accumulate_norm_mirror(*args, 16, *P, *V, 0, 0, 0, dt, 1, None) == UNSUPPORTED
    assert float(a.abs().max()) == 0.0                        # a refused call launches nothing


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_window_accumulate_mirror_t(case):
    """The plain logits-space form: fp32 logits [P, C] into the fp32 accumulator."""
    lib = _lib()
    P, V, origins = CASES[case]
    C = 7
    torch.manual_seed(3)
    g = torch.rand(*P, device=DEV) + 0.1
    zs = [torch.randn(*P, C, device=DEV) for _ in origins]

    def run(srcs, mask, entry, acc_dtype=torch.float32):
        acc, n = torch.zeros(*V, C, device=DEV, dtype=acc_dtype), torch.zeros(*V, device=DEV)
        code = 0 if acc_dtype == torch.float32 else 2
        for o, z in zip(origins, srcs):
            if entry == "mirror":
                rc = lib.dgtta_window_accumulate_mirror_t(z.data_ptr(), g.data_ptr(), acc.data_ptr(), n.data_ptr(), C, *P, *V, *o, code, mask, None)
            else:
                rc = lib.dgtta_window_accumulate_t(z.data_ptr(), g.data_ptr(), acc.data_ptr(), n.data_ptr(), C, *P, *V, *o, code, None)
            assert rc == 0
        return acc, n

    a0, n0 = run(zs, 0, "mirror")
    a1, n1 = run(zs, 0, "plain")
    assert torch.equal(a0, a1) and torch.equal(n0, n1)
    for mask in range(1, 8):
        acc, n = run(zs, mask, "mirror")
        ref, ref_n, absref, counts = _reference(P, V, origins, mask, g, zs)
        assert _within(acc, ref, absref, counts) and _within(n, ref_n, ref_n, counts)
        flipped = run([mr.flip(z, mask, first=0).contiguous() for z in zs], 0, "plain")
        assert torch.equal(acc, flipped[0]) and torch.equal(n, flipped[1]) and not torch.equal(acc, a1)
    torch.cuda.synchronize()
    a, n, z = torch.zeros(*V, C, device=DEV), torch.zeros(*V, device=DEV), zs[0]
    def rc(origin, mask, code=0):
        return lib.dgtta_window_accumulate_mirror_t(z.data_ptr(), g.data_ptr(), a.data_ptr(), n.data_ptr(), C, *P, *V, *origin, code, mask, None)
    assert rc((V[0] - P[0] + 1, 0, 0), 1) == BADARG and rc((0, 0, 0), 8) == BADARG and rc((0, 0, 0), -2) == BADARG
    assert rc((0, 0, 0), 1, code=2) == UNSUPPORTED            # fp16 accumulators are not mirrored into
    assert float(a.abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["mfma", "fma"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dts", ["bf16", "fp16"])
def test_seghead_window_accumulate_mirror_t(dts, case, kernel, monkeypatch):
    """The head fused with the mirrored accumulation (both head kernels).  Reference: logits = w z + b in float64 from the stored
    16-bit features, then the mirrored accumulation.  Bound: a contribution g * (w . z + b) carries the roundings of its dot product
    on top of the product's and the addition's - the vector-ALU kernel one per channel and one for the bias (33), the matrix-core
    kernel one per channel and weight term (3 x 32: the fp32 weights enter as three 16-bit terms) and the bias (97); 100 covers both -
    against sum |g| (sum_k |w_k z_k| + |b|)."""
    from conftest import reload_kernel_switches
    monkeypatch.setenv("DGTTA_HA_MFMA", "1" if kernel == "mfma" else "0")
    reload_kernel_switches()
    try:
        lib = _lib()
        dt, tdt = DTYPES[dts]
        P, V, origins = CASES[case]
        C = 21                                                # odd, two class groups of 16
        torch.manual_seed(4)
        g = torch.rand(*P, device=DEV) + 0.1
        zs = [torch.randn(*P, 32, device=DEV).to(tdt) for _ in origins]
        w, b = torch.randn(C, 32, device=DEV) * 0.3, torch.randn(C, device=DEV)

        def run(srcs, mask, entry):
            acc, n = torch.zeros(*V, C, device=DEV), torch.zeros(*V, device=DEV)
            for o, z in zip(origins, srcs):
                args = (z.data_ptr(), w.data_ptr(), b.data_ptr(), g.data_ptr(), acc.data_ptr(), n.data_ptr(), 32, C, *P, *V, *o, dt, 0)
                rc = lib.dgtta_seghead_window_accumulate_mirror_t(*args, mask, None) if entry == "mirror" else \
                    lib.dgtta_seghead_window_accumulate_t(*args, None)
                assert rc == 0
            return acc, n

        a0, n0 = run(zs, 0, "mirror")
        a1, n1 = run(zs, 0, "plain")
        assert torch.equal(a0, a1) and torch.equal(n0, n1) and float(a0.abs().max()) > 0
        wd, bd = w.cpu().double(), b.cpu().double()
        logits = [z.cpu().double() @ wd.t() + bd for z in zs]
        mags = [z.cpu().double().abs() @ wd.abs().t() + bd.abs() for z in zs]
        for mask in range(1, 8):
            acc, n = run(zs, mask, "mirror")
            ref, ref_n, _, counts = _reference(P, V, origins, mask, g, logits)
            absref = _reference(P, V, origins, mask, g, mags)[0]
            assert _within(acc, ref, absref, counts, extra=100) and _within(n, ref_n, ref_n, counts)
            flipped = run([mr.flip(z, mask, first=0).contiguous() for z in zs], 0, "plain")
            assert torch.equal(acc, flipped[0]) and torch.equal(n, flipped[1]) and not torch.equal(acc, a1)
        torch.cuda.synchronize()
        a, n, z = torch.zeros(*V, C, device=DEV), torch.zeros(*V, device=DEV), zs[0]
        def rc(cin, origin, mask, acc_code=0):
            return lib.dgtta_seghead_window_accumulate_mirror_t(z.data_ptr(), w.data_ptr(), b.data_ptr(), g.data_ptr(), a.data_ptr(),
                                                                n.data_ptr(), cin, C, *P, *V, *origin, dt, acc_code, mask, None)
        assert rc(32, (0, V[1] - P[1] + 1, 0), 1) == BADARG and rc(32, (0, 0, 0), 8) == BADARG and rc(32, (0, 0, 0), -1) == BADARG
        assert rc(16, (0, 0, 0), 1) == UNSUPPORTED and rc(32, (0, 0, 0), 1, acc_code=2) == UNSUPPORTED
        assert float(a.abs().max()) == 0.0
    finally:
        monkeypatch.undo()
        reload_kernel_switches()


# Every window entry of the C ABI: (the arguments it takes of c = Cin, a = acc_dtype, m = mirror; call(lib, t, P, origin, mask, cin,
# acc_code)).  16-bit sources are bf16 (dtype code 1); the multi entry is given one whole window (zoff 0, seg_len = PW).
def _multi(L, t, P, o, mask, cin, acc):
    import ctypes as C
    return L.dgtta_feature_window_accumulate_multi((C.c_void_p * 1)(t.z), (C.c_void_p * 1)(t.mr), (C.c_int * 1)(0), 1, t.gamma, t.beta, 0.01,
                                                   t.g, t.acc, t.n, cin, *P, P[2], *t.V, *o, 1, None)


WINDOW_ENTRIES = {
    "dgtta_window_accumulate": ("", lambda L, t, P, o, mask, cin, acc:
                                L.dgtta_window_accumulate(t.patch, t.g, t.acc, t.n, t.C, *P, *t.V, *o, None)),
    "dgtta_window_accumulate_t": ("a", lambda L, t, P, o, mask, cin, acc:
                                  L.dgtta_window_accumulate_t(t.patch, t.g, t.acc, t.n, t.C, *P, *t.V, *o, acc, None)),
    "dgtta_window_accumulate_mirror_t": ("am", lambda L, t, P, o, mask, cin, acc:
                                         L.dgtta_window_accumulate_mirror_t(t.patch, t.g, t.acc, t.n, t.C, *P, *t.V, *o, acc, mask, None)),
    "dgtta_seghead_window_accumulate": ("c", lambda L, t, P, o, mask, cin, acc:
                                        L.dgtta_seghead_window_accumulate(t.z, t.w, t.b, t.g, t.acc, t.n, cin, t.C, *P, *t.V, *o, 1, None)),
    "dgtta_seghead_window_accumulate_t": ("ca", lambda L, t, P, o, mask, cin, acc:
                                          L.dgtta_seghead_window_accumulate_t(t.z, t.w, t.b, t.g, t.acc, t.n, cin, t.C, *P, *t.V, *o, 1, acc,
                                                                              None)),
    "dgtta_seghead_window_accumulate_mirror_t": ("cam", lambda L, t, P, o, mask, cin, acc:
                                                 L.dgtta_seghead_window_accumulate_mirror_t(t.z, t.w, t.b, t.g, t.acc, t.n, cin, t.C, *P, *t.V,
                                                                                            *o, 1, acc, mask, None)),
    "dgtta_feature_window_accumulate": ("c", lambda L, t, P, o, mask, cin, acc:
                                        L.dgtta_feature_window_accumulate(t.z, t.g, t.acc, t.n, cin, *P, *t.V, *o, 1, None)),
    "dgtta_feature_window_accumulate_mirror": ("cm", lambda L, t, P, o, mask, cin, acc:
                                               L.dgtta_feature_window_accumulate_mirror(t.z, t.g, t.acc, t.n, cin, *P, *t.V, *o, 1, mask, None)),
    "dgtta_feature_window_accumulate_norm": ("c", lambda L, t, P, o, mask, cin, acc:
                                             L.dgtta_feature_window_accumulate_norm(t.z, t.mr, t.gamma, t.beta, 0.01, t.g, t.acc, t.n, cin, *P,
                                                                                    *t.V, *o, 1, None)),
    "dgtta_feature_window_accumulate_norm_mirror": ("cm", lambda L, t, P, o, mask, cin, acc:
                                                    L.dgtta_feature_window_accumulate_norm_mirror(t.z, t.mr, t.gamma, t.beta, 0.01, t.g, t.acc,
                                                                                                  t.n, cin, *P, *t.V, *o, 1, mask, None)),
    "dgtta_feature_window_accumulate_multi": ("c", _multi),
}


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(WINDOW_ENTRIES))
def test_window_entries_refuse_bad_places_with_their_codes(entry):
    """Every window entry on p568: a window outside the volume (one voxel too far on each axis, a negative origin, a zero patch extent) and
    a mirror mask outside 0..7 are DGTTA_ERR_BADARG, Cin = 16 and a fp16 accumulator with a non-zero mask DGTTA_ERR_UNSUPPORTED - for the
    arguments the entry takes - and a refused call launches nothing.  (The accumulators are the middle of a larger zeroed buffer:
    a launch that slipped through would show there, not beyond the allocation.)"""
    import types
    lib = _lib()
    takes, call = WINDOW_ENTRIES[entry]
    P, V, _ = CASES["p568"]
    torch.manual_seed(5)
    C = 7
    big_a, big_n = torch.zeros(V[0] + 4, V[1], V[2], 32, device=DEV), torch.zeros(V[0] + 4, V[1], V[2], device=DEV)
    tensors = dict(patch=torch.randn(*P, C, device=DEV), z=torch.randn(*P, 32, device=DEV).to(torch.bfloat16),
                   g=torch.rand(*P, device=DEV) + 0.1, w=torch.randn(C, 32, device=DEV), b=torch.randn(C, device=DEV),
                   mr=torch.stack([torch.randn(32, device=DEV), torch.rand(32, device=DEV) + 0.5], -1).contiguous(),
                   gamma=torch.randn(32, device=DEV), beta=torch.randn(32, device=DEV), acc=big_a[2:], n=big_n[2:])
    t = types.SimpleNamespace(V=V, C=C, **{k: v.data_ptr() for k, v in tensors.items()})

    def rc(P=P, o=(0, 0, 0), mask=0, cin=32, acc=0):
        return call(lib, t, P, o, mask, cin, acc)

    for axis in range(3):
        far, neg, flat = [0, 0, 0], [0, 0, 0], list(P)
        far[axis], neg[axis], flat[axis] = V[axis] - P[axis] + 1, -1, 0
        assert rc(o=far) == BADARG and rc(o=neg) == BADARG and rc(P=flat) == BADARG
    if "m" in takes:
        assert rc(mask=8) == BADARG and rc(mask=-1) == BADARG
    if "c" in takes:
        assert rc(cin=16) == UNSUPPORTED
    if "a" in takes and "m" in takes:
        assert rc(mask=1, acc=2) == UNSUPPORTED
    torch.cuda.synchronize()
    assert float(big_a.abs().max()) == 0.0 and float(big_n.abs().max()) == 0.0
    assert rc(o=(V[0] - P[0], V[1] - P[1], V[2] - P[2]), mask=7 if "m" in takes else 0) == 0      # (the call itself is well formed)
    torch.cuda.synchronize()
    assert float(big_a[2:].abs().max()) > 0 and float(big_n[2:].min()) >= 0 and float(big_n[2:].max()) > 0
    assert float(big_a[:2].abs().max()) == 0.0 and float(big_a[2 + V[0]:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ network level
FEAT32_1CH =dict(features=(32, 40), strides=(1, 2), n_conv_enc=(2, 2), n_conv_dec=(2,), in_channels=1, num_classes=9)


def _small_1ch():
    from conftest import SMALL_CFG
    return dict(SMALL_CFG, in_channels=1)


@functools.lru_cache(maxsize=None)
def _network_case(cfg_name):
    """(cfg, data, patch, members, reference logits with mirroring along (0, 1, 2)) - computed once on the CPU, shared, unchanged."""
    from oracle import inference as oinf, unet as ounet
    cfg = FEAT32_1CH if cfg_name == "feat32" else _small_1ch()
    torch.manual_seed(0)
    data = torch.randn(1, 24, 20, 28)
    patch = [16, 16, 16]
    members = [ounet.perturb_affine(ounet.init_he(ounet.PlainConvUNetOracle(cfg), s), s + 1) for s in (1, 2)]
    ref = oinf.ensemble_logits([mr.mirrored(m, (0, 1, 2)) for m in members], data, patch)
    return cfg, data, patch, members, ref


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name", ["feat32", "small"])
def test_mirrored_sliding_window_matches_cpu_restatement(cfg_name):
    """12 windows x 8 mirrored passes, two members: feature-space accumulator (feat32) and logits-space accumulator (small)."""
    from dg_tta_amd.tta import inference as pinf
    from dg_tta_amd.unet import HipPlainConvUNet
    cfg, data, patch, members, ref = _network_case(cfg_name)
    params = [m.state_dict() for m in members]
    net = HipPlainConvUNet(cfg, conv_impl=1).to(DEV)
    with torch.no_grad():
        assert pinf._can_accumulate_features(net) == (cfg_name == "feat32")
    acc, nsum, crop = pinf.predict_ensemble(data, net, params, patch, mirror_axes=(0, 1, 2))
    logits = acc.logits() if cfg_name == "feat32" else acc
    got = (logits / nsum[..., None] / len(members))[tuple(crop)].permute(3, 0, 1, 2).cpu().double()
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{cfg_name}: max |logits - ref| = {err:.3e} = {err / scale:.3e} max |ref|")
    assert err < 2e-4 * scale
    seg = pinf.run_inference(data, net, params, patch, mirror_axes=(0, 1, 2))
    assert tuple(seg.shape) == (24, 20, 28) and seg.dtype == torch.int64
    top2 = ref.topk(2, dim=0).values
    safe = (top2[0] - top2[1]) > 1e-3
    ref_seg = ref.argmax(0)
    print(f"{cfg_name}: {1 - float(safe.float().mean()):.4%} of the voxels excluded as near-ties")
    assert float((~safe).float().mean()) <= 0.005
    assert torch.equal(seg[safe], ref_seg[safe])
    # mirroring matters on these inputs: the unmirrored prediction is NOT the mirrored reference
    plain = pinf.run_inference(data, net, params, patch, mirror_axes=None)
    agree = float((plain == ref_seg).float().mean())
    print(f"{cfg_name}: unmirrored labels agree with the mirrored reference on {agree:.3f} of the voxels")
    assert agree < 0.9
    assert torch.equal(plain, pinf.run_inference(data, net, params, patch))          # (None is the default)


@pytest.mark.gpu
def test_mirroring_along_one_axis():
    """mirror_axes=(2,): two passes per window - nsum is twice the unmirrored one, the result the two-pass restatement.
    "Twice" up to the order of the additions: a voxel's weight is a sum of at most 16 positive fp32 terms here (8 windows x 2
    passes, added window by window in one path and mirrored-passes-first in the other), each addition rounds once, so two orders
    differ by at most 2 x 15 roundings: 32 x 2^-24 relative."""
    from dg_tta_amd.tta import inference as pinf
    from dg_tta_amd.unet import HipPlainConvUNet
    from oracle import inference as oinf
    cfg, data, patch, members, _ = _network_case("feat32")
    net = HipPlainConvUNet(cfg, conv_impl=1).to(DEV)
    net.load_state_dict(members[0].state_dict())
    facc, nsum, crop = pinf.accumulate_window_features(net, data, patch, mirror_axes=(2,))
    _, nsum0, _ = pinf.accumulate_window_features(net, data, patch)
    assert float(((nsum - 2 * nsum0).abs() / nsum).max()) <= 32 * U and float(nsum0.min()) > 0
    acc, nsum_l, _ = pinf.predict_sliding_window_return_logits(net, data, patch, acc_dtype=torch.float32, mirror_axes=(2,))
    assert float(((nsum_l - nsum).abs() / nsum).max()) <= 32 * U
    ref = oinf.ensemble_logits([mr.mirrored(members[0], (2,))], data, patch)
    head = net.decoder.seg_layers[-1]
    feats = pinf.WindowFeatures(facc[None], nsum, crop, head.weight.detach().reshape(1, 9, 32).float(), head.bias.detach().float()[None])
    for name, logits, n in (("features", feats.logits(), nsum), ("logits", acc, nsum_l)):
        got = (logits / n[..., None])[tuple(crop)].permute(3, 0, 1, 2).cpu().double()
        err = float((got - ref).abs().max())
        print(f"{name}: max |logits - ref| = {err:.3e} = {err / float(ref.abs().max()):.3e} max |ref|")
        assert err < 2e-4 * float(ref.abs().max())


@pytest.mark.gpu
def test_mind_prefetch_with_explicit_mirror_axes(monkeypatch):
    """A hooked (MIND) model called with explicit mirror_axes: the side-stream prefetch gathers the FLIPPED windows and computes
    their descriptor one batch ahead - the accumulators are those of the in-line path, bit for bit, and they are the mean over
    the mirrors of the CPU members on the descriptor of the flipped window (zero noise weighting on both sides)."""
    from conftest import SMALL_CFG
    from dg_tta_amd.mind import kernel_noise, mind_hook
    from dg_tta_amd.tta import inference as pinf
    from dg_tta_amd.unet import HipPlainConvUNet
    from oracle import inference as oinf, mind as omind, unet as ounet
    patch = [16, 16, 16]
    data = torch.randn(1, 24, 16, 28, generator=torch.Generator().manual_seed(0))
    member = ounet.perturb_affine(ounet.init_he(ounet.PlainConvUNetOracle(SMALL_CFG), 1), 2)
    net = HipPlainConvUNet(SMALL_CFG, conv_impl=1).to(DEV)
    net.register_forward_pre_hook(mind_hook)
    axes = (0, 2)
    assert 2 * 3 * len(mr.subsets(axes)) > pinf.WINDOW_BATCH      # more than one window batch: something IS prefetched
    from dg_tta_amd.utils import disable_internal_augmentation
    disable_internal_augmentation()                               # inference runs with it off (tta_main); the prefetch requires it
    outs = {}
    for prefetch in ("1", "0"):
        monkeypatch.setenv("DGTTA_INFER_PREFETCH", prefetch)
        assert pinf._mind_ahead_ok(net, DEV) == (prefetch == "1")
        with kernel_noise(1234):
            acc, nsum, crop = pinf.predict_ensemble(data, net, [member.state_dict()], patch, mirror_axes=axes)
        outs[prefetch] = (acc.clone(), nsum.clone())
    assert torch.equal(outs["1"][0], outs["0"][0]) and torch.equal(outs["1"][1], outs["0"][1])
    # without noise the descriptor is a function of the (flipped) window alone: compare with the CPU restatement
    net2 = HipPlainConvUNet(SMALL_CFG, conv_impl=1).to(DEV)
    from dg_tta_amd.mind import MIND3D
    net2.register_forward_pre_hook(lambda mod, inp: MIND3D(randn_weighting=0.0).forward(*inp))
    acc, nsum, crop = pinf.predict_ensemble(data, net2, [member.state_dict()], patch, mirror_axes=axes)
    zeros = torch.zeros(1, 12, *patch)
    ref = oinf.ensemble_logits([mr.mirrored(lambda x: member(omind.mind3d(x, zeros, randn_weighting=0.0)), axes)], data, patch)
    got = (acc / nsum[..., None])[tuple(crop)].permute(3, 0, 1, 2).cpu().double()
    err = float((got - ref).abs().max())
    print(f"MIND on the flipped window: max |logits - ref| = {err:.3e} = {err / float(ref.abs().max()):.3e} max |ref|")
    assert err < 2e-4 * float(ref.abs().max())
