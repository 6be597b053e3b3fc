"""Execution of HipPlainConvUNet (unet.py) by the HIP kernels, forward AND backward, as one autograd node.

`_plan` lists the layer executors of a pass (`_ConvLayer`, `_UpLayer`): each owns the choice of the C-ABI family that runs it
and keeps what the forward leaves for the backward; `_UNetFn.forward` / `.backward` are sequences of steps over them.

Data layout in HBM: activations are channels-last [B][D][H][W][C] (fp32, or bf16 / fp16 storage with fp32 accumulation);
`torch.cat((up, skip), 1)` never happens: the transposed conv writes the first channel half of a pre-allocated
[.., 2C] buffer and the encoder's InstanceNorm+LeakyReLU writes the skip directly into the second half.
"""
import collections
import contextlib
import ctypes as C
import os

import torch

from . import _lib
from ._lib import check, ptr, stream_of
from ._state import state_of
from .ops import F32, F16, _ws, dtype_code

EPS, SLOPE = 1e-5, 1e-2


def _wgrad_on_side_stream():
    return os.environ.get("DGTTA_WGRAD_STREAM", "1") != "0"


def _pad(c, m):
    return (c + m - 1) // m * m


def _k3(k):
    return tuple(k) if isinstance(k, (tuple, list)) else (k, k, k)


def _odim(i, s):
    return (i + 2 - 3) // s + 1


def _check_patch_divisible(strides, dims):
    tot = [1, 1, 1]
    for s in strides:
        tot = [a * b for a, b in zip(tot, _k3(s))]
    assert all(d % t == 0 for d, t in zip(dims, tot)), \
        f"patch {dims[0]}x{dims[1]}x{dims[2]} must be divisible by {tot[0]}x{tot[1]}x{tot[2]} (the product of the strides per axis)"


# ------------------------------------------------------------------------------------------------ sliding-window target
# What HipPlainConvUNet.fuse_window_accumulate / fuse_window_feature_accumulate hand the forward: window k of the batch goes into
# acc / nsum at origins[k], read under the mirror mask mirrors[k]; space: "logits" (the head runs here) or "features" (it does not)
WindowSink = collections.namedtuple("WindowSink", "acc nsum gauss origins mirrors space")


def window_segments(origins, w, max_cover=4):
    """Launches of the feature-space window accumulation for windows at origins[k] = (x, y, z), w long on the last axis: a
    window index k (that window on its own) or (x, y, a, b, [window indices]): positions a..b-1 of the last axis of a row,
    which every listed window (at most max_cover) covers."""
    # consecutive windows of a sliding-window row overlap along the last axis: one launch per SEGMENT of that axis adds
    # every covering window's contribution in registers (same order, same bits) and touches the accumulator once
    launches = []
    k = 0
    while k < len(origins):
        j = k + 1
        while (j < len(origins) and origins[j][:2] == origins[k][:2]
               and origins[j - 1][2] < origins[j][2] < origins[j - 1][2] + w):
            j += 1
        if j - k == 1:
            launches.append(k)
        else:
            sx, sy = origins[k][:2]
            zs = [origins[i][2] for i in range(k, j)]
            cuts = sorted(set(zs + [z + w for z in zs]))
            for a, b in zip(cuts[:-1], cuts[1:]):
                cover = [i for i in range(k, j) if origins[i][2] <= a and b <= origins[i][2] + w]
                for c0 in range(0, len(cover), max_cover):      # (more than max_cover on a voxel: steps below w / max_cover)
                    launches.append((sx, sy, a, b, cover[c0:c0 + max_cover]))
        k = j
    return launches


# ------------------------------------------------------------------------------------------------ what a pass carries
class _Rows:
    """Channels-last rows in a tensor: the tensor that owns the memory, the address of the first row, the row pitch."""
    __slots__ = ("t", "ptr", "ld")

    def __init__(self, t, ptr_, ld):
        self.t, self.ptr, self.ld = t, ptr_, ld


class _Workspaces:
    """Byte buffers of one half of a pass by name, grown on demand."""
    # separate identities because they are live at the same time: "ws" (kernel workspace on the main stream), "stats"
    # (InstanceNorm statistics riding on the conv epilogue: one reusable buffer, conv -> finalize are stream ordered),
    # "gstats" (InstanceNorm backward sums left by a data gradient), "ws_side" (weight gradients on the side stream)

    def __init__(self, dev):
        self.dev, self.bufs = dev, {}

    def get(self, nbytes, key="ws"):
        nb = int(nbytes)
        t = self.bufs.get(key)
        if t is None or t.numel() < nb:
            t = self.bufs[key] = _ws(nb, self.dev)
        return t


@contextlib.contextmanager
def _timed(probe, where, key, nbatch, stream=None, **info):
    """bench.py (unet.set_probe): if the probe watches `where`, events around the body on `stream` go to probe[key]."""
    if probe is None or probe["where"] != where:
        yield
        return
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(stream)
    yield
    ev1.record(stream)
    probe.setdefault(key, []).append((ev0, ev1, nbatch))
    probe.update(info)


class _Pass:
    """What the steps of one half (forward or backward) of a network pass share."""

    def __init__(self, net, dev, batch):
        self.lib, self.net, self.dev, self.B = _lib.load(), net, dev, batch
        self.adt, self.impl = net.act_dtype, net.conv_impl
        self.dt = dtype_code(self.adt)
        self.esz = 4 if self.dt == F32 else 2
        self.cp = 8 if self.dt == F32 else 16      # channel padding granule of packed weights / first-layer input
        self.st = stream_of(dev)
        self.ws = _Workspaces(dev)
        self.probe = state_of(net).probe

    def empty(self, *shape, dtype=None):
        return torch.empty(shape, dtype=self.adt if dtype is None else dtype, device=self.dev)


class _BackwardPass(_Pass):
    """+ where the parameter gradients go and the side stream of the weight gradients."""

    def __init__(self, net, dev, batch):
        super().__init__(net, dev, batch)
        self.grads = {}          # id(param) -> grad tensor
        self.inplace = bool(net.accumulate_grads_in_place)
        self.acc = 1 if self.inplace else 0      # kernels add to the gradient buffers (which then are the parameters' .grad)
        # The weight gradients of the conv blocks are leaves of the backward chain (IN-bwd(L) -> dgrad(L) -> IN-bwd(L-1) ...
        # only passes dy on): they run on a SIDE STREAM, so that the MFMA-bound weight-gradient kernels overlap the
        # HBM-bound InstanceNorm passes of the main chain instead of queueing between them (DGTTA_WGRAD_STREAM=0: one stream)
        self.main_stream = torch.cuda.current_stream(dev)
        self.side = state_of(net).stream("side_stream", dev) if _wgrad_on_side_stream() else None
        if self.side is not None:
            self.side.wait_stream(self.main_stream)

    def gbuf(self, p):
        if self.inplace:
            if p.grad is None:
                p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
            return p.grad
        g = self.grads.get(id(p))
        if g is None:
            g = self.grads[id(p)] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return g

    def scratch_like(self, p):
        """Throw-away gradient buffer (only the bias of this layer wants a gradient): it is written by the kernel on
        the side stream, so it comes from that stream's pool - a main-stream block could be handed out again while
        the side kernel still writes to it."""
        if self.side is None:
            return torch.empty_like(p)
        with torch.cuda.stream(self.side):
            return torch.empty_like(p)

    def hand_over(self, nbytes, *reads):
        """(workspace, stream handle) for a weight-gradient launch that reads `reads`, complete on the main stream now."""
        if self.side is None:
            return self.ws.get(nbytes), self.st
        ev = torch.cuda.Event()
        ev.record(self.main_stream)
        self.side.wait_event(ev)
        for t in reads:
            t.record_stream(self.side)      # the allocator must not hand the block out again before the side stream is done
        with torch.cuda.stream(self.side):
            w = self.ws.get(nbytes, "ws_side")
        return w, self.side.cuda_stream


# ------------------------------------------------------------------------------------------------ layer executors
class _ConvLayer:
    """One Conv3d + InstanceNorm + LeakyReLU block of a pass: static shape, the kernel family of the conv - 3x3x3 (`conv_impl`
    applies) or, for a (kd, 3, 3) kernel / per-axis stride, anisotropic (csrc/conv_aniso.hip) - and what the forward leaves
    for the backward (input rows x, raw conv output y, InstanceNorm mean / rstd mr, activation rows z)."""
    __slots__ = ("mod", "where", "aniso", "halfwise", "cin", "cout", "cinp", "coutp", "stride", "din", "dout", "vout",
                 "x", "xbs", "y", "mr", "z")

    def __init__(self, p, mod, where, cin, din):
        conv = mod.conv
        self.mod, self.where, self.aniso = mod, where, conv.aniso
        # the two halves of a concat buffer on their own (input planes, packed weight slices): not the anisotropic kernels
        self.halfwise = not conv.aniso
        self.cin, self.cout = cin, conv.out_channels
        self.cinp, self.coutp = _pad(cin, p.cp), _pad(self.cout, p.cp)
        self.stride = _k3(conv.stride)
        self.din, self.dout = tuple(din), tuple(_odim(i, s) for i, s in zip(din, self.stride))
        self.vout = self.dout[0] * self.dout[1] * self.dout[2]

    def weights(self, p, cin_slice=None):
        """Packed weight blob; cin_slice = (lo, hi): of the conv restricted to input channels lo..hi-1."""
        conv = self.mod.conv
        if self.aniso:
            assert cin_slice is None, "the anisotropic kernels have no packed weight slices"
            return p.net.kpacked(conv, p.dt, self.cinp, self.coutp)
        if cin_slice is None:
            return p.net.packed(conv, p.dt, self.cinp, self.coutp)
        return p.net.packed(conv, p.dt, _pad(cin_slice[1] - cin_slice[0], p.cp), self.coutp, cin_slice)

    def forward(self, p, x, xbs=0):
        """y = conv(x) + bias; returns the InstanceNorm statistics the epilogue left.  xbs: x is two planes, xbs elements apart."""
        conv, B, cin, cout = self.mod.conv, p.B, self.cin, self.cout
        self.x, self.xbs = x, xbs
        w = self.weights(p)
        self.y = p.empty(B, *self.dout, cout)
        stats = p.ws.get(p.lib.dgtta_conv3d_stats_bytes(B, cout, *self.dout), "stats")
        with _timed(p.probe, self.where, "events", B, cin=cin, cout=cout, vout=self.vout, batch=B):
            if self.aniso:
                check(p.lib.dgtta_conv3d_fwd(x.ptr, x.ld, ptr(w), ptr(conv.bias), ptr(self.y), cout, ptr(stats), B, cin, cout,
                                             self.cinp, self.coutp, *self.din, conv.kernel_size[0], *self.stride, p.dt, p.st),
                      "dgtta_conv3d_fwd")
            elif xbs:
                check(p.lib.dgtta_conv3d_k3_fwd_blocked(x.ptr, xbs, ptr(w), ptr(conv.bias), ptr(self.y), cout, ptr(stats), B, cin,
                                                        cout, self.cinp, self.coutp, *self.din, p.dt, p.st),
                      "dgtta_conv3d_k3_fwd_blocked")
            else:
                check(p.lib.dgtta_conv3d_k3_fwd(x.ptr, x.ld, ptr(w), ptr(conv.bias), ptr(self.y), cout, ptr(stats), B, cin, cout,
                                                self.cinp, self.coutp, *self.din, self.stride[0], p.dt, p.impl, p.st),
                      "dgtta_conv3d_k3_fwd")
        return stats

    def dgrad(self, p, dy, dst, ld, accumulate=0, cin_slice=None):
        """Data gradient written (accumulate=1: added) to rows of pitch ld at dst; cin_slice: of those input channels only."""
        cin = self.cin if cin_slice is None else cin_slice[1] - cin_slice[0]
        w = self.weights(p, cin_slice)
        if self.aniso:
            check(p.lib.dgtta_conv3d_dgrad(ptr(dy), self.cout, ptr(w), dst, ld, p.B, cin, self.cout, self.cinp, self.coutp,
                                           *self.din, self.mod.conv.kernel_size[0], *self.stride, accumulate, p.dt, p.st),
                  "dgtta_conv3d_dgrad")
        else:
            check(p.lib.dgtta_conv3d_k3_dgrad(ptr(dy), self.cout, ptr(w), dst, ld, p.B, cin, self.cout, _pad(cin, p.cp),
                                              self.coutp, *self.din, self.stride[0], accumulate, p.dt, p.impl, p.st),
                  "dgtta_conv3d_k3_dgrad")

    def dgrad_gstats(self, p, dy, gin, prev):
        """Data gradient into the dense tensor gin = the gradient of the activation of block `prev`, which this conv alone read;
        returns the sums of prev's InstanceNorm backward where the kernel left them (csrc/conv_rows.hip, GST), else None."""
        if self.aniso or self.stride[0] != 1 or p.dt == F32 or prev.cout != self.cin or prev.dout != self.din:
            return self.dgrad(p, dy, ptr(gin), self.cin)      # (no fused statistics for these)
        w, pn, cin = self.weights(p), prev.mod.norm, self.cin
        gbytes = p.lib.dgtta_conv3d_stats_bytes(p.B, cin, *self.din)
        gstats = p.ws.get(gbytes, "gstats")
        produced = C.c_int(0)
        check(p.lib.dgtta_conv3d_k3_dgrad_gstats(ptr(dy), self.cout, ptr(w), ptr(gin), cin, p.B, cin, self.cout, self.cinp,
                                                 self.coutp, *self.din, ptr(prev.y), cin, ptr(prev.mr), ptr(pn.weight),
                                                 ptr(pn.bias), SLOPE, ptr(gstats), gbytes, C.byref(produced), p.dt, p.impl, p.st),
              "dgtta_conv3d_k3_dgrad_gstats")
        return gstats if produced.value else None

    def wgrad_ws_bytes(self, p):
        B, cin, cout, s = p.B, self.cin, self.cout, self.stride[0]
        if self.aniso:
            return p.lib.dgtta_conv3d_kwgrad_ws_bytes(B, cin, cout, *self.din, self.mod.conv.kernel_size[0], *self.stride)
        # fp32 storage: offer the split workspace - the weight gradient then runs as six launches of the
        # 16-bit matrix-core kernels on exact three-term bf16 splits of x and dy (csrc/conv_wgrad.hip)
        if p.dt == F32 and p.impl != 1 and (s == 1 or not ((self.din[0] | self.din[1] | self.din[2]) & 1)):
            return p.lib.dgtta_conv3d_wgrad_split_ws_bytes(B, cin, cout, *self.dout, s)
        return p.lib.dgtta_conv3d_wgrad_ws_bytes(B, cin, cout, *self.dout)

    def wgrad(self, p, dy, dw, db, ws, nb, stream):
        """Weight (dw) and bias (db or None) gradient from the saved input and dy, on `stream` with its workspace ws."""
        x, cin, cout = self.x, self.cin, self.cout
        if self.aniso:
            check(p.lib.dgtta_conv3d_wgrad(x.ptr, x.ld, ptr(dy), cout, ptr(dw), ptr(db), ptr(ws), nb, p.B, cin, cout, *self.din,
                                           self.mod.conv.kernel_size[0], *self.stride, p.acc, p.dt, stream), "dgtta_conv3d_wgrad")
        elif self.xbs:
            check(p.lib.dgtta_conv3d_k3_wgrad_blocked(x.ptr, self.xbs, ptr(dy), cout, ptr(dw), ptr(db), ptr(ws), nb, p.B, cin,
                                                      cout, *self.din, p.acc, p.dt, stream), "dgtta_conv3d_k3_wgrad_blocked")
        else:
            check(p.lib.dgtta_conv3d_k3_wgrad(x.ptr, x.ld, ptr(dy), cout, ptr(dw), ptr(db), ptr(ws), nb, p.B, cin, cout,
                                              *self.din, self.stride[0], p.acc, p.dt, p.impl, stream), "dgtta_conv3d_k3_wgrad")


class _UpLayer:
    """One transposed conv (kernel = stride) of a pass: 2x2x2 (`conv_impl` applies) or anisotropic; keeps its input rows x."""
    __slots__ = ("mod", "aniso", "halfwise", "cin", "cout", "din", "x")

    def __init__(self, mod, cin, cout, din):
        self.mod, self.aniso, self.cin, self.cout, self.din = mod, mod.aniso, cin, cout, tuple(din)
        self.halfwise = not mod.aniso      # (reads the up half of a concat gradient kept as a plane)

    def fwd(self, p, x, out):
        """Writes up(x) to the rows `out` (the first channel half of a concat buffer)."""
        m = self.mod
        self.x = x
        if self.aniso:
            nb = p.lib.dgtta_convT3d_s_fwd_ws_bytes(self.cin, self.cout, *m.kernel_size, p.dt)
            ws = p.ws.get(nb)
            check(p.lib.dgtta_convT3d_s_fwd(x.ptr, x.ld, ptr(m.weight), ptr(m.bias), out.ptr, out.ld, ptr(ws), nb, p.B, self.cin,
                                            self.cout, *self.din, *m.kernel_size, p.dt, p.st), "dgtta_convT3d_s_fwd")
        else:
            nb = p.lib.dgtta_convT3d_fwd_ws_bytes(self.cin, self.cout, p.dt)
            ws = p.ws.get(nb)
            check(p.lib.dgtta_convT3d_k2s2_fwd(x.ptr, x.ld, ptr(m.weight), ptr(m.bias), out.ptr, out.ld, ptr(ws), nb, p.B,
                                               self.cin, self.cout, *self.din, p.dt, p.impl, p.st), "dgtta_convT3d_k2s2_fwd")

    def bwd_ws_bytes(self, p):
        if self.aniso:
            return p.lib.dgtta_convT3d_s_bwd_ws_bytes(p.B, self.cin, self.cout, *self.din, *self.mod.kernel_size)
        # fp32 storage: room for the weight gradient as six 16-bit launches on exact bf16 splits (as for the 3x3x3 convs)
        return (p.lib.dgtta_convT3d_bwd_split_ws_bytes if p.dt == F32 and p.impl != 1 else
                p.lib.dgtta_convT3d_bwd_ws_bytes)(p.B, self.cin, self.cout, *self.din)

    def bwd(self, p, g, dx, dw, db, ws, nb, stream):
        """From the output's gradient rows g: data gradient to dx and / or weight, bias gradient to dw, db (addresses or None)."""
        x, m = self.x, self.mod
        if self.aniso:
            check(p.lib.dgtta_convT3d_s_bwd(x.ptr, x.ld, g.ptr, g.ld, ptr(m.weight), dx, self.cin, dw, db, ptr(ws), nb, p.B,
                                            self.cin, self.cout, *self.din, *m.kernel_size, p.acc, p.dt, stream),
                  "dgtta_convT3d_s_bwd")
        else:
            check(p.lib.dgtta_convT3d_k2s2_bwd(x.ptr, x.ld, g.ptr, g.ld, ptr(m.weight), dx, self.cin, dw, db, ptr(ws), nb, p.B,
                                               self.cin, self.cout, *self.din, p.acc, p.dt, p.impl, stream),
                  "dgtta_convT3d_k2s2_bwd")


class _Cat:
    """Concat buffer [up | skip] of a decoder level, c channels per half: rows of 2 c channels, or two planes xbs apart."""
    __slots__ = ("buf", "c", "dims", "xbs")

    def __init__(self, p, c, dims, planar):
        self.c, self.dims = c, dims
        if planar:
            self.buf = p.empty(2, p.B, *dims, c)
            self.xbs = p.B * dims[0] * dims[1] * dims[2] * c
        else:
            self.buf = p.empty(p.B, *dims, 2 * c)
            self.xbs = 0

    def rows(self):
        """The whole buffer = where its up half starts (planes: the dense tensor at the buffer's start)."""
        return _Rows(self.buf, self.buf.data_ptr(), self.c if self.xbs else 2 * self.c)

    def skip_rows(self, p):
        if self.xbs:
            return _Rows(self.buf, self.buf[1].data_ptr(), self.c)
        return _Rows(self.buf, self.buf.data_ptr() + self.c * p.esz, 2 * self.c)


def _plan(p, cin, dims):
    """Layers of a pass on `cin` channels of size `dims`: (encoder blocks per stage, transposed convs, decoder blocks per stage)."""
    enc_mods, dec_mods = p.net.conv_blocks()
    enc, ups, dec = [], [], []
    for si, mods in enumerate(enc_mods):
        enc.append([])
        for bi, mod in enumerate(mods):
            blk = _ConvLayer(p, mod, ("enc", si, bi), cin, dims)
            enc[-1].append(blk)
            cin, dims = blk.cout, blk.dout
    for k, mods in enumerate(dec_mods):
        skip = enc[-(k + 2)][-1]
        ups.append(_UpLayer(p.net.decoder.transpconvs[k], cin, skip.cout, dims))
        cin, dims = 2 * skip.cout, skip.dout
        dec.append([])
        for bi, mod in enumerate(mods):
            blk = _ConvLayer(p, mod, ("dec", k, bi), cin, dims)
            dec[-1].append(blk)
            cin, dims = blk.cout, blk.dout
    return enc, ups, dec


# ------------------------------------------------------------------------------------------------ forward steps
def _input_rows(p, x):
    """The network input as NDHWC rows padded to the channel granule."""
    B, cin, D, H, W = x.shape
    cinp = _pad(cin, p.cp)
    if (x.dtype == p.adt and x.stride(1) == 1 and x.stride(4) == cinp and x.stride(3) == W * cinp
            and x.stride(2) == H * W * cinp and x.stride(0) == D * H * W * cinp):
        xin = x            # already voxel-major with rows of cinp (zero padded) channels, e.g. from mind_hook
    else:
        xin = p.empty(B, D, H, W, cinp)
        xs = x.contiguous().float()
        check(p.lib.dgtta_ncdhw_to_ndhwc(ptr(xs), ptr(xin), B, cin, D * H * W, cinp, p.dt, p.st), "dgtta_ncdhw_to_ndhwc")
    return _Rows(xin, xin.data_ptr(), cinp)


def _block_forward(p, blk, x, xbs=0, z=None, stats_only=False):
    """conv -> InstanceNorm -> LeakyReLU of `blk` on rows x; returns the activation's rows (z if given, else a fresh tensor).
    stats_only: the InstanceNorm statistics are finalised but not applied (nothing is written; blk carries y and mr)."""
    B, cout = p.B, blk.cout
    norm = blk.mod.norm
    stats = blk.forward(p, x, xbs)
    blk.mr = p.empty(B, cout, 2, dtype=torch.float32)
    if stats_only:
        z = _Rows(None, None, cout)
    elif z is None:
        zt = p.empty(B, *blk.dout, cout)
        z = _Rows(zt, zt.data_ptr(), cout)
    blk.z = z
    nb = p.lib.dgtta_instnorm_ws_bytes(B, cout, blk.vout)
    ws = p.ws.get(nb)
    check(p.lib.dgtta_instnorm_lrelu_fwd(ptr(blk.y), cout, ptr(stats), ptr(norm.weight), ptr(norm.bias), ptr(blk.mr), z.ptr, z.ld,
                                         ptr(ws), nb, B, cout, blk.vout, EPS, SLOPE, p.dt, p.st), "dgtta_instnorm_lrelu_fwd")
    return z


# Where a HALF of the concat buffer is 64 bytes per voxel (32 channels of 16-bit values: level 0), the two halves are kept
# as dense PLANES [up | skip] instead of interleaved rows of 2 C channels: the kernels that read one half (the stride-2 conv
# of the skip below, its weight gradient, the transposed conv's backward) then use whole 128-byte lines (the memory side
# moves whole lines: 4.3x the input fetched before, profiles/r05_ab.txt).  The decoder conv that reads BOTH halves takes them
# as 32-channel blocks (dgtta_conv3d_k3_fwd_blocked) - where the ring kernels run (asked up front) and every layer that
# reads this buffer (`readers`: the next stage's first conv, the decoder's first conv of this level, the transposed conv)
# can (the anisotropic kernels take the interleaved layout); DGTTA_PLANAR_CAT=0: the interleaved layout everywhere.
def _planar_cat(p, skip, readers):
    """Is the concat buffer of the level whose skip the block `skip` writes kept as two planes?"""
    c = skip.cout
    return (c * p.esz == 64 and p.impl != 1 and os.environ.get("DGTTA_PLANAR_CAT", "1") != "0"
            and all(r.halfwise for r in readers)
            and os.environ.get("DGTTA_SPLIT_CAT_GRAD", "1") != "0"
            and p.lib.dgtta_conv3d_k3_blocked_supported(p.B, 2 * c, c, *skip.dout, p.dt) == 1)


def _encoder_forward(p, enc, ups, dec, x):
    """Encoder on rows x (a stage's last block writes the skip half of its level's concat buffer): (deepest rows, buffers)."""
    cats = []
    for si, stage in enumerate(enc):
        for blk in stage:
            z = None
            if blk is stage[-1] and si < len(enc) - 1:
                dk = len(enc) - 2 - si
                cats.append(_Cat(p, blk.cout, blk.dout, _planar_cat(p, blk, (enc[si + 1][0], dec[dk][0], ups[dk]))))
                z = cats[-1].skip_rows(p)
            x = _block_forward(p, blk, x, z=z)
    return x, cats


def _decoder_forward(p, ups, dec, cats, x, feat_fold):
    """Runs the decoder from the deepest activation x; returns every stage's output rows (the last: what the segmentation
    head reads, the others: what the auxiliary heads of deep supervision read)."""
    stage_rows = []
    for up, stage, cat in zip(ups, dec, reversed(cats)):
        up.fwd(p, x, cat.rows())
        x = cat.rows()
        for blk in stage:
            # feature-space window accumulation: the block in front of the head hands over its raw conv output and statistics -
            # its InstanceNorm + LeakyReLU apply runs inside the accumulation kernel, z is never written
            fold = feat_fold and blk is dec[-1][-1]
            x = _block_forward(p, blk, x, xbs=cat.xbs if blk is stage[0] else 0, stats_only=fold)
        stage_rows.append(x)
    return stage_rows


def _accumulate_feature_windows(p, sink, last, z, feat_fold, dims):
    """Adds gauss * (the 32 channels the head reads) of window k into the accumulator at origins[k] (csrc/window_features.hip)."""
    lib, dt, st = p.lib, p.dt, p.st
    acc, nsum, gauss, origins, mirrors = sink.acc, sink.nsum, sink.gauss, sink.origins, sink.mirrors
    X, Y, Z = acc.shape[:3]
    D, H, W = dims
    nrm = last.mod.norm
    src0 = last.y.data_ptr() if feat_fold else z.ptr
    assert (32 if feat_fold else z.ld) == 32
    wbytes = D * H * W * 32 * p.esz            # one window of the source
    mrbytes = 32 * 2 * 4                       # one window of mean / rstd
    fold = (ptr(nrm.weight), ptr(nrm.bias), SLOPE)

    def one(k):      # one window per launch, un-flipped by the kernel (mask 0: the unmirrored kernel)
        place = (ptr(gauss), ptr(acc), ptr(nsum), 32, D, H, W, X, Y, Z, *origins[k], dt, mirrors[k], st)
        if feat_fold:
            check(lib.dgtta_feature_window_accumulate_norm_mirror(src0 + k * wbytes, last.mr.data_ptr() + k * mrbytes, *fold, *place),
                  "dgtta_feature_window_accumulate_norm_mirror")
        else:
            check(lib.dgtta_feature_window_accumulate_mirror(src0 + k * wbytes, *place), "dgtta_feature_window_accumulate_mirror")

    for k in (k for k in range(len(origins)) if mirrors[k]):
        one(k)
    plain = [k for k in range(len(origins)) if not mirrors[k]]      # the unmirrored windows keep the segment merging
    segments = os.environ.get("DGTTA_FEATURE_SEGMENTS", "1") != "0"
    for launch in window_segments([origins[k] for k in plain], W) if segments else range(len(plain)):
        if isinstance(launch, int):
            one(plain[launch])
            continue
        sx, sy, a, b, part = launch
        part = [plain[i] for i in part]
        n = len(part)
        srcs = (C.c_void_p * n)(*[src0 + i * wbytes for i in part])
        mrs = (C.c_void_p * n)(*[last.mr.data_ptr() + i * mrbytes for i in part]) if feat_fold else None
        zoffs = (C.c_int * n)(*[a - origins[i][2] for i in part])
        check(lib.dgtta_feature_window_accumulate_multi(srcs, mrs, zoffs, n, *fold, ptr(gauss), ptr(acc), ptr(nsum), 32, D, H, W, b - a,
                                                        X, Y, Z, sx, sy, a, dt, st), "dgtta_feature_window_accumulate_multi")


def _accumulate_logit_windows(p, sink, head, z, dims):
    """Head fused with the Gaussian window accumulation: overlapping windows are accumulated one after the other, a mirrored pass
    un-flipped on its way into the accumulator (mask 0: the unmirrored kernel)."""
    acc, nsum = sink.acc, sink.nsum
    D, H, W = dims
    for k, origin in enumerate(sink.origins):
        args = (z.ptr + k * D * H * W * z.ld * p.esz, ptr(head.weight), ptr(head.bias), ptr(sink.gauss), ptr(acc), ptr(nsum),
                head.in_channels, head.out_channels, D, H, W, *acc.shape[:3], *origin, p.dt)
        if acc.dtype == torch.float32:
            check(p.lib.dgtta_seghead_window_accumulate_mirror_t(*args, F32, sink.mirrors[k], p.st), "dgtta_seghead_window_accumulate_mirror_t")
        else:      # the _mirror entry takes fp32 accumulators only; a fp16 one is never mirrored into (fuse_window_accumulate)
            check(p.lib.dgtta_seghead_window_accumulate_t(*args, F16, p.st), "dgtta_seghead_window_accumulate_t")


def _head_forward(p, head, z, sel, nsel, fw, dims):
    """Head (the selected rows) on rows z, fused with the inverse warp of its logits if fw = (theta device, theta host)."""
    D, H, W = dims
    out = p.empty(p.B, D, H, W, nsel, dtype=torch.float32)
    if fw is not None:
        assert z.ld == head.in_channels and tuple(fw[0].shape) == (p.B, 3, 4), "fuse_output_warp: shape mismatch"
        check(p.lib.dgtta_seghead_warp_fwd(z.ptr, ptr(head.weight), ptr(head.bias), ptr(sel), nsel, ptr(fw[0]), ptr(out), p.B,
                                           head.in_channels, D, H, W, 1, p.dt, p.st), "dgtta_seghead_warp_fwd")
    else:
        check(p.lib.dgtta_seghead_fwd(z.ptr, z.ld, ptr(head.weight), ptr(head.bias), ptr(sel), nsel, ptr(out), 1, nsel, p.B,
                                      head.in_channels, D * H * W, p.dt, p.st), "dgtta_seghead_fwd")
    return out


def _aux_heads_forward(p, net, dec, stage_rows, sel, nsel):
    """Deep supervision: seg_layers[k] (the selected rows) on the output rows of decoder stage k, for every stage but the last;
    returned highest resolution first (the order of nnU-Net's decoder, after the full-resolution output)."""
    return [_head_forward(p, net.decoder.seg_layers[k], stage_rows[k], sel, nsel, None, dec[k][-1].dout)
            for k in range(len(dec) - 2, -1, -1)]


# ------------------------------------------------------------------------------------------------ backward steps
def _scatter_head_grads(p, head, sel, dws, dbs):
    """Adds the compact weight / bias gradient rows of a head (its selected rows) into the parameters' gradient buffers."""
    cin = head.in_channels
    gw, gb = p.gbuf(head.weight), p.gbuf(head.bias)
    if sel is None:
        gw.view(-1, cin).add_(dws)       # buffers start at zero (or hold earlier accumulation steps)
        gb.add_(dbs)
    else:
        gw.view(-1, cin).index_add_(0, sel.long(), dws)
        gb.index_add_(0, sel.long(), dbs)


def _aux_head_backward(p, head, z, sel, nsel, gout, gz, dims):
    """Backward of an auxiliary head from gout, the gradient of its logits: ADDS its data gradient to the rows gz (which the
    transposed conv's backward has just written) and its weight / bias gradient to the parameters' buffers."""
    D, H, W = dims
    cin = head.in_channels
    assert gz.ld >= cin and z.ld >= cin
    g = gout.contiguous(memory_format=torch.channels_last_3d).float()      # [B,nsel,D,H,W] stored NDHWC
    need_hw = head.weight.requires_grad or head.bias.requires_grad
    dws = p.empty(nsel, cin, dtype=torch.float32) if need_hw else None
    dbs = p.empty(nsel, dtype=torch.float32) if need_hw else None
    nb = p.lib.dgtta_seghead_bwd_ws_bytes(p.B, cin, nsel, D * H * W)
    ws = p.ws.get(nb)
    check(p.lib.dgtta_seghead_bwd_acc(z.ptr, z.ld, ptr(g), nsel, ptr(head.weight), ptr(sel), nsel, gz.ptr, gz.ld, ptr(dws), ptr(dbs),
                                      ptr(ws), nb, p.B, cin, D * H * W, 0, 1, p.dt, p.st), "dgtta_seghead_bwd_acc")
    if need_hw:
        _scatter_head_grads(p, head, sel, dws, dbs)


# The gradient rows of the head's input as their two factors (DGTTA_HEAD_GZ_FOLD): d16, the gathered logit gradient (rows of
# nsel values in the storage type), and the head whose selected weight rows multiply it.  gz = W^T d16 is never stored: the
# InstanceNorm backward of the block in front of the head rebuilds it in both of its passes (dgtta_instnorm_lrelu_bwd_head).
_HeadGrad = collections.namedtuple("_HeadGrad", "d16 head sel nsel")


def _head_backward(p, head, z, sel, nsel, fw, g16, gout, dims):
    """Backward of `_head_forward` from gout (or g16, what the loss left in the Grad16Sink): the gradient rows of z - or, on
    the fused head + warp path with 16 classes of a 16-bit network, a _HeadGrad in their place."""
    lib, B, dt, st = p.lib, p.B, p.dt, p.st
    D, H, W = dims
    if g16 is not None and any(gout.stride()):
        # the placeholder has stride 0 everywhere; a dense gout means another consumer of the output contributed: sum in fp32
        gout = gout + g16.permute(0, 4, 1, 2, 3).float()
        g16 = None
    g = None if g16 is not None else gout.contiguous(memory_format=torch.channels_last_3d).float()      # [B,nsel,D,H,W] stored NDHWC
    cin = head.in_channels
    need_hw = head.weight.requires_grad or head.bias.requires_grad
    dws = p.empty(nsel, cin, dtype=torch.float32) if need_hw else None
    dbs = p.empty(nsel, dtype=torch.float32) if need_hw else None
    if (fw is not None and g16 is not None and nsel == 16 and cin == 32 and z.ld == 32 and p.esz == 2 and p.impl != 1
            and os.environ.get("DGTTA_HEAD_GZ_FOLD", "1") != "0"):
        nb = lib.dgtta_seghead_warp_bwd_ws_bytes(B, cin, nsel, D, H, W)
        ws = p.ws.get(nb)
        assert tuple(g16.shape) == (B, D, H, W, nsel) and g16.dtype == p.adt and g16.is_contiguous()
        d16 = p.empty(B, D, H, W, nsel)
        check(lib.dgtta_seghead_warp_bwd_g16_d16(z.ptr, ptr(g16), ptr(fw[0]), ptr(fw[1]), nsel, ptr(d16), ptr(dws), ptr(dbs), ptr(ws),
                                                 nb, B, cin, D, H, W, 1, 0, dt, st), "dgtta_seghead_warp_bwd_g16_d16")
        if need_hw:
            _scatter_head_grads(p, head, sel, dws, dbs)
        return _HeadGrad(d16, head, sel, nsel)
    gz = p.empty(B, D, H, W, cin)
    if fw is not None:      # g is the gradient of the WARPED logits: fused gather + W^T (+ weight / bias gradient)
        nb = lib.dgtta_seghead_warp_bwd_ws_bytes(B, cin, nsel, D, H, W)
        ws = p.ws.get(nb)
        assert g16 is None or (tuple(g16.shape) == (B, D, H, W, nsel) and g16.dtype == p.adt and g16.is_contiguous())
        bwd = lib.dgtta_seghead_warp_bwd if g16 is None else lib.dgtta_seghead_warp_bwd_g16
        check(bwd(z.ptr, ptr(g if g16 is None else g16), ptr(fw[0]), ptr(fw[1]), ptr(head.weight), ptr(sel), nsel, ptr(gz),
                  ptr(dws), ptr(dbs), ptr(ws), nb, B, cin, D, H, W, 1, 0, dt, st), bwd.__name__)
    else:
        nb = lib.dgtta_seghead_bwd_ws_bytes(B, cin, nsel, D * H * W)
        ws = p.ws.get(nb)
        check(lib.dgtta_seghead_bwd(z.ptr, z.ld, ptr(g), nsel, ptr(head.weight), ptr(sel), nsel, ptr(gz), cin, ptr(dws), ptr(dbs),
                                    ptr(ws), nb, B, cin, D * H * W, 0, dt, st), "dgtta_seghead_bwd")
    if need_hw:
        _scatter_head_grads(p, head, sel, dws, dbs)
    return _Rows(gz, gz.data_ptr(), cin)


def _norm_backward(p, blk, gz, gstats):
    """InstanceNorm + LeakyReLU backward of `blk` from gradient rows gz: dy (dense, fresh).  gstats: the reduction's sums,
    where the data gradient that produced gz left them.  gz may be a _HeadGrad (the block in front of the head)."""
    lib, B, cout, v = p.lib, p.B, blk.cout, blk.vout
    norm = blk.mod.norm
    dy = p.empty(B, *blk.dout, cout)
    nb = lib.dgtta_instnorm_ws_bytes(B, cout, v)
    ws = p.ws.get(nb)
    dgam = p.gbuf(norm.weight) if norm.weight.requires_grad else torch.empty_like(norm.weight)
    dbet = p.gbuf(norm.bias) if norm.bias.requires_grad else torch.empty_like(norm.bias)
    if isinstance(gz, _HeadGrad):
        assert cout == 32 and gstats is None
        check(lib.dgtta_instnorm_lrelu_bwd_head(ptr(gz.d16), ptr(gz.head.weight), ptr(gz.sel), gz.nsel, ptr(blk.y), cout,
                                                ptr(norm.weight), ptr(norm.bias), ptr(blk.mr), ptr(dy), cout, ptr(dgam), ptr(dbet),
                                                ptr(ws), nb, B, cout, v, SLOPE, p.acc, p.dt, p.st), "dgtta_instnorm_lrelu_bwd_head")
    elif gstats is not None:
        check(lib.dgtta_instnorm_lrelu_bwd_gstats(gz.ptr, gz.ld, ptr(blk.y), cout, ptr(norm.weight), ptr(norm.bias), ptr(blk.mr),
                                                  ptr(dy), cout, ptr(dgam), ptr(dbet), ptr(gstats), ptr(ws), nb, B, cout, v,
                                                  SLOPE, p.acc, p.dt, p.st), "dgtta_instnorm_lrelu_bwd_gstats")
    else:
        check(lib.dgtta_instnorm_lrelu_bwd(gz.ptr, gz.ld, ptr(blk.y), cout, ptr(norm.weight), ptr(norm.bias), ptr(blk.mr), ptr(dy),
                                           cout, ptr(dgam), ptr(dbet), ptr(ws), nb, B, cout, v, SLOPE, p.acc, p.dt, p.st),
              "dgtta_instnorm_lrelu_bwd")
    return dy


def _weight_grad(p, blk, dy):
    """Weight / bias gradient of the conv of `blk` (a leaf of the backward chain: on the side stream where there is one)."""
    conv = blk.mod.conv
    if not (conv.weight.requires_grad or conv.bias.requires_grad):
        return
    nb = blk.wgrad_ws_bytes(p)
    dw = p.gbuf(conv.weight) if conv.weight.requires_grad else p.scratch_like(conv.weight)
    db = p.gbuf(conv.bias) if conv.bias.requires_grad else None
    if p.net.exact_zero_bias_grad:
        db = None       # gradient buffer stays exactly zero (see HipPlainConvUNet.exact_zero_bias_grad)
    ws, stream = p.hand_over(nb, dy)      # dy (and the gradient buffers) are complete on the main stream
    with _timed(p.probe, blk.where, "wgrad_events", p.B, p.main_stream if p.side is None else p.side):
        blk.wgrad(p, dy, dw, db, ws, nb, stream)


def _concat_grad(p, blk, dy, cat):
    """Data gradient of `blk`, whose input was the concat buffer `cat`: gradient rows of (up half, skip half), fully written."""
    B, c = p.B, cat.c
    if c * p.esz == 64 and blk.halfwise and (cat.xbs or os.environ.get("DGTTA_SPLIT_CAT_GRAD", "1") != "0"):
        # 32 channels of 16-bit values = HALF a 128-byte line: as one [voxel][2 C] tensor every consumer of ONE half of this
        # gradient (the transposed conv's backward, the stride-2 data gradient's accumulate, the InstanceNorm backward
        # of the skip block) would fetch whole lines and use 64 bytes of each (profiles/r05_ab.txt, fetch_calib.sh).
        # The data gradient's two 32-channel output blocks are independent jobs of the kernel anyway: two launches on
        # the weight halves write two DENSE tensors (same values, the same reads of dy).
        halves = [p.empty(B, *cat.dims, c), p.empty(B, *cat.dims, c)]
        for i, dst in enumerate(halves):
            blk.dgrad(p, dy, ptr(dst), c, cin_slice=(i * c, (i + 1) * c))
        return tuple(_Rows(t, t.data_ptr(), c) for t in halves)
    gc = torch.empty_like(cat.buf)
    blk.dgrad(p, dy, ptr(gc), 2 * c)
    return _Rows(gc, gc.data_ptr(), 2 * c), _Rows(gc, gc.data_ptr() + c * p.esz, 2 * c)


def _up_backward(p, up, g):
    """Transposed-conv backward from the gradient rows g of its output: the gradient rows of its input."""
    m = up.mod
    glow = p.empty(p.B, *up.din, up.cin)
    nb = up.bwd_ws_bytes(p)
    ws = p.ws.get(nb)
    need_w = m.weight.requires_grad or m.bias.requires_grad
    dw = (p.gbuf(m.weight) if m.weight.requires_grad else p.scratch_like(m.weight)) if need_w else None
    db = p.gbuf(m.bias) if m.bias.requires_grad else None
    if p.side is None or not need_w:
        up.bwd(p, g, ptr(glow), ptr(dw), ptr(db), ws, nb, p.st)
    else:
        # data gradient on the main chain, weight / bias gradient (a leaf) on the side stream
        ws_side, stream = p.hand_over(nb, g.t)      # g is complete on the main stream
        up.bwd(p, g, ptr(glow), None, None, ws, nb, p.st)
        up.bwd(p, g, None, ptr(dw), ptr(db), ws_side, nb, stream)
    return _Rows(glow, glow.data_ptr(), up.cin)


def _plain_grad(p, blk, dy, prev):
    """Data gradient of `blk` towards the activation of `prev`: (its rows, prev's InstanceNorm backward sums or None)."""
    gin = p.empty(p.B, *blk.din, blk.cin)
    gstats = blk.dgrad_gstats(p, dy, gin, prev)
    return _Rows(gin, gin.data_ptr(), blk.cin), gstats


class _UNetFn(torch.autograd.Function):
    """Whole-network autograd node: forward saves raw conv outputs, normalised activations and IN statistics."""

    @staticmethod
    def forward(ctx, net, x, sel, need_grad, sink, deep_supervision, *params):
        _lib.require_cuda(x)
        B, cin0, D, H, W = x.shape
        dims = (D, H, W)
        p = _Pass(net, x.device, B)
        cfg = net.cfg
        assert cin0 == cfg["in_channels"], f"expected {cfg['in_channels']} input channels, got {cin0}"
        _check_patch_divisible(cfg["strides"], dims)
        head = net.decoder.seg_layers[-1]
        sink_w = net._window_acc      # a WindowSink or None
        feat_fold = (sink_w is not None and sink_w.space == "features" and not need_grad and os.environ.get("DGTTA_FEATURE_FOLD", "1") != "0" and
                     head.in_channels == cfg["features"][0] == 32)
        enc, ups, dec = _plan(p, cin0, dims)
        z, cats = _encoder_forward(p, enc, ups, dec, _input_rows(p, x))
        stage_rows = _decoder_forward(p, ups, dec, cats, z, feat_fold)
        z = stage_rows[-1]
        if sink_w is not None:
            assert not need_grad and sel is None and z.ld == head.in_channels and len(sink_w.origins) == B, "fuse_window_accumulate: misuse"
            if sink_w.space == "features":      # feature space: no head here
                _accumulate_feature_windows(p, sink_w, dec[-1][-1], z, feat_fold, dims)
            else:
                _accumulate_logit_windows(p, sink_w, head, z, dims)
            return p.empty(B, 0, D, H, W, dtype=torch.float32)
        nsel = head.out_channels if sel is None else int(sel.numel())
        fw = net._fused_warp
        out = _head_forward(p, head, z, sel, nsel, fw, dims)
        aux = _aux_heads_forward(p, net, dec, stage_rows, sel, nsel) if deep_supervision else []
        if need_grad:
            ctx.set_materialize_grads(False)      # an output the loss does not use contributes nothing and launches nothing
            ctx.aux = [(stage_rows[k], dec[k][-1].dout) for k in range(len(dec) - 1)] if deep_supervision else None
            ctx.net, ctx.sel, ctx.params = net, sel, params
            ctx.blocks = [blk for stage in enc + dec for blk in stage]
            ctx.ups, ctx.cats = ups, cats
            ctx.meta = (B, dims, nsel, z)
            ctx.fused_warp = fw
            ctx.sink = sink if fw is not None else None
        if deep_supervision:
            return (out.permute(0, 4, 1, 2, 3),) + tuple(a.permute(0, 4, 1, 2, 3) for a in aux)
        return out.permute(0, 4, 1, 2, 3)

    @staticmethod
    def backward(ctx, gout, *gaux):
        net, blocks, ups, cats = ctx.net, ctx.blocks, ctx.ups, ctx.cats
        B, dims, nsel, z = ctx.meta
        if gout is None:      # the loss used auxiliary outputs only
            dev = next(g for g in gaux if g is not None).device
            gout = torch.zeros((B, nsel) + tuple(dims), dtype=torch.float32, device=dev)
        p = _BackwardPass(net, gout.device, B)
        g16 = ctx.sink.take() if ctx.sink is not None else None      # the loss left its gradient in the storage type
        gz = _head_backward(p, net.decoder.seg_layers[-1], z, ctx.sel, nsel, ctx.fused_warp, g16, gout, dims)
        gskip = {}          # decoder stage -> gradient rows of the skip half of its concat buffer
        gstats = None       # InstanceNorm backward sums left by the data gradient that produced the current gz
        for idx in range(len(blocks) - 1, -1, -1):
            blk = blocks[idx]
            dy = _norm_backward(p, blk, gz, gstats)
            _weight_grad(p, blk, dy)
            if idx == 0:
                break
            kind, sidx, bidx = blk.where
            gstats = None
            if kind == "dec" and bidx == 0:
                gup, gskip[sidx] = _concat_grad(p, blk, dy, cats[-(sidx + 1)])
                gz = _up_backward(p, ups[sidx], gup)
                # gz = the gradient rows of decoder stage sidx - 1's output: its auxiliary head (output n - sidx of n) adds to them
                if sidx > 0 and gaux and gaux[len(ups) - 1 - sidx] is not None:
                    za, adims = ctx.aux[sidx - 1]
                    _aux_head_backward(p, net.decoder.seg_layers[sidx - 1], za, ctx.sel, nsel, gaux[len(ups) - 1 - sidx], gz, adims)
            elif kind == "enc" and bidx == 0:
                # input was the previous encoder stage's output, which lives in the skip half of a concat buffer
                # and already holds the decoder's skip gradient: accumulate into it.
                gz = gskip[len(ups) - sidx]
                blk.dgrad(p, dy, gz.ptr, gz.ld, accumulate=1)
            else:
                gz, gstats = _plain_grad(p, blk, dy, blocks[idx - 1])
        if p.side is not None:
            p.main_stream.wait_stream(p.side)         # gradients complete before anything downstream (optimizer, next pass)
        return (None,) * 6 + tuple(p.grads.get(id(q)) if q.requires_grad else None for q in ctx.params)
