"""nnUNet 3d_fullres PlainConvUNet executed by the HIP kernels (forward AND backward), as one autograd node.

Drop-in for the network object the reference obtains from nnUNetPredictor (dg_tta/tta/nnunet_utils.py:88-113; class
`dynamic_network_architectures.architectures.unet.PlainConvUNet`, built at
dg_tta/pretraining/nnUNetTrainer_GIN_MIND.py:46-53): same state-dict keys (incl. the duplicated `all_modules.*` and
`decoder.encoder.*` entries), `.encoder` attribute (tta.py:210), norm modules whose class name contains
"instancenorm" (torch_utils.py:130-137), forward (pre-)hooks honoured (model_utils.py:22-33).

This file is the module tree and the public API; unet_exec.py runs it (layer executors, the autograd node).
"""
import contextlib
import copy
import os

import torch
from torch import nn

from . import _lib
from ._lib import check, ptr, stream_of
from ._state import state_of
from .ops import F32, BF16, F16, dtype_code
from .unet_exec import EPS, SLOPE, WindowSink, _UNetFn, _k3

PLANS_3D_FULLRES = dict(features=(32, 64, 128, 256, 320), strides=(1, 2, 2, 2, 2),
                        n_conv_enc=(2, 2, 2, 2, 2), n_conv_dec=(2, 2, 2, 2),
                        in_channels=12, num_classes=105)


# ------------------------------------------------------------------------------------------------ parameter holders
class HipConv3d(nn.Module):
    """Parameter holder for a 3x3x3 / 1x1x1 conv (weights in PyTorch layout so checkpoints load unchanged).  An anisotropic
    layer (kernel (kd, 3, 3) or a per-axis stride, from anisotropic plans) keeps tuples in kernel_size / stride and aniso=True;
    an isotropic one keeps today's ints."""

    def __init__(self, cin, cout, k, stride):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size, self.stride = cin, cout, k, stride
        self.aniso = isinstance(k, tuple) or isinstance(stride, tuple)
        self.weight = nn.Parameter(torch.empty(cout, cin, *_k3(k)))
        self.bias = nn.Parameter(torch.empty(cout))


class HipConvTranspose3d(nn.Module):
    def __init__(self, cin, cout, k):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = cin, cout, k
        self.aniso = isinstance(k, tuple)       # kernel = stride (kd, kh, kw) other than (2, 2, 2)
        self.weight = nn.Parameter(torch.empty(cin, cout, *_k3(k)))
        self.bias = nn.Parameter(torch.empty(cout))


def layer_geometry(kernel, stride):
    """(kernel, stride) as a conv layer holds them: ints for a 3x3x3 kernel with an isotropic stride (the k3 kernels), tuples
    otherwise (the anisotropic kernels)."""
    k, s = _k3(kernel), _k3(stride)
    if k == (3, 3, 3) and len(set(s)) == 1:
        return 3, s[0]
    return k, s


class HipInstanceNorm3d(nn.Module):
    """name contains 'instancenorm' so that release_norms (torch_utils.py:130-137) finds it."""

    def __init__(self, c):
        super().__init__()
        self.num_features, self.eps = c, EPS
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))


class HipLeakyReLU(nn.Module):
    negative_slope = SLOPE


class ConvNormAct(nn.Module):
    def __init__(self, cin, cout, stride, kernel=3):
        super().__init__()
        self.conv = HipConv3d(cin, cout, *layer_geometry(kernel, stride))
        self.norm = HipInstanceNorm3d(cout)
        self.nonlin = HipLeakyReLU()
        self.all_modules = nn.Sequential(self.conv, self.norm, self.nonlin)


class StackedConvs(nn.Module):
    def __init__(self, n, cin, cout, first_stride, kernel=3):
        super().__init__()
        self.convs = nn.Sequential(*[ConvNormAct(cin if i == 0 else cout, cout, first_stride if i == 0 else 1, kernel)
                                     for i in range(n)])


class Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        stages, cin = [], cfg["in_channels"]
        kernels = cfg.get("kernel_sizes") or (3,) * len(cfg["features"])
        for f, s, n, k in zip(cfg["features"], cfg["strides"], cfg["n_conv_enc"], kernels):
            stages.append(nn.Sequential(StackedConvs(n, cin, f, s, k)))
            cin = f
        self.stages = nn.Sequential(*stages)


class Decoder(nn.Module):
    def __init__(self, encoder, cfg):
        super().__init__()
        self.encoder = encoder
        f, st = cfg["features"], cfg["strides"]
        kernels = cfg.get("kernel_sizes") or (3,) * len(f)
        stages, ups, segs = [], [], []
        for s in range(1, len(f)):
            below, skip = f[-s], f[-(s + 1)]
            up = _k3(st[-s])
            assert all(a in (1, 2) for a in up) and up != (1, 1, 1), f"transposed conv of stride {st[-s]} is not built"
            # kernel = stride (nnU-Net's rule); the decoder convs use the kernel of the skip's encoder stage
            ups.append(HipConvTranspose3d(below, skip, 2 if up == (2, 2, 2) else up))
            stages.append(StackedConvs(cfg["n_conv_dec"][s - 1], 2 * skip, skip, 1, kernels[-(s + 1)]))
            segs.append(HipConv3d(skip, cfg["num_classes"], 1, 1))
        self.stages = nn.ModuleList(stages)
        self.transpconvs = nn.ModuleList(ups)
        self.seg_layers = nn.ModuleList(segs)


# ------------------------------------------------------------------------------------------------ the network
class HipPlainConvUNet(nn.Module):
    """PlainConvUNet whose forward/backward run on hand-written gfx950 kernels.

    act_dtype: torch.float32 (parity mode), torch.bfloat16 or torch.float16 (16-bit storage + MFMA, fp32 accumulation;
    fp16 carries 3 more mantissa bits than bf16 and needs `loss_scale` for its gradients: BASELINE config 5).
    conv_impl: 0 auto (MFMA where covered, else general VALU kernel), 1 force VALU, 2 force MFMA.  It applies to the 3x3x3
    layers with isotropic strides; the anisotropic layers of anisotropic plans (cfg "kernel_sizes" (kd, 3, 3) / per-axis
    "strides") always run their matrix-core kernels (dgtta_conv3d_fwd / _dgrad / _wgrad, dgtta_convT3d_s_*).
    deep_supervision (a plain attribute, as nnU-Net's decoder.deep_supervision: toggle it at will): forward returns a tuple of
    logits, highest resolution first - element 0 is the usual output, element i is seg_layers[-1-i] on the output of decoder
    stage n-1-i - and the backward takes a gradient for each (ops.deep_supervision_loss).  It does not combine with
    fuse_output_warp / fuse_window_accumulate / fuse_window_feature_accumulate (ValueError).
    """

    def __init__(self, cfg=None, act_dtype=torch.float32, conv_impl=0, deep_supervision=False):
        super().__init__()
        cfg = dict(PLANS_3D_FULLRES if cfg is None else cfg)
        self.cfg = cfg
        self.encoder = Encoder(cfg)
        self.decoder = Decoder(self.encoder, cfg)
        self.act_dtype = act_dtype
        self.conv_impl = conv_impl
        # A conv bias in front of InstanceNorm has an identically zero gradient in exact arithmetic (the norm removes
        # the channel mean); autograd in the reference accumulates rounding noise there.  True: report exact zeros and
        # skip the reduction pass; False: compute sum(dy) like autograd does (parity experiments).
        self.exact_zero_bias_grad = False
        # True: backward adds straight into each parameter's .grad (allocated on first use) and returns no gradient
        # tensors to autograd - saves a zero-fill + add per parameter and backward pass.  Tensor hooks on parameters
        # are then not invoked; torch.autograd.grad() w.r.t. parameters is not supported in this mode.
        self.accumulate_grads_in_place = False
        # static loss scale of the fp16 storage path: the TTA loop multiplies the loss gradient by it (tta.tta_epoch) and
        # HipAdamW divides it out; 1 for fp32 / bf16 (their exponent range needs none)
        self.loss_scale = 16384.0 if act_dtype == torch.float16 else 1.0
        self._packed = {}        # id(weight) -> (version, wf, wb)
        self.selected_classes = None   # optional LongTensor: evaluate only these head rows (== map_label 'logits')
        self._fused_warp = None        # (theta on the device, theta on the host) while fuse_output_warp() is active
        self._window_acc = None        # sliding-window target (a WindowSink) while a fuse_window_*() context is active
        self.deep_supervision = bool(deep_supervision)

    def __deepcopy__(self, memo):
        # get_model_from_network deep-copies the network per ensemble member: do not drag the packed-weight cache along
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k == "_packed" else copy.deepcopy(v, memo)
        return new

    # -- structure helpers
    def conv_blocks(self):
        enc = [[c for c in st[0].convs] for st in self.encoder.stages]
        dec = [[c for c in st.convs] for st in self.decoder.stages]
        return enc, dec

    def set_selected_classes(self, idx):
        """Fuses map_label(..., 'logits') (torch_utils.py:214-221) into the head: forward returns only these rows."""
        self.selected_classes = None if idx is None else torch.as_tensor(idx, dtype=torch.int32)

    def _no_deep_supervision(self, what):
        if self.deep_supervision:
            raise ValueError(f"{what} does not combine with deep_supervision=True (the fused kernels know one head): "
                             "switch net.deep_supervision off first")

    @contextlib.contextmanager
    def _during(self, attr, make):
        """Context behind the fuse_* methods: attribute `attr` holds make() inside the block and None after it."""
        setattr(self, attr, make())
        try:
            yield
        finally:
            setattr(self, attr, None)

    # -- head fused with the inverse warp of its logits (csrc/warp.hip: head_warp_*_kernel)
    def can_fuse_output_warp(self, x_shape, theta_host):
        """True when `forward` can hand back the logits already warped by theta (R_inverse, zeros padding, the TTA grid
        algebra): 16-bit storage, 32 head input channels, 4 / 8 / 12 / 16 selected classes, maps the gather kernel accepts."""
        if os.environ.get("DGTTA_FUSE_HEAD_WARP", "1") == "0" or self.selected_classes is None:
            return False
        if self.act_dtype not in (torch.float16, torch.bfloat16):
            return False
        b, _, d, h, w = x_shape
        th = theta_host.detach().float().contiguous()
        if tuple(th.shape) != (b, 3, 4) or th.is_cuda:
            return False
        head = self.decoder.seg_layers[-1]
        return bool(_lib.load().dgtta_seghead_warp_supported(th.data_ptr(), b, head.in_channels, int(self.selected_classes.numel()),
                                                             d, h, w, dtype_code(self.act_dtype)))

    def fuse_output_warp(self, theta_dev, theta_host):
        """Context: the next forward returns affine_warp(logits, theta, zeros, tta_grid_algebra) computed by the fused
        head + warp kernels (and its backward runs the fused gather).  Check can_fuse_output_warp first."""
        self._no_deep_supervision("fuse_output_warp")
        return self._during("_fused_warp", lambda: (theta_dev.float().contiguous(), theta_host.detach().float().contiguous()))

    # -- head fused with the Gaussian window accumulation of the sliding-window inference (csrc/window_logits.hip)
    def can_fuse_window_accumulate(self):
        return (os.environ.get("DGTTA_FUSE_HEAD_ACCUMULATE", "1") != "0" and self.selected_classes is None and
                self.act_dtype in (torch.float16, torch.bfloat16) and self.decoder.seg_layers[-1].in_channels == 32 and
                self.decoder.seg_layers[-1].out_channels <= 112 and not torch.is_grad_enabled())

    def fuse_window_accumulate(self, acc, nsum, gauss, origins, *, mirrors=None):
        """Context (inference, no grad): the next forward adds gauss * logits of window k of the batch into
        acc [X,Y,Z,ncls] / nsum [X,Y,Z] at origins[k] instead of returning the logits (it returns an empty placeholder).
        mirrors: one mirror mask per origin (bit a = the window was fed flipped along axis a: its logits are un-flipped on the
        way into the accumulator, the Gaussian is not); fp32 accumulators only."""
        mirrors = self._window_mirrors(mirrors, origins, "fuse_window_accumulate")
        if any(mirrors) and acc.dtype != torch.float32:
            raise ValueError("fuse_window_accumulate: mirrored windows need the fp32 accumulator (eight passes per window at "
                             "Gaussian weight 10 leave no headroom in half)")
        if acc.dtype not in (torch.float32, torch.float16):      # the kernel knows these two accumulator storage types
            raise ValueError(f"fuse_window_accumulate: the accumulator is fp32 or fp16, not {acc.dtype}")
        if not (acc.is_contiguous() and nsum.dtype == torch.float32 and gauss.dtype == torch.float32):
            raise ValueError("fuse_window_accumulate: contiguous accumulator, fp32 weight sum and fp32 Gaussian expected")
        self._no_deep_supervision("fuse_window_accumulate")
        return self._during("_window_acc", lambda: WindowSink(acc, nsum, gauss, list(origins), mirrors, "logits"))

    @staticmethod
    def _window_mirrors(mirrors, origins, what):
        mirrors = [0] * len(origins) if mirrors is None else [int(m) for m in mirrors]
        if len(mirrors) != len(origins) or any(not 0 <= m <= 7 for m in mirrors):
            raise ValueError(f"{what}: one mirror mask in 0..7 per origin expected")
        return mirrors

    # -- the same in FEATURE space (csrc/window_features.hip): the head is linear and last, so the window accumulator
    #    holds the Gaussian-weighted input of the head and the head runs once per voxel at the end
    def can_fuse_window_feature_accumulate(self):
        return (os.environ.get("DGTTA_FUSE_HEAD_ACCUMULATE", "1") != "0" and self.selected_classes is None and
                self.decoder.seg_layers[-1].in_channels == 32 and not torch.is_grad_enabled())

    def fuse_window_feature_accumulate(self, facc, nsum, gauss, origins, *, mirrors=None):
        """Context (inference, no grad): the next forward adds gauss * z of window k of the batch - z = the 32 feature channels the
        segmentation head reads - into facc [X,Y,Z,32] (fp32) / nsum [X,Y,Z] at origins[k]; the head is NOT evaluated (the forward
        returns an empty placeholder).  Label map: ops.feature_head_argmax with the members' head weights.  mirrors: as in
        fuse_window_accumulate."""
        mirrors = self._window_mirrors(mirrors, origins, "fuse_window_feature_accumulate")
        if not (facc.dtype == torch.float32 and facc.is_contiguous() and facc.shape[-1] == 32 and nsum.dtype == torch.float32 and
                gauss.dtype == torch.float32):
            raise ValueError("fuse_window_feature_accumulate: contiguous fp32 accumulator [X,Y,Z,32], fp32 weight sum and Gaussian expected")
        self._no_deep_supervision("fuse_window_feature_accumulate")
        return self._during("_window_acc", lambda: WindowSink(facc, nsum, gauss, list(origins), mirrors, "features"))

    def forward(self, x):
        sel = self.selected_classes
        if sel is not None and sel.device != x.device:
            sel = self.selected_classes = sel.to(x.device)
        ds = bool(self.deep_supervision)
        if ds and (self._fused_warp is not None or self._window_acc is not None):      # switched on inside a fuse_* context
            self._no_deep_supervision("fuse_output_warp" if self._fused_warp is not None else "a fuse_window_* context")
        params = [p for p in self.parameters()]
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        # With the head fused into the inverse warp and 16-bit storage, the network's backward can take the gradient of
        # its output in the storage type (half the bytes for the fused gather).  autograd hands gradients over in the OUTPUT's
        # dtype (fp32), so the offer travels beside the output tensor: a loss that knows it (ops.consistency_loss on the batched
        # pair) leaves its 16-bit gradient in the sink and returns a stride-0 placeholder; anything else is summed as usual.
        sink = None
        if (need_grad and self._fused_warp is not None and self.act_dtype in (torch.bfloat16, torch.float16)
                and os.environ.get("DGTTA_GRAD16", "1") != "0"):
            sink = Grad16Sink(self.act_dtype)
        y = _UNetFn.apply(self, x, sel, need_grad, sink, ds, *params)
        if sink is not None:
            y._dgtta_grad16 = sink
        return y

    # -- packed weights (re-packed only when the parameter changed)
    def _cached_pack(self, key, w, dt, nbytes, pack):
        """The packed-weight cache: the blob under `key`, made anew - nbytes() bytes in storage format dt, filled by pack(blob) -
        when the parameter w changed or moved."""
        ent = self._packed.get(key)
        if ent is not None and ent[0] == w._version and ent[1].device == w.device:
            return ent[1]
        tdt = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[dt]
        wpack = torch.empty(nbytes() // tdt.itemsize, dtype=tdt, device=w.device)
        pack(wpack)
        self._packed[key] = (w._version, wpack)
        return wpack

    def packed(self, conv, dt, cinp, coutp, cin_slice=None):
        """Packed weight blob of `conv` in storage format dt (F32 | BF16 | F16), re-packed only when the parameter changed.
        cin_slice = (lo, hi): the blob of the conv restricted to input channels lo..hi-1 (cinp = its padded count) - the data
        gradient of a conv on a concat buffer is evaluated half by half (see unet_exec._concat_grad)."""
        w, lib = conv.weight, _lib.load()

        def pack(wpack):
            wsrc = w.detach() if cin_slice is None else w.detach()[:, cin_slice[0]:cin_slice[1]].contiguous()
            check(lib.dgtta_conv3d_pack_weights(ptr(wsrc), ptr(wpack), wsrc.shape[1], conv.out_channels,
                                                cinp, coutp, dt, stream_of(w.device)), "dgtta_conv3d_pack_weights")
        return self._cached_pack((id(w), dt, cinp, coutp, cin_slice), w, dt,
                                 lambda: lib.dgtta_conv3d_packed_bytes(cinp, coutp, dt), pack)

    def kpacked(self, conv, dt, cinp, coutp):
        """Packed weight blob of an anisotropic conv (dgtta_conv3d_kpack_weights), re-packed only when the parameter changed."""
        w, lib = conv.weight, _lib.load()
        kd, kh, kw = conv.kernel_size

        def pack(wpack):
            wsrc = w.detach().contiguous()
            check(lib.dgtta_conv3d_kpack_weights(ptr(wsrc), ptr(wpack), kd, kh, kw, conv.in_channels, conv.out_channels, cinp, coutp,
                                                 dt, stream_of(w.device)), "dgtta_conv3d_kpack_weights")
        return self._cached_pack((id(w), dt, cinp, coutp, "k"), w, dt,
                                 lambda: lib.dgtta_conv3d_kpacked_bytes(kd, cinp, coutp, dt), pack)


class Grad16Sink:
    """Side channel for the gradient of the network output in the 16-bit storage type (see HipPlainConvUNet.forward):
    `put` by the loss backward, taken by _UNetFn.backward of the same pass."""

    def __init__(self, dtype):
        self.dtype, self.g16, self.claimed = dtype, None, False

    def claim(self):
        """ONE consumer of the output may use the channel (a second sink-aware loss on the same output takes the fp32 route, so
        that autograd sums its dense gradient with the first one's instead of one `put` overwriting the other)."""
        if self.claimed:
            return False
        self.claimed = True
        return True

    def put(self, g16):
        self.g16 = g16

    def take(self):
        g, self.g16 = self.g16, None
        return g


def set_probe(model, where):
    """bench.py hook: record (start, end) events around the forward conv launch and the weight-gradient launch (sweep + slab
    reduction, on the stream it runs on) of block `where` = (kind, stage, idx) of `model` (None: stop).  Returns the probe dict
    (events are appended to probe["events"] / probe["wgrad_events"] while the model runs)."""
    st = state_of(model)
    st.probe = None if where is None else dict(where=where, events=[])
    return st.probe
