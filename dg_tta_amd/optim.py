"""Optimisers on the multi-tensor HIP kernels: HipAdamW (csrc/adamw.hip) for test-time adaptation, HipSGD + PolyLRScheduler
(csrc/sgd.hip) for source-domain pre-training.  HipAdamW: stand-in for `torch.optim.AdamW(model.parameters(), lr)`
of dg_tta/tta/tta.py:185 with PyTorch's defaults; state layout (`step`, `exp_avg`, `exp_avg_sq`) matches torch's so
optimizer state dicts are interchangeable.  Parameters whose .grad is None are skipped, as PyTorch does."""
import torch

from . import ops


class HipAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0,
                 min_grad_scale=1.0):
        """grad_scale: loss scale carried by the gradients (fp16 storage path, HipPlainConvUNet.loss_scale); the kernel
        divides it out on load, so state and parameters are those of the unscaled problem.  With grad_scale != 1 every
        step is guarded: when a gradient is inf / NaN the kernel leaves parameters and state untouched, and the next
        `resolve_overflow()` (called by tta_epoch at the start of an epoch, when the stream is drained anyway) halves the
        scale and takes the skipped step out of the step counters.  The guard belongs to the 16-bit path, not to the value
        of the scale: it stays on when the scale has decayed to min_grad_scale = 1."""
        self.grad_scale = float(grad_scale)
        self.guarded = float(grad_scale) != 1.0
        self.min_grad_scale = float(min_grad_scale)
        self.skipped_steps = 0
        self._flag = None               # int32 device scalar of the last guarded step
        self._pending = []              # parameters whose step counter that step advanced
        if lr < 0.0 or eps < 0.0 or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0) or weight_decay < 0.0:
            raise ValueError("invalid AdamW hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def resolve_overflow(self):
        """Reads the overflow flag of the last guarded step (one small device->host copy).  True: that step was skipped;
        the loss scale is halved (not below min_grad_scale) and the step counters are rolled back."""
        if self._flag is None:
            return False
        bad = bool(self._flag.item())
        if bad:
            for p in self._pending:
                self.state[p]["step"] = int(self.state[p]["step"]) - 1
            self.skipped_steps += 1
            self.grad_scale = max(self.grad_scale * 0.5, self.min_grad_scale)
        self._flag, self._pending = None, []
        return bad

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # the gradients of THIS step carry the scale that was in force when they were produced: settling an unread flag of
        # the previous step may halve self.grad_scale, which then applies to the NEXT backward (a caller that reads
        # `grad_scale` for its loss only after step(), e.g. tta_epoch, sees one consistent value)
        scale_now = self.grad_scale
        self.resolve_overflow()
        guarded = self.guarded
        work = []                        # (group, step, params)
        for group in self.param_groups:
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("HipAdamW does not support sparse gradients")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] = int(st["step"]) + 1
                if not p.is_contiguous() or not p.grad.is_contiguous():
                    raise RuntimeError("HipAdamW needs contiguous parameters and gradients")
                by_step.setdefault(st["step"], []).append(p)
            work.extend((group, step, ps) for step, ps in by_step.items())
        flag = None
        if guarded and work:             # all or nothing: one flag over every gradient of this step
            flag = torch.zeros((), dtype=torch.int32, device=work[0][2][0].device)
            ops.grads_nonfinite([p.grad for _, _, ps in work for p in ps], flag)
        for group, step, ps in work:
            ops.adamw_step([p.data for p in ps], [p.grad for p in ps], [self.state[p]["exp_avg"] for p in ps],
                           [self.state[p]["exp_avg_sq"] for p in ps], step, group["lr"], group["betas"],
                           group["eps"], group["weight_decay"], scale_now, skip_flag=flag)
            # the kernel wrote through raw pointers: tell autograd / weight caches that the tensors changed
            torch.autograd.graph.increment_version(ps)
            if guarded:
                self._pending.extend(ps)
        self._flag = flag
        return loss


class HipSGD(torch.optim.Optimizer):
    """nnU-Net's optimiser on the multi-tensor HIP kernels (csrc/sgd.hip): torch.nn.utils.clip_grad_norm_(params,
    max_grad_norm) followed by torch.optim.SGD(lr, momentum, nesterov, weight_decay) with dampening 0, in one norm pass and
    one fused update pass; the norm stays on the device.  The state key is `momentum_buffer`, so state dicts interchange
    with torch.optim.SGD.  Parameters whose .grad is None are skipped and do not enter the norm (as clip_grad_norm_ and SGD
    do).  max_grad_norm=None: no clipping.  grad_scale / min_grad_scale / resolve_overflow() / skipped_steps: HipAdamW's
    overflow protocol for the fp16 storage path; a skipped step that would have been a parameter's first leaves its
    momentum buffer uninitialised, so the next clean step is its first."""

    def __init__(self, params, lr=1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5, max_grad_norm=12.0, grad_scale=1.0,
                 min_grad_scale=1.0):
        self.grad_scale = float(grad_scale)
        self.guarded = float(grad_scale) != 1.0
        self.min_grad_scale = float(min_grad_scale)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skipped_steps = 0
        self._flag = None               # int32 device scalar of the last guarded step
        self._pending = []              # parameters whose momentum buffer that step created
        self._ws = None                 # workspace of the norm pass, kept between steps
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0 or (self.max_grad_norm is not None and self.max_grad_norm <= 0.0):
            raise ValueError("invalid SGD hyper-parameter")
        if nesterov and momentum <= 0.0:
            raise ValueError("Nesterov momentum requires a momentum")
        # dampening is carried (always 0) because torch.optim.SGD reads it from a loaded state dict's param_groups
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0.0, weight_decay=weight_decay, nesterov=nesterov))

    def resolve_overflow(self):
        """Reads the overflow flag of the last guarded step (one small device->host copy).  True: that step was skipped;
        the loss scale is halved (not below min_grad_scale) and the momentum buffers it created are dropped again."""
        if self._flag is None:
            return False
        bad = bool(self._flag.item())
        if bad:
            for p in self._pending:
                self.state[p].pop("momentum_buffer", None)
            self.skipped_steps += 1
            self.grad_scale = max(self.grad_scale * 0.5, self.min_grad_scale)
        self._flag, self._pending = None, []
        return bad

    def state_dict(self):
        self.resolve_overflow()          # a buffer created by a step that turns out skipped is not state
        return super().state_dict()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        scale_now = self.grad_scale      # the scale THESE gradients carry (see HipAdamW.step)
        self.resolve_overflow()
        work = []                        # (group, first_step, params)
        for group in self.param_groups:
            if group.get("dampening", 0.0) != 0.0 or group.get("maximize", False):
                raise RuntimeError("HipSGD implements dampening 0 and minimisation only")
            first, later = [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("HipSGD does not support sparse gradients")
                ops.require_cuda(p, p.grad)
                if not p.is_contiguous() or not p.grad.is_contiguous():
                    raise RuntimeError("HipSGD needs contiguous parameters and gradients")
                (later if self.state[p].get("momentum_buffer") is not None else first).append(p)
            work.extend((group, f, ps) for f, ps in ((True, first), (False, later)) if ps)
        if not work:
            return loss
        grads = [p.grad for _, _, ps in work for p in ps]
        device = grads[0].device
        flag = None
        if self.guarded:                 # all or nothing: one flag over every gradient of this step
            flag = torch.zeros((), dtype=torch.int32, device=device)
            ops.grads_nonfinite(grads, flag)
        sumsq = None
        if self.max_grad_norm is not None:
            need = ops.grad_sumsq_ws_bytes(sum(g.numel() for g in grads), len(grads))
            if self._ws is None or self._ws.numel() < need or self._ws.device != device:
                self._ws = torch.empty(need, dtype=torch.uint8, device=device)
            sumsq = ops.grad_sumsq(grads, ws=self._ws)
        for group, first, ps in work:
            if first:
                for p in ps:             # written, never read, by the first step
                    self.state[p]["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                if self.guarded:
                    self._pending.extend(ps)
            ops.sgd_step([p.data for p in ps], [p.grad for p in ps], [self.state[p]["momentum_buffer"] for p in ps],
                         group["lr"], group["momentum"], group["weight_decay"], group["nesterov"], first_step=first,
                         grad_scale=scale_now, sumsq=sumsq, max_norm=self.max_grad_norm or 1.0, skip_flag=flag)
            # the kernel wrote through raw pointers: tell autograd / weight caches that the tensors changed
            torch.autograd.graph.increment_version(ps)
        self._flag = flag
        return loss


class PolyLRScheduler:
    """nnU-Net's polynomial learning rate [3P nnunetv2 PolyLRScheduler, from memory: UNPINNED]:
    step(current_step) sets lr = initial_lr * (1 - current_step / max_steps) ** exponent on every parameter group."""

    def __init__(self, optimizer, initial_lr, max_steps, exponent=0.9):
        self.optimizer, self.initial_lr, self.max_steps, self.exponent = optimizer, float(initial_lr), int(max_steps), float(exponent)
        self.ctr = 0

    def lr_at(self, current_step):
        return self.initial_lr * (1 - current_step / self.max_steps) ** self.exponent

    def step(self, current_step=None):
        if current_step is None:
            current_step = self.ctr
        self.ctr = current_step + 1
        lr = self.lr_at(current_step)
        for group in self.optimizer.param_groups:
            group["lr"] = lr
        return lr
