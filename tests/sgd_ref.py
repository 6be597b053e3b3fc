"""Float64 numpy restatement of the clipped SGD step of csrc/sgd.hip (formula in include/dgtta.h):

    norm = sqrt(sumsq) * inv_scale
    coef = min(1, max_norm / (norm + 1e-6))          (1 when clipping is off)
    g'   = g * inv_scale * coef
    d    = g' + wd * p
    buf  = first_step ? d : mu * buf + d
    u    = nesterov ? d + mu * buf : buf
    p   -= lr * u

tests/test_sgd_ref.py checks it against torch.nn.utils.clip_grad_norm_ + torch.optim.SGD in float64;
tests/test_gpu_sgd.py checks the kernels against it.  Parameters whose gradient is None are skipped and do not enter
the norm."""
import numpy as np


def grad_sumsq(grads):
    """Sum of squares over every element of the gradients that are not None, in float64."""
    return float(sum(np.sum(np.asarray(g, dtype=np.float64) ** 2) for g in grads if g is not None))


def clip_coef(sumsq, max_norm, grad_scale=1.0):
    if max_norm is None:
        return 1.0
    norm = np.sqrt(np.float64(sumsq)) * (1.0 / grad_scale)
    return float(min(1.0, max_norm / (norm + 1e-6)))


def sgd_step(params, grads, bufs, lr, momentum=0.99, weight_decay=3e-5, nesterov=True, max_norm=12.0, grad_scale=1.0,
             sumsq=None):
    """One step on lists of float64 arrays.  bufs[i] is None before parameter i's first step (that step is then its
    `first_step`).  sumsq: the norm's sum of squares when the caller has it (e.g. the kernel's own, to isolate the update);
    default: computed here from `grads`.  Returns (new params, new bufs, coef); inputs are not modified."""
    if sumsq is None:
        sumsq = grad_sumsq(grads)
    coef = clip_coef(sumsq, max_norm, grad_scale)
    inv_scale = 1.0 / grad_scale
    new_p, new_b = [], []
    for p, g, b in zip(params, grads, bufs):
        p = np.asarray(p, dtype=np.float64)
        if g is None:
            new_p.append(p.copy())
            new_b.append(None if b is None else np.asarray(b, dtype=np.float64).copy())
            continue
        gc = np.asarray(g, dtype=np.float64) * inv_scale * coef
        d = gc + weight_decay * p
        b = d.copy() if b is None else momentum * np.asarray(b, dtype=np.float64) + d
        u = d + momentum * b if nesterov else b
        new_p.append(p - lr * u)
        new_b.append(b)
    return new_p, new_b, coef


def poly_lr(initial_lr, current_step, max_steps, exponent=0.9):
    return initial_lr * (1 - current_step / max_steps) ** exponent
