"""Float64 numpy restatement of the multi-tensor AdamW step of csrc/adamw.hip, in the order its header states:

    g'  = g * (1 / grad_scale)
    p   = p * (1 - lr wd)
    m   = m + (g' - m) (1 - b1)
    v   = v b2 + ((1 - b2) g') g'
    p   = p - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)),       bc1 = 1 - b1^step, bc2 = 1 - b2^step

tests/test_adamw_ref.py checks it against torch.optim.AdamW in float64; tests/test_gpu_adamw.py checks the kernels against
it.  Parameters whose gradient is None are skipped: p, m and v stay as they are."""
import ctypes

import numpy as np


def f32(x):
    return ctypes.c_float(x).value


def kernel_scalars(step, lr, b1, b2, eps, wd, grad_scale=1.0):
    """The scalars as the KERNEL receives them: the C ABI takes lr, b1, b2, eps, wd and grad_scale as fp32, forms lr * wd and
    1 / grad_scale in fp32, the bias corrections in double and rounds lr / bc1 and sqrt(bc2) to fp32 once.
    Returns (lr_wd, b1, b2, eps, step_size, sqrt_bc2, inv_scale) as Python floats holding fp32 values."""
    lr, b1, b2, eps, wd, grad_scale = (f32(x) for x in (lr, b1, b2, eps, wd, grad_scale))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return f32(lr * wd), b1, b2, eps, f32(lr / bc1), f32(np.sqrt(bc2)), f32(1.0 / grad_scale)


def exact_scalars(step, lr, b1, b2, eps, wd, grad_scale=1.0):
    """The same tuple without any rounding to fp32 (what torch.optim.AdamW computes with in float64)."""
    return lr * wd, b1, b2, eps, lr / (1.0 - b1 ** step), float(np.sqrt(1.0 - b2 ** step)), 1.0 / grad_scale


def adamw_step(params, grads, ms, vs, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, grad_scale=1.0,
               as_kernel=True):
    """One step on lists of float64 arrays; returns (new params, new ms, new vs), the inputs are not modified.
    as_kernel: use kernel_scalars (default) or exact_scalars."""
    lr_wd, b1, b2, eps, step_size, sqrt_bc2, inv_scale = (kernel_scalars if as_kernel else exact_scalars)(
        step, lr, betas[0], betas[1], eps, weight_decay, grad_scale)
    new_p, new_m, new_v = [], [], []
    for p, g, m, v in zip(params, grads, ms, vs):
        p, m, v = (np.asarray(x, dtype=np.float64) for x in (p, m, v))
        if g is None:
            new_p.append(p.copy()), new_m.append(m.copy()), new_v.append(v.copy())
            continue
        gi = np.asarray(g, dtype=np.float64) * inv_scale
        p = p * (1.0 - lr_wd)
        m = m + (gi - m) * (1.0 - b1)
        v = v * b2 + ((1.0 - b2) * gi) * gi
        denom = np.sqrt(v) / sqrt_bc2 + eps
        new_p.append(p - step_size * (m / denom))
        new_m.append(m)
        new_v.append(v)
    return new_p, new_m, new_v
