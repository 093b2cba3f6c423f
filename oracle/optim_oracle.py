"""Float64 restatements (numpy only) of what ``csrc/dir_optim.hip`` computes: one optimizer step of ``torch.optim.Adam`` /
``torch.optim.SGD`` (the arithmetic of torch's single-tensor paths, ``adam.py: _single_tensor_adam`` without amsgrad and
``sgd.py: _single_tensor_sgd``), and the two bf16 operands the convolution kernels read (``dir_conv_prep_weights*``).

Float32 inputs are widened to float64 and every operation is done there; the hyperparameters stay Python doubles and the bias
corrections are formed as torch forms them (``1 - beta ** step``, ``bias_correction2 ** 0.5``), so the only error of these functions is
float64 round-off. The layouts are written from their description (the header comment of ``dir_optim.hip`` and the torch flip / permute
and parity-class formulation of ``tests/test_hip_conv.py``) with numpy slicing and transposes: no index arithmetic is shared with the kernel.
"""
import numpy as np


def _f64(x):
    return np.asarray(x).astype(np.float64)


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
    """One Adam step (L2 weight decay, no amsgrad). ``step`` is the count AFTER the increment (>= 1). Returns ``(p, exp_avg, exp_avg_sq)``."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    if weight_decay != 0:
        g = g + weight_decay * p                                   # grad.add(param, alpha=weight_decay)
    m = m + (1 - beta1) * (g - m)                                  # exp_avg.lerp_(grad, 1 - beta1)
    v = v * beta2 + (1 - beta2) * g * g                            # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    step_size = lr / bias_correction1
    bias_correction2_sqrt = bias_correction2 ** 0.5
    denom = np.sqrt(v) / bias_correction2_sqrt + eps               # (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p - step_size * (m / denom)                                # param.addcdiv_(exp_avg, denom, value=-step_size)
    return p, m, v


def sgd_step(p, g, buf, lr, momentum, dampening, weight_decay, nesterov):
    """One SGD step. ``buf`` is the momentum buffer or ``None`` (no momentum, or the first step with momentum: torch then starts the
    buffer as a copy of the gradient). Returns ``(p, momentum_buffer or None)``."""
    p, g = _f64(p), _f64(g)
    if weight_decay != 0:
        g = g + weight_decay * p                                   # grad.add(param, alpha=weight_decay)
    if momentum != 0:
        if buf is None:
            buf = g.copy()                                         # clone(grad)
        else:
            buf = _f64(buf) * momentum + (1 - dampening) * g       # buf.mul_(momentum).add_(grad, alpha=1 - dampening)
        g = g + momentum * buf if nesterov else buf
    else:
        buf = None
    return p - lr * g, buf                                         # param.add_(grad, alpha=-lr)


def prep_w16(w):
    """bf16 bit patterns (uint16, same shape) of a float32 array: round to nearest, ties to even; a NaN keeps its sign and upper payload
    bits and gets its quiet bit set (it never rounds to an infinity)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    u = w.view(np.uint32).astype(np.uint64)
    hi = u >> 16
    rounded = (u + 0x7FFF + (hi & 1)) >> 16                         # + half an ulp, less one when the kept part is even
    is_nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(is_nan, hi | 0x40, rounded).astype(np.uint16)


def prep_w16_rot(w, rot_mode):
    """The data-gradient operand of a float32 ``[Cout][R][S][Cin]`` master weight, as a flat uint16 array of bf16 bit patterns.

    ``rot_mode`` 0: ``[Cin][R][S][Cout]`` with the taps rotated by 180 degrees (the stride-1 data gradient is a convolution with it).
    ``rot_mode`` 1 (3x3): the four parity classes of the stride-2 data gradient, packed back to back in the order (0,0) (0,1) (1,0) (1,1).
    Class ``(a, b)`` serves the input pixels ``(2 i + a, 2 j + b)``: along an axis, parity 0 is reached by the centre tap alone and parity 1
    by the outer taps, last one first (filter index 2, then 0). Each class is ``[Cin][taps along R][taps along S][Cout]``."""
    w = np.asarray(w)
    assert w.ndim == 4, w.shape
    h = prep_w16(w)                                                 # [Cout][R][S][Cin]
    if rot_mode == 0:
        return np.ascontiguousarray(h[:, ::-1, ::-1, :].transpose(3, 1, 2, 0)).reshape(-1)
    assert rot_mode == 1 and w.shape[1:3] == (3, 3), (rot_mode, w.shape)
    taps = ([1], [2, 0])
    pieces = []
    for a in (0, 1):
        for b in (0, 1):
            sub = h[:, taps[a], :, :][:, :, taps[b], :]            # [Cout][1 + a][1 + b][Cin]
            pieces.append(np.ascontiguousarray(sub.transpose(3, 1, 2, 0)).reshape(-1))
    return np.concatenate(pieces)
