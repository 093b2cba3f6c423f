"""Shared by tests/test_optim_oracle_host.py (CPU) and tests/test_hip_optim_exact.py (-m gpu): the rows, hyperparameter settings and
fixed-seed inputs of the optimizer-step tests, the COUNTED per-element error bounds of one float32 step against oracle/optim_oracle.py,
and the deliberately wrong formulas the bounds must tell apart from the right one.

The bounds (first order, every term a product of exactly known float64 quantities; u = 2**-24)
------------------------------------------------------------------------------------------------
Each float32 operation contributes half an ulp of its result, |result| * u at the most; each hyperparameter that reaches the arithmetic
as a float32 contributes one relative u to whatever it multiplies. These are pushed through the derivatives of the operations that
follow. A fused multiply-add is charged as its two operations, so a bound holds whether ``a + alpha * b`` is contracted (torch's
kernels, ``sgd_update``) or not (``adam_update``). There is no array-scale term: an element far below its tensor's maximum is held to its
own magnitude. The first-order sum is multiplied by 1 + 2**-16 for the second-order terms (products of two of the <= 20 relative
errors of 6e-8 each: below 2e-6 of the sum).

Adam, ``adam_bound``. G = g + wd p, D = G - m, T = (1-b1) D, M = m + T, A = v b2, B = (1-b2) G^2, V = A + B, S = sqrt V, Q = S / c2,
N = Q + eps, R = M / N, X = ss R, P = p - X (c2 = bias_correction2 ** 0.5, ss = lr / bias_correction1):
    E_G = u (2 |wd p| + |G|)                         wd rounded, multiply, add            (0 when wd = 0: no operation)
    E_M = (1-b1) (E_G + u |D|) + 2 u |T| + u |M|     subtract; 1-b1 rounded, multiply; add                     -> exp_avg
    E_V = 2 u A + (1-b2) (2 |G| E_G + u G^2) + 2 u B + u V      b2 rounded, multiply; square; 1-b2 rounded, multiply; add -> exp_avg_sq
    E_S = E_V / (2 S) + u S                          correctly rounded sqrtf               (0 when V = 0)
    E_N = E_S / c2 + 3 u Q + u eps + u N             c2 rounded, divide (charged twice: a kernel that multiplies by the float32
                                                     reciprocal, as torch's device kernels do for a scalar divisor, rounds twice); eps rounded; add
    E_P = ss (E_M / N + |R| E_N / N + u |R|) + 2 u |X| + u |P|   divide; ss rounded, multiply; subtract         -> parameter
SGD, ``sgd_bound``. G = g + wd p, B = mom b + (1-damp) G (first step: B = G), H = G + mom B (Nesterov) or B, P = p - lr H:
    E_G = u (2 |wd p| + |G|)
    E_B = 2 u |mom b| + (1-damp) E_G + 2 u |(1-damp) G| + u |B|        (first step: E_B = E_G, a copy)          -> momentum_buffer
    E_H = E_G + mom E_B + 2 u |mom B| + u |H|                           (no Nesterov: E_H = E_B; no momentum: E_H = E_G)
    E_P = lr E_H + 2 u |lr H| + u |P|                                                                            -> parameter
"""
import functools
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -16

Row = namedtuple("Row", "numel cout cin r rot_mode has_rot")            # cout == 0: a plain row
PLAIN_NUMELS = [1, 63, 64, 65, 255, 256, 257, 32768, 32769, 100003]    # 32768 = one sweep of the 128 x 256 grid
CONV_ROWS = [(64, 64, 1, 0, True),        # one tile
             (128, 64, 3, 1, True),       # stride-2 classes, Cin != Cout
             (64, 128, 3, 0, True),
             (128, 192, 3, 1, True),
             (256, 256, 3, 0, True),      # 144 tiles > 128 workgroups
             (64, 64, 7, 0, False),       # null w16_rot, RS = 49
             (48, 32, 3, 0, True),        # generic branch
             (80, 48, 3, 1, True),        # generic branch
             (64, 32, 1, 0, True),        # generic branch, only Cin not a multiple of 64
             (8, 3, 7, 0, False)]         # generic branch, no w16_rot
# plain and convolution rows interleaved, so a table row's kind does not follow from its position
ROWS = [r for pair in zip([Row(n, 0, 0, 0, 0, False) for n in PLAIN_NUMELS],
                          [Row(co * r * r * ci, co, ci, r, mode, rot) for co, ci, r, mode, rot in CONV_ROWS]) for r in pair]

# (lr, (beta1, beta2), eps, weight_decay, first step count)
ADAM_SETTINGS = [(1e-3, (0.9, 0.999), 1e-8, 0.0, 1),
                 (1e-3, (0.9, 0.999), 1e-8, 1e-4, 2),
                 (0.1, (0.5, 0.9), 1e-3, 1e-2, 7),
                 (1e-3, (0.0, 0.999), 1e-8, 0.0, 3),
                 (1e-3, (0.9, 0.999), 1e-8, 1e-4, 100000)]
SGD_LR = 1e-2
# (momentum, weight_decay, nesterov, dampening): the four settings of tests/test_hip_optim.py
SGD_SETTINGS = [(0.9, 1e-4, False, 0.0), (0.0, 0.0, False, 0.0), (0.9, 0.0, True, 0.0), (0.8, 1e-3, False, 0.1)]
# (setting, first): every setting from a fresh buffer and from a non-trivial one; momentum = 0 has no buffer at all
SGD_CASES = [(s, first) for s in SGD_SETTINGS for first in ((1, 0) if s[0] else (0,))]
NSTEPS = 3


# ----------------------------------------------------------------------------------------------------------------- inputs
def _signed_log_uniform(rng, n, lo, hi):
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo, hi, n)).astype(np.float32)


def _fixed(fn):
    """Inputs are made once per process and shared read-only."""
    @functools.lru_cache(maxsize=None)
    def cached(*args):
        out = fn(*args)
        for a in (out if isinstance(out, tuple) else (out,)):
            a.setflags(write=False)
        return out
    return functools.wraps(fn)(cached)


def _zero_runs(n):
    """(always, later): index ranges whose gradient is an exact zero at every step (their state is zero too: zero on zero), and from
    the second step on (zero on non-zero state). Tensors below 16 elements have none."""
    if n < 16:
        return (0, 0), (0, 0)
    return (n // 8, n // 8 + max(1, n // 16)), (n // 2, n // 2 + max(1, n // 16))


@_fixed
def make_param(row, n):
    return _signed_log_uniform(np.random.default_rng([11, row]), n, -3.0, 0.3)


@_fixed
def make_grad(row, n, k):
    """Gradient of step ``k`` (0-based): magnitudes 1e-12 .. 1e4, log-uniform; runs of +0 and -0 (see ``_zero_runs``)."""
    g = _signed_log_uniform(np.random.default_rng([12, row, k]), n, -12.0, 4.0)
    always, later = _zero_runs(n)
    for lo, hi in (always,) + ((later,) if k >= 1 else ()):
        g[lo:hi] = 0.0
        g[lo:hi:2] = -0.0
    return g


@_fixed
def make_adam_state(row, n, zero):
    """(exp_avg, exp_avg_sq): zeros for a run that starts at step 1, otherwise what earlier steps could have left (exp_avg_sq >= 0)."""
    if zero:
        return np.zeros(n, np.float32), np.zeros(n, np.float32)
    rng = np.random.default_rng([13, row])
    m = _signed_log_uniform(rng, n, -8.0, 2.0)
    v = (_signed_log_uniform(rng, n, -8.0, 2.0).astype(np.float64) ** 2 * rng.uniform(0.25, 4.0, n)).astype(np.float32)
    lo, hi = _zero_runs(n)[0]
    m[lo:hi] = 0.0
    v[lo:hi] = 0.0
    return m, v


@_fixed
def make_sgd_buffer(row, n):
    b = _signed_log_uniform(np.random.default_rng([14, row]), n, -8.0, 2.0)
    lo, hi = _zero_runs(n)[0]
    b[lo:hi] = 0.0
    return b


SPECIAL_BITS = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # exact ties: kept part even / odd, both signs
                         0x3F807FFF, 0x3F808001, 0x00000000, 0x80000000,      # just below / above a tie, +0, -0
                         0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF,      # +-inf, the largest finite floats (round to +-inf)
                         0x7F7F7FFF, 0x7F7F8000,                              # the largest float that stays finite, the tie above it
                         0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF80FFFF,      # quiet NaNs, signalling NaNs with a low-half payload
                         0x7FFFFFFF, 0x7FA55555], dtype=np.uint32)


@_fixed
def make_prep_weight(row, n):
    """Master weight for the un-fused preparation calls: random values with every entry of ``SPECIAL_BITS`` planted at positions
    spread over the tensor (so they fall into different tiles, rows and lanes)."""
    w = np.random.default_rng([15, row]).standard_normal(n).astype(np.float32)
    k = len(SPECIAL_BITS)
    if n >= 4 * k:
        pos = np.arange(k) * (n // k) + np.arange(k) % (n // k)
        w.view(np.uint32)[pos] = SPECIAL_BITS
    return w


# ----------------------------------------------------------------------------------------------------------------- bounds
def adam_bound(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
    """Per-element bounds ``(E_P, E_M, E_V)`` of one float32 Adam step against ``optim_oracle.adam_step`` (module docstring)."""
    p, g, m, v = (np.asarray(a).astype(np.float64) for a in (p, g, m, v))
    ab = np.abs
    G, E_G = g, np.zeros_like(g)
    if weight_decay != 0:
        G = g + weight_decay * p
        E_G = U * (2 * ab(weight_decay * p) + ab(G))
    D = G - m
    T = (1 - beta1) * D
    M = m + T
    E_M = (1 - beta1) * (E_G + U * ab(D)) + 2 * U * ab(T) + U * ab(M)
    A, B = v * beta2, (1 - beta2) * G * G
    V = A + B
    E_V = 2 * U * A + (1 - beta2) * (2 * ab(G) * E_G + U * G * G) + 2 * U * B + U * V
    S = np.sqrt(V)
    E_S = np.where(V > 0, E_V / (2 * np.where(V > 0, S, 1.0)) + U * S, 0.0)
    c2 = (1 - beta2 ** step) ** 0.5
    ss = lr / (1 - beta1 ** step)
    Q = S / c2
    N = Q + eps
    E_N = E_S / c2 + 3 * U * Q + U * eps + U * N
    R = M / N
    X = ss * R
    P = p - X
    E_P = ss * (E_M / N + ab(R) * E_N / N + U * ab(R)) + 2 * U * ab(X) + U * ab(P)
    return E_P * SECOND_ORDER, E_M * SECOND_ORDER, E_V * SECOND_ORDER


def sgd_bound(p, g, buf, lr, momentum, dampening, weight_decay, nesterov):
    """Per-element bounds ``(E_P, E_B or None)`` of one float32 SGD step against ``optim_oracle.sgd_step`` (module docstring)."""
    p, g = np.asarray(p).astype(np.float64), np.asarray(g).astype(np.float64)
    ab = np.abs
    G, E_G = g, np.zeros_like(g)
    if weight_decay != 0:
        G = g + weight_decay * p
        E_G = U * (2 * ab(weight_decay * p) + ab(G))
    H, E_H, E_B = G, E_G, None
    if momentum != 0:
        if buf is None:
            B, E_B = G, E_G
        else:
            b = np.asarray(buf).astype(np.float64)
            B = momentum * b + (1 - dampening) * G
            E_B = 2 * U * ab(momentum * b) + (1 - dampening) * E_G + 2 * U * ab((1 - dampening) * G) + U * ab(B)
        if nesterov:
            H = G + momentum * B
            E_H = E_G + momentum * E_B + 2 * U * ab(momentum * B) + U * ab(H)
        else:
            H, E_H = B, E_B
    P = p - lr * H
    E_P = lr * E_H + 2 * U * ab(lr * H) + U * ab(P)
    return E_P * SECOND_ORDER, None if E_B is None else E_B * SECOND_ORDER


def worst_fraction(got, want, bound):
    """max |got - want| / bound over the elements (0 / 0 = 0: an exact result where the bound is zero); inf if one is off where the bound is 0."""
    err = np.abs(np.asarray(got).astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(err == 0, 0.0, err / bound)
    return float(frac.max()) if frac.size else 0.0


# ----------------------------------------------------------------------------------------------------------------- wrong formulas
def _adam_variant(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, wrong):
    p, g, m, v = (np.asarray(a).astype(np.float64) for a in (p, g, m, v))
    if weight_decay != 0 and wrong != "adamw":
        g = g + weight_decay * p
    m = m + (beta1 if wrong == "lerp_beta1" else 1 - beta1) * (g - m)
    v = v * beta2 + (1 - beta2) * g * g
    c1 = 1.0 if wrong == "no_bias_correction1" else 1 - beta1 ** step
    c2 = 1.0 if wrong == "no_bias_correction2" else (1 - beta2 ** step) ** 0.5
    denom = (np.sqrt(v) + eps) / c2 if wrong == "eps_before_division" else np.sqrt(v) / c2 + eps
    if wrong == "adamw":
        p = p * (1 - lr * weight_decay)
    return p - lr / c1 * (m / denom), m, v


def _sgd_variant(p, g, buf, lr, momentum, dampening, weight_decay, nesterov, wrong):
    p, g = np.asarray(p).astype(np.float64), np.asarray(g).astype(np.float64)
    if weight_decay != 0:
        g = g + weight_decay * p
    if momentum != 0:
        if buf is None:
            buf = (1 - dampening) * g if wrong == "first_buffer_dampened" else g.copy()
        elif wrong == "momentum_on_new_buffer":
            buf = momentum * (np.asarray(buf).astype(np.float64) + (1 - dampening) * g)
        else:
            buf = np.asarray(buf).astype(np.float64) * momentum + (1 - dampening) * g
        if nesterov:
            g = buf if wrong == "nesterov_buffer_alone" else g + momentum * buf
        else:
            g = buf
    else:
        buf = None
    return p - lr * g, buf


ADAM_WRONG = ["eps_before_division", "no_bias_correction1", "no_bias_correction2", "adamw", "lerp_beta1"]
SGD_WRONG = ["first_buffer_dampened", "nesterov_buffer_alone", "momentum_on_new_buffer"]


def adam_wrong(wrong, *args):
    assert wrong in ADAM_WRONG
    return _adam_variant(*args, wrong=wrong)


def sgd_wrong(wrong, *args):
    assert wrong in SGD_WRONG
    return _sgd_variant(*args, wrong=wrong)

