"""Rounding-aware float64 references of the BatchNorm, max-pool, stem-tail and stem weight-gradient kernels, and the bars the
tests hold those kernels to (a helper module, imported by tests/test_hip_bn_exact.py and tests/test_bf16_reference_host.py).

Every reference is plain torch float64 (CPU or GPU) and takes the kernel's own DISCRETE decisions as arguments where the exact
computation could decide otherwise by rounding alone: the ReLU mask (the kernel's own ``y > 0``), the max-pool route where the two
best candidates are within float32 rounding of each other, the bf16 dy the weight gradient is fed. Everything continuous is
computed exactly: batch statistics two-pass from the same bf16 / float32 input, sums in float64.

Bars (``ratio`` = max |got - ref| / bar, a test passes at ratio <= 1):
  * bf16 outputs: ``2^-8 |ref| + 1e-6 max|ref|`` = half a bf16 ulp plus float32 slack (+ ``extra`` where the output is formed from
    float32 sums: 2e-5 S of those sums, propagated);
  * float32 outputs of reductions: ``2e-5 S`` per element, S = sum of |terms| of that element's sum in float64;
  * float32 statistics (save_mean / save_rstd / running stats): ``1e-5 |ref| + 1e-6 max|ref|``.
"""
import torch

BF16_REL = 2.0 ** -8          # half a bf16 ulp, relative to the value (the ulp of [2^e, 2^(e+1)) is 2^(e-7))
ABS_SLACK = 1e-6              # float32 arithmetic before the one rounding, relative to the array's scale
SUM_REL = 2e-5                # float32 sum chains of a few hundred terms: n 2^-24 S < 2e-5 S
STAT_REL = 1e-5               # save_mean / save_rstd / running statistics
TIE_REL = 4 * 2.0 ** -24      # two candidates within this of each other (relative) may be ordered either way in float32
AMBIGUOUS_MAX = 1e-3          # kernel decisions taken as given must stay rarer than this


# ---- bars -------------------------------------------------------------------------------------------------------------------
def bf16_bar(ref, extra=0.0):
    ref = ref.double()
    return BF16_REL * ref.abs() + ABS_SLACK * float(ref.abs().max()) + extra


def sum_bar(S):
    return SUM_REL * S.double() + 1e-30


def stat_bar(ref):
    ref = ref.double()
    return STAT_REL * ref.abs() + ABS_SLACK * float(ref.abs().max())


def ratio(got, ref, bar):
    """max |got - ref| / bar over all elements (0 for empty tensors); NaN anywhere gives inf."""
    d = (got.double() - ref.double()).abs()
    if d.numel() == 0:
        return 0.0
    r = d / bar
    if torch.isnan(r).any():
        return float("inf")
    return float(r.max())


def check(got, ref, bar, name):
    r = ratio(got, ref, bar)
    assert r <= 1.0, f"{name}: max |got - ref| / bar = {r:.3g}"
    return r


def has_teeth(defective, ref, bar, name):
    """The bar must reject the reference with a plausible defect applied."""
    r = ratio(defective, ref, bar)
    assert r > 1.0, f"{name}: bar does not catch the defect (ratio {r:.3g})"
    return r


def bf16_round_toward_zero(t):
    """float64 -> bf16 by truncation (the defect 'rounded toward zero instead of to nearest'), returned as float64."""
    f = t.float().contiguous()
    bits = f.view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).double()


# ---- BatchNorm ----------------------------------------------------------------------------------------------------------------
def _c(v):
    return v.view(1, -1, 1, 1)


def bn_stats(x):
    """Two-pass float64 batch statistics of an [N, C, H, W] tensor: (mean, biased var) per channel."""
    xd = x.detach().double()
    mean = xd.mean(dim=(0, 2, 3))
    var = ((xd - _c(mean)) ** 2).mean(dim=(0, 2, 3))
    return mean, var


def bn_coef(gamma, beta, mean, var, eps):
    """Exact per-channel scale / shift of the normalisation: bn(x) = x a + b."""
    rstd = 1.0 / torch.sqrt(var + eps)
    a = gamma.detach().double() * rstd
    return a, beta.detach().double() - mean * a, rstd


def bn_fwd(x, gamma, beta, eps, mean, var, res=None):
    """Pre-activation x a + b (+ residual) in float64."""
    a, b, _ = bn_coef(gamma, beta, mean, var, eps)
    pre = x.double() * _c(a) + _c(b)
    if res is not None:
        pre = pre + res.double()
    return pre


def bn_terms(x, gamma, beta, eps, mean, var, res=None):
    """Sum of |terms| the kernel forms a pre-activation from in float32: |x a| + |b| (+ |residual|)."""
    a, b, _ = bn_coef(gamma, beta, mean, var, eps)
    t = (x.double() * _c(a)).abs() + _c(b).abs()
    return t if res is None else t + res.double().abs()


def relu_ambiguous(pre, mask, terms=None):
    """Elements where the kernel's mask differs from ``pre > 0``: allowed only where pre is within float32 rounding of 0, relative
    to the |terms| it was formed from (``bn_terms``). Returns (fraction of ambiguous elements, all disagreements explained)."""
    disagree = (pre > 0) != mask
    scale = pre.abs() if terms is None else terms + pre.abs()
    near = pre.abs() <= TIE_REL * scale + 1e-30
    return float(disagree.double().mean()), bool((~disagree | near).all())


def running_stats(rm0, rv0, mean, var, m, momentum):
    unbiased = var * m / (m - 1) if m > 1 else var
    return (1 - momentum) * rm0.double() + momentum * mean, (1 - momentum) * rv0.double() + momentum * unbiased


def bn_bwd(g, x, gamma, eps, mean, var):
    """BatchNorm backward on the (already masked) gradient g, float64. Returns dict with dx, dgamma, dbeta, the S of the two sums and
    the bar term ``dx_extra`` that 2e-5 S uncertainty in those sums carries into dx."""
    g, xd, gamma = g.double(), x.detach().double(), gamma.detach()
    m = g.numel() // g.shape[1]
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (xd - _c(mean)) * _c(rstd)
    dbeta = g.sum(dim=(0, 2, 3))
    dgamma = (g * xhat).sum(dim=(0, 2, 3))
    a = gamma.double() * rstd
    dx = _c(a) * (g - _c(dbeta) / m - xhat * _c(dgamma) / m)
    S_dbeta = g.abs().sum(dim=(0, 2, 3))
    # the kernels form dgamma as rstd (sum g x - mean sum g): its float32 terms are g x and mean g
    S_dgamma = rstd * (g.abs() * (xd.abs() + _c(mean.abs()))).sum(dim=(0, 2, 3))
    dx_extra = _c(a.abs() / m) * SUM_REL * (_c(S_dbeta) + xhat.abs() * _c(S_dgamma))
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, S_dgamma=S_dgamma, S_dbeta=S_dbeta, dx_extra=dx_extra, a=a)


def bn_block_rows(m, c, vec, block=0):
    """Row indices of row block ``block`` of the BatchNorm kernels' reduction passes (dir_bn.hip bn_geom: rows r with
    (r // rpi) % rblocks == block) — for the 'one row block dropped' defect. A restatement of bn_geom (dir_bn.hip:43-57): 256 threads
    per workgroup (DIR_TPB), >= 4 row iterations per workgroup, <= 768 / ctiles row blocks (BN_CAP_TOTAL). Keep the two in step: if
    the kernel's geometry changes, this still names a set of rows a dropped-block defect would lose, but no longer a real block."""
    ct = min(c, 32 * vec)
    tpr = ct // vec
    rpi = 256 // tpr
    ctiles = c // ct
    want = max(1, -(-m // (rpi * 4)))
    rblocks = min(want, max(1, 768 // ctiles))
    r = torch.arange(m)
    return r[(r // rpi) % rblocks == block]


# ---- 3x3 / stride-2 / pad-1 max pool -------------------------------------------------------------------------------------------
def _windows(v, fill):
    """[N, C, H, W] -> [N, C, Ho, Wo, 9] candidates in scan order k = 3 r + s (padding = fill)."""
    n, c, h, w = v.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    p = torch.full((n, c, 2 * ho + 1, 2 * wo + 1), fill, dtype=v.dtype, device=v.device)
    p[:, :, 1:h + 1, 1:w + 1] = v
    cand = [p[:, :, r:r + 2 * ho:2, s:s + 2 * wo:2] for r in range(3) for s in range(3)]
    return torch.stack(cand, dim=-1), ho, wo


def pool_route(v, tie_rel=0.0, tie_scale=None):
    """Per window: max value, route (first maximum in scan order), the runner-up's position and a near-tie flag (best two within
    tie_rel (|f1| + tie_scale) of each other). v: float64 [N, C, H, W]."""
    cand, _, _ = _windows(v, float("-inf"))
    best, route = cand.max(dim=-1)                              # torch returns the FIRST maximal index
    k = torch.arange(9, device=v.device)
    first = k.view(1, 1, 1, 1, 9) == route.unsqueeze(-1)
    rest = cand.masked_fill(first, float("-inf"))
    second, second_pos = rest.max(dim=-1)
    scale = best.abs() if tie_scale is None else best.abs() + tie_scale
    near = (second > float("-inf")) & ((best - second) <= tie_rel * scale) & (best != second)
    return best, route, second_pos, near


def pool_scatter(dy, route, valid, h, w):
    """Gradient of the pool: dy of window (ho, wo) added to input position route (where valid). float64 [N, C, H, W]."""
    n, c, ho, wo = dy.shape
    r, s = route // 3, route % 3
    hi = 2 * torch.arange(ho, device=dy.device).view(1, 1, ho, 1) - 1 + r
    wi = 2 * torch.arange(wo, device=dy.device).view(1, 1, 1, wo) - 1 + s
    dx = torch.zeros((n, c, h + 2, w + 2), dtype=torch.float64, device=dy.device)
    flat = dx.view(n, c, -1)
    lin = (hi + 1) * (w + 2) + (wi + 1)
    val = torch.where(valid, dy.double(), torch.zeros((), dtype=torch.float64, device=dy.device))
    flat.scatter_add_(2, lin.reshape(n, c, -1), val.reshape(n, c, -1))
    return dx[:, :, 1:h + 1, 1:w + 1].contiguous()


def maxpool_ref(x):
    """MaxPool2d(3, 2, 1) of bf16 x: values are exact, so the route is the first maximum in scan order (torch's rule)."""
    best, route, second, _ = pool_route(x.double())
    return best, route, second


def stem_tail_ref(x, gamma, beta, eps, mean, var, kernel_idx=None):
    """maxpool(relu(bn(x))) in float64. Route = argmax of x a + b; where the best two are within float32 rounding of each other, or
    the window's maximum is within float32 rounding of 0 (the ReLU clip), the kernel's idx byte (0..8, 9 = clipped) decides.
    Returns y, route (0..8), valid (not clipped), the near-tie mask and the runner-up position."""
    a, b, _ = bn_coef(gamma, beta, mean, var, eps)
    v = x.double() * _c(a) + _c(b)
    tie_scale = _c(b).abs().expand(v.shape[0], -1, (v.shape[2] - 1) // 2 + 1, (v.shape[3] - 1) // 2 + 1)
    best, route, second, near = pool_route(v, TIE_REL, tie_scale)
    clip_near = best.abs() <= TIE_REL * (best.abs() + tie_scale)
    valid = best > 0
    amb = near | clip_near
    if kernel_idx is not None:
        k = kernel_idx.long()
        route = torch.where(amb & (k < 9), k, route).contiguous()
        valid = torch.where(amb, k < 9, valid)
    y = torch.clamp(best, min=0.0)
    return dict(y=y, route=route, valid=valid, ambiguous=amb, second=second)


# ---- 7x7 / stride-2 / pad-3 stem weight gradient ------------------------------------------------------------------------------
def stem_wgrad_ref(dy, x):
    """dW[co, c, r, s] = sum over (n, ho, wo) of dy[n, co, ho, wo] x[n, c, 2 ho - 3 + r, 2 wo - 3 + s] in float64, and S = the same
    sum of |terms|."""
    from torch.nn.grad import conv2d_weight
    dyd, xd = dy.double(), x.double()
    shape = (dy.shape[1], x.shape[1], 7, 7)
    dw = conv2d_weight(xd, shape, dyd, stride=2, padding=3)
    S = conv2d_weight(xd.abs(), shape, dyd.abs(), stride=2, padding=3)
    return dw, S
