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

Convolutions (``conv_fwd_ref`` / ``conv_dgrad_ref`` / ``conv_wgrad_ref``: explicit per-tap GEMMs, each returning the result and S, the
same operation on |operands|):
  * bf16 output of one float32 sum (forward, plain data gradient): ``bf16_bar(ref, SUM_REL S)``. The MFMA kernels add exact products
    into a float32 accumulator 16 at a time, so the longest chain of the network (K = 9 * 512 = 4608) has 288 roundings:
    288 * 2^-24 S < 2e-5 S even in the worst case.
  * bf16 output after fused roundings (``join_ref``): the kernel stores bf16(bf16(conv) + addend) and adds the compact stride-2 addend
    with one more rounding. ref is the exact total; every intermediate rounding adds half an ulp of the intermediate,
    ``2^-8 (|intermediate| + e)`` with e the error the intermediate already carries. The error e of the value before the final rounding
    also moves that rounding's half ulp: all extra terms are scaled by (1 + 2^-8). Where the ReLU mask is 0 the output is exactly 0.
  * float32 weight gradient: BOTH ``SUM_REL S`` (holds for any float32 order of an honest sum) and ``WGRAD_REL max|ref|`` per
    element. S grows like sqrt(M) faster than |dW|: at M = 256 * 56^2 the median S / |ref| is ~825, so 2e-5 S alone allows ~1.6 % of
    |ref| — a dropped 64-pixel K-step would pass. An honest split-K order reaches ~0.06 of the second bar there
    (tests/test_bf16_reference_host.py emulates it).
  * forward statistics (the epilogue's per-tile column sums of the stored y): ``stats_bar`` = 1e-5 |ref| + 1e-5 max|ref| against
    float64 sums of the kernel's own y (test_hip_conv.py's tolerance).
"""
import torch

BF16_REL = 2.0 ** -8          # half a bf16 ulp, relative to the value (the ulp of [2^e, 2^(e+1)) is 2^(e-7))
ABS_SLACK = 1e-6              # float32 arithmetic before the one rounding, relative to the array's scale
SUM_REL = 2e-5                # float32 sum chains of a few hundred terms: n 2^-24 S < 2e-5 S
STAT_REL = 1e-5               # save_mean / save_rstd / running statistics
TIE_REL = 4 * 2.0 ** -24      # two candidates within this of each other (relative) may be ordered either way in float32
AMBIGUOUS_MAX = 1e-3          # kernel decisions taken as given must stay rarer than this
WGRAD_REL = 1e-5              # float32 weight gradients: second bar, relative to the array's scale (test_hip_conv_wgrad3.py's)
CONV_STATS_REL = 1e-5         # forward statistics column sums: relative to the element and to the array's scale


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


# ---- convolutions (explicit per-tap GEMMs, NCHW in and out, float64; CPU or GPU) -------------------------------------------------
def _out_hw(h, w, r, s, stride, pad):
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1


def _tap(t, i, j, stride, ho, wo):
    """Rows of padded t [N, C, Hp, Wp] that tap (i, j) reads for the output grid ho x wo: [N, C, ho, wo] view."""
    return t[:, :, i:i + stride * (ho - 1) + 1:stride, j:j + stride * (wo - 1) + 1:stride]


def _gemm(a, b):
    """[N, C, H, W] x [C, D] -> [N, D, H, W] (channels-last GEMM)."""
    return (a.permute(0, 2, 3, 1) @ b).permute(0, 3, 1, 2)


def conv_fwd_ref(x, w, stride, pad):
    """y[n, co, ho, wo] = sum over (ci, i, j) of x[n, ci, stride ho - pad + i, stride wo - pad + j] w[co, ci, i, j] (zero outside the map).
    Returns (y, S) in float64, S = the same sum of |terms|."""
    xd, wd = x.double(), w.double()
    n, _, h, wdt = xd.shape
    cout, _, r, s = wd.shape
    ho, wo = _out_hw(h, wdt, r, s, stride, pad)
    xp = torch.nn.functional.pad(xd, (pad, pad, pad, pad))
    xa = xp.abs()
    y = torch.zeros((n, cout, ho, wo), dtype=torch.float64, device=xd.device)
    S = torch.zeros_like(y)
    for i in range(r):
        for j in range(s):
            wt = wd[:, :, i, j].t()
            y += _gemm(_tap(xp, i, j, stride, ho, wo), wt)
            S += _gemm(_tap(xa, i, j, stride, ho, wo), wt.abs())
    return y, S


def conv_dgrad_ref(dy, w, x_shape, stride, pad):
    """Gradient of conv(x, w, stride, pad) with respect to x for output gradient dy, from the ORIGINAL weight w [Cout, Cin, R, S]:
    dx[n, ci, h, w] = sum over (co, i, j) with h = stride ho - pad + i, w = stride wo - pad + j of dy[n, co, ho, wo] w[co, ci, i, j].
    Returns (dx, S) in float64."""
    dyd, wd = dy.double(), w.double()
    n, cin, h, wdt = x_shape
    cout, _, r, s = wd.shape
    ho, wo = dyd.shape[2], dyd.shape[3]
    dxp = torch.zeros((n, cin, h + 2 * pad, wdt + 2 * pad), dtype=torch.float64, device=dyd.device)
    Sp = torch.zeros_like(dxp)
    da = dyd.abs()
    for i in range(r):
        for j in range(s):
            wt = wd[:, :, i, j]
            _tap(dxp, i, j, stride, ho, wo).add_(_gemm(dyd, wt))
            _tap(Sp, i, j, stride, ho, wo).add_(_gemm(da, wt.abs()))
    return dxp[:, :, pad:pad + h, pad:pad + wdt], Sp[:, :, pad:pad + h, pad:pad + wdt]


def conv_wgrad_ref(dy, x, k, stride, pad):
    """dW[co, ci, i, j] = sum over (n, ho, wo) of dy[n, co, ho, wo] x[n, ci, stride ho - pad + i, stride wo - pad + j] (k x k kernel).
    Returns (dW, S) in float64."""
    dyd, xd = dy.double(), x.double()
    ho, wo = dyd.shape[2], dyd.shape[3]
    cout, cin = dyd.shape[1], xd.shape[1]
    xp = torch.nn.functional.pad(xd, (pad, pad, pad, pad))
    g = dyd.permute(0, 2, 3, 1).reshape(-1, cout)
    ga = g.abs()
    dw = torch.zeros((cout, cin, k, k), dtype=torch.float64, device=dyd.device)
    S = torch.zeros_like(dw)
    for i in range(k):
        for j in range(k):
            xt = _tap(xp, i, j, stride, ho, wo).permute(0, 2, 3, 1).reshape(-1, cin)
            dw[:, :, i, j] = g.t() @ xt
            S[:, :, i, j] = ga.t() @ xt.abs()
    return dw, S


def up2(a, ho, wo):
    """Compact stride-2 gradient [N, C, ho/2, wo/2] placed at the even pixels of an [N, C, ho, wo] map (zeros elsewhere)."""
    out = torch.zeros((a.shape[0], a.shape[1], ho, wo), dtype=torch.float64, device=a.device)
    out[:, :, 0::2, 0::2] = a.double()
    return out


def join_ref(conv, S, addend=None, addend_s2=None, mask=None):
    """Fused data gradient relu'(mask) * (conv + addend + up2(addend_s2)) from the exact conv (and its S). The kernel rounds
    bf16(conv), then bf16(. + addend), then (even pixels) bf16(. + compact): each rounding that is not the last is an intermediate.
    Returns (ref, bar): bar = bf16_bar(ref, (1 + 2^-8) (SUM_REL S + sum of 2^-8 (|intermediate| + e))); mask 0 -> ref 0 (the test
    asserts exact zeros there separately)."""
    c = conv.double()
    e = SUM_REL * S.double()
    ho, wo = c.shape[2], c.shape[3]
    total, extra = c, e
    if addend is not None:
        extra = extra + BF16_REL * (total.abs() + extra)                 # bf16(conv) before the add
        total = total + addend.double()
    if addend_s2 is not None:
        even = torch.zeros_like(c, dtype=torch.bool)
        even[:, :, 0::2, 0::2] = True
        extra = torch.where(even, extra + BF16_REL * (total.abs() + extra), extra)   # the value before the compact add, rounded
        total = total + up2(addend_s2, ho, wo)
    if mask is not None:
        keep = mask.bool()
        total = torch.where(keep, total, torch.zeros((), dtype=torch.float64, device=c.device))
        extra = torch.where(keep, extra, torch.zeros((), dtype=torch.float64, device=c.device))
    return total, bf16_bar(total, (1.0 + BF16_REL) * extra)


def bits_to_mask(bits, shape):
    """Bit-per-element ReLU mask ([N*H*W*C / 8] bytes, NHWC element order, element e at bit e % 8 of byte e // 8) -> bool [N, C, H, W]."""
    n, c, h, w = shape
    b = bits.reshape(-1).long()
    flat = ((b.unsqueeze(1) >> torch.arange(8, device=b.device)) & 1).reshape(-1).bool()
    return flat.view(n, h, w, c).permute(0, 3, 1, 2)


def mask_to_bits(mask, reverse=False):
    """bool [N, C, H, W] -> uint8 bytes in the layout of bits_to_mask (reverse: the defect 'bit order reversed within a byte')."""
    flat = mask.permute(0, 2, 3, 1).reshape(-1, 8).long()
    sh = torch.arange(8, device=mask.device)
    if reverse:
        sh = 7 - sh
    return (flat << sh).sum(1).to(torch.uint8)


def wgrad_bar(ref, S):
    """Both weight-gradient bars at once: min(SUM_REL S, WGRAD_REL max|ref|) per element."""
    return torch.minimum(sum_bar(S), torch.full_like(S.double(), WGRAD_REL * float(ref.double().abs().max()) + 1e-30))


def stats_bar(ref):
    ref = ref.double()
    return CONV_STATS_REL * ref.abs() + CONV_STATS_REL * float(ref.abs().max()) + 1e-30
