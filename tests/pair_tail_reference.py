"""numpy restatement of the fused STS-B-DIR pair head (a helper module, imported by tests/test_pair_tail_host.py and
tests/test_hip_pair_tail.py), written from the rules of include/dir_hip.h (dir_pair_tail_fwd / dir_pair_tail_bwd), in two precisions:

  dtype=np.float32  every operation in float32, one rounding each, in the order the header fixes: the BIT-EXACT yardstick for emb, uv,
                    arg1, arg2, ds1, ds2 (numpy rounds every float32 ufunc result once and never fuses a multiply with an add);
  dtype=np.float64  the same chain in float64 (the inputs widened, the float32 keep factor widened): the yardstick for the sums
                    (logits, dweight, dbias) and for autograd compositions.

Dropout enters as keep masks [B, T, D] (bool) and the float32 keep factor, so the module knows nothing about Philox: on the GPU the
masks come from dirhip.tail.dropout_mask(seed, offset, p, B * T, D) (element index row * D + d with row = b * T + t), on the host
from any generator.
"""
import numpy as np


def keep_factor(p):
    """(float)(1 / (1 - p)), 0 at p == 1: the scale of the kept values."""
    return np.float32(0.0) if p == 1.0 else np.float32(1.0 / (1.0 - p))


def dropped(x, keep, factor, dtype):
    x = np.asarray(x).astype(dtype)
    if keep is None:
        return x
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(keep, x * dtype(factor), dtype(0.0)).astype(dtype)


def max_over_time(x, mask):
    """x [B, T, D], mask [B, T] -> (max [B, D], arg [B, D] int32): over the unmasked t, the lowest t that attains the maximum; a NaN
    wins over every number and the lowest NaN stays (torch.max); no unmasked t: -inf and -1."""
    b, t, d = x.shape
    m = np.full((b, d), -np.inf, dtype=x.dtype)
    arg = np.full((b, d), -1, dtype=np.int32)
    mask = np.asarray(mask).astype(bool)
    for i in range(t):
        xt = x[:, i, :]
        with np.errstate(invalid="ignore"):
            take = mask[:, i][:, None] & ((arg < 0) | (xt > m) | (np.isnan(xt) & ~np.isnan(m)))
        m = np.where(take, xt, m)
        arg = np.where(take, np.int32(i), arg)
    return m, arg


def calibrate(f, bins, m1, scale, m2):
    """dir_fds_calibrate_fwd on f [B, K]: row bins[b] of the tables, bins < 0 = row untouched, scale < 0 = column untouched."""
    out = f.copy()
    if bins is None:
        return out
    dt = f.dtype.type
    for b, r in enumerate(np.asarray(bins)):
        if r < 0:
            continue
        s = scale[r].astype(dt)
        with np.errstate(invalid="ignore", over="ignore"):
            out[b] = np.where(s < 0, f[b], (f[b] - m1[r].astype(dt)) * s + m2[r].astype(dt))
    return out


def forward(s1, s2, mask1, mask2, weight, bias, keep1=None, keep2=None, factor=1.0, bins=None, m1=None, scale=None, m2=None,
            dtype=np.float32):
    """-> dict: u, v [B, D]; arg1, arg2 [B, D] int32; f [B, 4D] (uncalibrated); emb [B, 4D] (calibrated); logits [B] (a plain sum in
    `dtype`: a yardstick in float64 only)."""
    x1, x2 = dropped(s1, keep1, factor, dtype), dropped(s2, keep2, factor, dtype)
    u, arg1 = max_over_time(x1, mask1)
    v, arg2 = max_over_time(x2, mask2)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.concatenate([u, v, np.abs(u - v), u * v], axis=1).astype(dtype)
    emb = calibrate(f, bins, m1, scale, m2)
    with np.errstate(invalid="ignore", over="ignore"):
        logits = (emb * np.asarray(weight).reshape(1, -1).astype(dtype)).sum(axis=1) + dtype(np.asarray(bias).reshape(-1)[0])
    return dict(u=u, v=v, arg1=arg1, arg2=arg2, f=f, emb=emb, logits=logits)


def _scatter(g, arg, keep, factor, t, dtype):
    """ds [B, T, D]: (t == arg) ? (keep ? g * factor : 0) : 0."""
    b, d = g.shape
    ds = np.zeros((b, t, d), dtype=dtype)
    bi, di = np.nonzero(arg >= 0)
    ti = arg[bi, di]
    val = g[bi, di]
    if keep is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            val = np.where(keep[bi, ti, di], val * dtype(factor), dtype(0.0)).astype(dtype)
    ds[bi, ti, di] = val
    return ds


def backward(fw, dlogits, weight, t1, t2, demb=None, keep1=None, keep2=None, factor=1.0, bins=None, scale=None, dtype=np.float32):
    """`fw` = forward(..., dtype=dtype). -> dict: du, dv [B, D]; ds1 [B, T1, D], ds2 [B, T2, D]; dweight [4D], dbias (plain sums in
    `dtype`: yardsticks in float64 only)."""
    u, v, emb = fw["u"], fw["v"], fw["emb"]
    d = u.shape[1]
    dl = np.asarray(dlogits).reshape(-1).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        g = dl[:, None] * np.asarray(weight).reshape(1, -1).astype(dtype)
        if demb is not None:
            g = g + np.asarray(demb).astype(dtype)
        if bins is not None:
            for b, r in enumerate(np.asarray(bins)):
                if r >= 0:
                    s = scale[r].astype(dtype)
                    g[b] = np.where(s < 0, g[b], g[b] * s)
        g_u, g_v, g_a, g_m = g[:, :d], g[:, d:2 * d], g[:, 2 * d:3 * d], g[:, 3 * d:]
        sg = (u > v).astype(dtype) - (u < v).astype(dtype)                     # sign(u - v), sign(0) = 0
        du = (g_u + sg * g_a) + g_m * v
        dv = (g_v - sg * g_a) + g_m * u
        dweight = (dl[:, None] * emb).sum(axis=0)
    return dict(du=du, dv=dv, ds1=_scatter(du, fw["arg1"], keep1, factor, t1, dtype), ds2=_scatter(dv, fw["arg2"], keep2, factor, t2, dtype),
                dweight=dweight, dbias=dl.sum())


def torch_chain64(s1, s2, mask1, mask2, weight, bias, keep1=None, keep2=None, factor=1.0, bins=None, m1=None, scale=None, m2=None):
    """The head as a plain torch float64 autograd composition on the CPU (where / masked_fill(-inf) / max(dim=1) / cat / calibration /
    linear), mask and dropout given as arrays. -> (logits [B], emb [B, 4D], leaves dict s1, s2, weight, bias with requires_grad)."""
    import torch
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    leaves = dict(s1=t64(s1).requires_grad_(True), s2=t64(s2).requires_grad_(True),
                  weight=t64(weight).reshape(-1).requires_grad_(True), bias=t64(bias).reshape(-1).requires_grad_(True))

    def pooled(x, keep, mask):
        if keep is not None:
            x = torch.where(torch.tensor(np.asarray(keep, dtype=bool)), x * float(factor), torch.zeros_like(x))
        pad = ~torch.tensor(np.asarray(mask).astype(bool))
        return x.masked_fill(pad[:, :, None], -float("inf")).max(dim=1).values

    u, v = pooled(leaves["s1"], keep1, mask1), pooled(leaves["s2"], keep2, mask2)
    emb = torch.cat([u, v, torch.abs(u - v), u * v], dim=1)
    if bins is not None:
        rows = torch.tensor(np.asarray(bins, dtype=np.int64))
        r = rows.clamp(min=0)
        s = t64(scale)[r]
        live = (rows >= 0)[:, None] & (s >= 0)
        emb = torch.where(live, (emb - t64(m1)[r]) * s + t64(m2)[r], emb)
    logits = emb @ leaves["weight"] + leaves["bias"]
    return logits, emb, leaves


def loss64(kind, logits, targets, weights=None, beta=0.5):
    """Weighted 'mse' / 'huber' mean over the batch in torch float64 (sts-b-dir/loss.py:5-28), written from the formulas."""
    import torch
    d = logits - targets
    if kind == "mse":
        term = d * d
    else:
        a = d.abs()
        term = torch.where(a < beta, a * a * (0.5 / beta), a - 0.5 * beta)
    if weights is not None:
        term = term * weights
    return term.mean()
