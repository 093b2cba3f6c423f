"""Float64 restatement of the NYUD2-DIR evaluator (``dirhip/eval_nyud2.py`` / ``dir_depth_eval_accumulate``) and the bars its tests use.

Per-pixel terms are formed in numpy **float32**, one rounding per operation, exactly as the kernel forms them (the library is built
with ``-ffp-contract=off`` and hipcc's correctly rounded division), so apart from ``log`` they are the kernel's terms bit for bit:

    bucket = min(int(depth * mult), bucket_num - 1)           float32 product, truncated; depth <= 0 -> 0
    d      = |pred - depth|
    terms  = d * d,  d,  d / depth,  |log(pred) / ln10 - log(depth) / ln10|         ln10 = float32(math.log(10))
    r      = pred / depth unless that is < depth / pred (a NaN ratio stays NaN)
    counts = [r <= 1.25], [r <= 1.5625], [r <= 1.953125], 1

and summed per bucket in float64 (``np.add.at`` on float64 copies: sequential, pixel order). Pixels with a NaN depth or a zero
mask byte are in no sum.

Bars
----
* counts (three delta columns, NUM): exact. Every comparison is on float32 values both sides form identically.
* d*d, d, d / depth: the terms are identical float32 numbers; kernel and restatement differ only in the ORDER of a float64 sum.
  Reordering n float64 additions moves the sum by at most (n - 1) * 2^-53 * sum|terms| (Higham, Accuracy and Stability, §4.2);
  the bar ``1e-12 * sum|terms|`` is that bound for n <= 9 000 and far above the typical sqrt(n) * 2^-53 growth for the 2e8 pixels
  of a test set. A float32 running sum misses it by orders of magnitude (2^-24 per addition).
* LG10: the device ``logf`` is documented to within 1 ulp of the true logarithm (HIP math API, single-precision table). The
  restatement takes ``log`` in float64 and rounds to float32: within 0.5 ulp (+ 2^-29 relative from the double rounding). Hence for
  L = log(x):  |L_dev - L_ref| <= 1.5 ulp(L) <= 1.5 * 2^-23 * |L|.  q = L / ln10 is a correctly rounded division on both sides; rounding
  is monotone, so |q_dev - q_ref| <= 1.5 * 2^-23 * |q| * (1 + 2^-23) + ulp(q) <= 2.5 * 2^-23 * |q| (+ second order). The difference
  t = |q_p - q_z| is again rounded once on both sides: |t_dev - t_ref| <= |dq_p| + |dq_z| + ulp(t)
  <= 2^-23 * (2.5 * (|q_p| + |q_z|) + |t|) =: lg10_term_bound.  We multiply by 1.01 for the second-order terms dropped above and add
  the float64 reordering bar. ``lg10_bound`` is the per-bucket sum of these. Near x = 1 (|L| tiny) an ulp of L is tiny too, so the
  bound stays relative to the logarithms, not to x.
* bilinear: ``bilinear_align_corners`` restates the kernel's formula in float32 steps, so upsampled predictions are the kernel's bit
  for bit. Against torch's CPU ``F.interpolate(mode='bilinear', align_corners=True)`` it is NOT bit-equal (torch's vectorised kernel
  orders the four products differently): see tests/test_nyud2_eval_host.py for the measured difference and how the golden
  comparison caps the delta counts with ``delta_flip_cap``.
"""
import math

import numpy as np

f32 = np.float32
LN10 = f32(math.log(10))
THRESHOLDS = (f32(1.25), f32(1.5625), f32(1.953125))
SHOT_IDX = {
    'many': [9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27,
             28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 47, 49],
    'medium': [7, 8, 46, 48, 50, 51, 52, 53, 54, 55, 56, 58, 60, 61, 63],
    'few': [0, 1, 2, 3, 4, 5, 6, 57, 59, 62, 64, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77,
            78, 79, 80, 81, 82, 83, 84, 85, 86, 87, 88, 89, 90, 91, 92, 93, 94, 95, 96, 97, 98, 99]}
COLUMNS = ("MSE", "MAE", "ABS_REL", "LG10", "DELTA1", "DELTA2", "DELTA3", "NUM")


def _axis(n_in, n_out):
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    s = np.arange(n_out, dtype=f32) * scale                           # float32 product
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.where(i0 < n_in - 1, i0 + 1, i0)
    lo = (s - i0.astype(f32)).astype(f32)
    return i0, i1, (f32(1) - lo).astype(f32), lo


def bilinear_align_corners(pred, H, W, align_corners=True):
    """pred [N, h, w] float32 -> [N, H, W] float32: hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11), every step float32.
    ``align_corners=False`` (half-pixel centres) exists only as the emulated defect of the GPU tests."""
    pred = np.asarray(pred, dtype=f32)
    n, h, w = pred.shape
    if align_corners:
        y0, y1, hy, ly = _axis(h, H)
        x0, x1, hx, lx = _axis(w, W)
    else:
        def half(n_in, n_out):
            s = np.maximum((np.arange(n_out, dtype=f32) + f32(0.5)) * f32(n_in / n_out) - f32(0.5), f32(0)).astype(f32)
            i0 = np.minimum(s.astype(np.int64), n_in - 1)
            lo = (s - i0.astype(f32)).astype(f32)
            return i0, np.where(i0 < n_in - 1, i0 + 1, i0), (f32(1) - lo).astype(f32), lo
        y0, y1, hy, ly = half(h, H)
        x0, x1, hx, lx = half(w, W)
    hy, ly = hy[None, :, None], ly[None, :, None]
    hx, lx = hx[None, None, :], lx[None, None, :]
    v00, v01 = pred[:, y0][:, :, x0], pred[:, y0][:, :, x1]
    v10, v11 = pred[:, y1][:, :, x0], pred[:, y1][:, :, x1]
    with np.errstate(all="ignore"):
        top = (hx * v00).astype(f32) + (lx * v01).astype(f32)
        bot = (hx * v10).astype(f32) + (lx * v11).astype(f32)
        return ((hy * top).astype(f32) + (ly * bot).astype(f32)).astype(f32)


def bucket_of(depth, mult=10.0, bucket_num=100):
    with np.errstate(all="ignore"):
        v = (np.asarray(depth, dtype=f32) * f32(mult)).astype(f32)
        v = np.where(np.isnan(v), f32(0), v)
        k = np.where(v >= f32(2147483520.0), np.int64(2147483647), np.where(v <= 0, 0, np.minimum(v, f32(2147483520.0)).astype(np.int64)))
    return np.minimum(k, bucket_num - 1)


def log32(x):
    """log of float32 x, correctly rounded to float32 up to double rounding (float64 log, then one rounding)."""
    with np.errstate(all="ignore"):
        return np.log(np.asarray(x, dtype=f32).astype(np.float64)).astype(f32)


def max_ratio(pred, depth):
    with np.errstate(all="ignore"):
        yz, zy = (pred / depth).astype(f32), (depth / pred).astype(f32)
    return np.where(yz < zy, zy, yz)                                   # maxOfTwo: keep yz unless it is < zy


def pixel_terms(pred, depth):
    """float32 [n] each -> terms float32 [n, 4], counts bool [n, 3], lg10_term_bound float64 [n]."""
    pred, depth = np.asarray(pred, dtype=f32), np.asarray(depth, dtype=f32)
    with np.errstate(all="ignore"):
        d = np.abs((pred - depth).astype(f32))
        qp, qz = (log32(pred) / LN10).astype(f32), (log32(depth) / LN10).astype(f32)
        lg = np.abs((qp - qz).astype(f32))
        terms = np.stack([(d * d).astype(f32), d, (d / depth).astype(f32), lg], axis=1)
        r = max_ratio(pred, depth)
        counts = np.stack([r <= t for t in THRESHOLDS], axis=1)
        bound = 2.0 ** -23 * (2.5 * (np.abs(qp.astype(np.float64)) + np.abs(qz.astype(np.float64))) + lg.astype(np.float64))
    return terms, counts, bound


def table(pred, depth, mask=None, mult=10.0, bucket_num=100, acc_dtype=np.float64, bucket_from=None):
    """Flat float32 pred / depth of equal size (already upsampled) -> dict with
    ``table`` [bucket_num, 8] float64, ``abs`` [bucket_num, 4] (sum of |terms|, for the reordering bar), ``lg10_bound`` [bucket_num].
    ``acc_dtype=np.float32`` and ``bucket_from`` (bucket computed from another array) exist only to emulate defects."""
    pred, depth = np.asarray(pred, dtype=f32).reshape(-1), np.asarray(depth, dtype=f32).reshape(-1)
    keep = ~np.isnan(depth)
    if mask is not None:
        keep &= np.asarray(mask).reshape(-1) != 0
    p, z = pred[keep], depth[keep]
    b = bucket_of(z if bucket_from is None else np.asarray(bucket_from, dtype=f32).reshape(-1)[keep], mult, bucket_num)
    terms, counts, bound = pixel_terms(p, z)
    out = np.zeros((bucket_num, 8), dtype=acc_dtype)
    with np.errstate(all="ignore"):
        for k in range(4):
            np.add.at(out[:, k], b, terms[:, k].astype(acc_dtype))
        for k in range(3):
            np.add.at(out[:, 4 + k], b, counts[:, k].astype(acc_dtype))
        np.add.at(out[:, 7], b, np.ones(b.shape, dtype=acc_dtype))
        tabs = np.zeros((bucket_num, 4))
        for k in range(4):
            np.add.at(tabs[:, k], b, np.abs(terms[:, k].astype(np.float64)))
        lgb = np.zeros(bucket_num)
        np.add.at(lgb, b, bound)
    return {"table": out.astype(np.float64), "abs": tabs, "lg10_bound": 1.01 * lgb + 1e-12 * tabs[:, 3]}


def metrics(row):
    """one summed row (8 numbers) -> the reference's dict (nyud2-dir/util.py:89-133)."""
    e = {'MSE': 0, 'RMSE': 0, 'ABS_REL': 0, 'LG10': 0, 'MAE': 0, 'DELTA1': 0, 'DELTA2': 0, 'DELTA3': 0, 'NUM': 0}
    if row[7] > 0:
        for k, name in enumerate(COLUMNS[:7]):
            e[name] = float(row[k] / row[7])
        e['NUM'] = int(row[7])
    e['RMSE'] = float(np.sqrt(e['MSE']))
    return e


def shot_dict(tab):
    tab = np.asarray(tab, dtype=np.float64)
    out = {'overall': metrics(tab.sum(axis=0))}
    for shot, idx in SHOT_IDX.items():
        out[shot] = metrics(tab[[i for i in idx if i < tab.shape[0]]].sum(axis=0))
    return out


def delta_flip_cap(pred, depth, rel):
    """Number of pixels whose max-ratio lies within a relative ``rel`` of one of the three thresholds: an upper bound on how many
    delta decisions can differ between two predictions that agree to within ``rel / 2`` relatively (the ratio pred / depth, or its
    inverse, moves by the same relative amount plus one rounding, 2^-24, which ``rel`` must include)."""
    r = max_ratio(np.asarray(pred, dtype=f32).reshape(-1), np.asarray(depth, dtype=f32).reshape(-1)).astype(np.float64)
    near = np.zeros(r.shape, dtype=bool)
    for t in THRESHOLDS:
        near |= np.abs(r - float(t)) <= rel * float(t)
    return int(near.sum())
