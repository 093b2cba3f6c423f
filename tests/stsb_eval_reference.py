"""numpy / Python-int restatement of the balanced STS-B evaluator (``dirhip/eval_stsb.py`` / ``dir_stsb_eval``), of the LDS weights
over histogram buckets (``dir_lds_weights_binned``) and the bars their tests use.

Binning (sts-b-dir/util.py:115-120): float32 edges of ``np.histogram(np.array([], float32), 50, range=(0., 5.))``, bin = (number of
edges <= label) - 1 (``np.searchsorted(..., side='right') - 1``), ``label == 5`` in the last bin; group 0 many / 1 medium / 2 few by
the reference's ``_shot_idx`` lists.

Moment table [4, 10] float64 (rows many / medium / few / overall): per sample, float64, one rounding per operation — the kernel's terms
bit for bit apart from ``log``:
    p = 5.0 * float64(pred)   (exact: 24 + 3 bits),  l = float64(label),  d = |p - l|,  p' = p - 2.5,  l' = l - 2.5
    NUM, [d == 0], d * d, d, ln d (d > 0), p', l', p' * p', l' * l', p' * l'
summed per group with ``np.sum`` (pairwise), the overall row (many + medium) + few as the kernel forms it.

Rank table [4, 5] Python integers: a = 2 * #less + #equal + 1 (twice scipy's average rank) for pred, b for label, within the group
(rows 0-2) and over the whole set (row 3): sum a, sum b, sum a^2, sum b^2, sum ab. Counted on the raw float32 values.

Bars
----
* counts and the rank table: exact.
* a float64 column: kernel and restatement add identical terms in different orders; reordering n additions moves a sum by at most
  (n - 1) * 2^-53 * sum|terms| (Higham, Accuracy and Stability, §4.2): ``bound = n * 2^-53 * sum|terms|`` per row and column, n the
  row's sample count. The overall row is two more additions, of the three group sums: n + 2 there.
* ln d: both sides take the logarithm of the SAME float64 d. The device's double-precision ``log`` is documented to within 1 ulp, numpy's
  to within 0.5 ulp: one term differs by at most 1.5 * 2^-53 * |ln d| (the allowance of tests/age_eval_reference.py), a row by
  1.5 * 2^-53 * sum|ln d| on top of the reordering bound.
"""
import math

import numpy as np

f32 = np.float32
NUM_BINS = 50
ROWS = ("many", "medium", "few", "overall")
MOMENT_COLUMNS = ("NUM", "ZERO", "SE", "AE", "LN", "SP", "SL", "SPP", "SLL", "SPL")
KEYS = ("mse", "l1", "gmean", "pearsonr", "spearmanr", "num_samples")
ALL_METRICS = ["mse", "l1", "gmean", "pearsonr", "spearmanr"]
SHOT_IDX = {
    'many': [0, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 49],
    'medium': [2, 4, 6, 8, 27, 35, 37],
    'few': [1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 29, 31, 33, 39, 41, 43, 45, 47],
}


def edges(num_bins=NUM_BINS):
    return np.asarray(np.histogram(a=np.array([], dtype=f32), bins=num_bins, range=(0., 5.))[1], dtype=f32)


def bin_of(labels, e=None):
    e = edges() if e is None else np.asarray(e, dtype=f32)
    lab = np.asarray(labels, dtype=f32).reshape(-1)
    if not ((lab >= e[0]) & (lab <= e[-1])).all():
        raise ValueError("label outside the edges")
    return np.minimum(np.searchsorted(e, lab, side='right') - 1, len(e) - 2)


def group_of_bin():
    g = np.full(NUM_BINS, 2, dtype=np.uint8)
    g[SHOT_IDX['many']] = 0
    g[SHOT_IDX['medium']] = 1
    return g


def groups(labels):
    return group_of_bin()[bin_of(labels)]


def terms(pred, label):
    """[n, 8] float64 summed terms and the zero flags, formed as the kernel forms them."""
    p = 5.0 * np.asarray(pred, dtype=f32).reshape(-1).astype(np.float64)
    l = np.asarray(label, dtype=f32).reshape(-1).astype(np.float64)
    d = np.abs(p - l)
    ps, ls = p - 2.5, l - 2.5
    pos = d > 0
    ln = np.where(pos, np.log(np.where(pos, d, 1.0)), 0.0)
    return np.stack([d * d, d, ln, ps, ls, ps * ps, ls * ls, ps * ls], axis=1), d == 0


def moment_table(pred, label, grp=None):
    """-> dict: ``table`` [4, 10] float64, ``bound`` [4, 10] (0 for the two count columns)."""
    t, zero = terms(pred, label)
    g = groups(label) if grp is None else np.asarray(grp)
    tab, bound = np.zeros((4, 10)), np.zeros((4, 10))
    for r in range(3):
        m = g == r
        n = int(m.sum())
        tab[r, 0], tab[r, 1] = n, int(zero[m].sum())
        tab[r, 2:] = t[m].sum(axis=0)
        mag = np.abs(t[m]).sum(axis=0)
        bound[r, 2:] = n * 2.0 ** -53 * mag
        bound[r, 4] += 1.5 * 2.0 ** -53 * mag[2]
    tab[3] = (tab[0] + tab[1]) + tab[2]
    mag = np.abs(t).sum(axis=0)
    bound[3, 2:] = (len(g) + 2) * 2.0 ** -53 * mag
    bound[3, 4] += 1.5 * 2.0 ** -53 * mag[2]
    return {"table": tab, "bound": bound}


def doubled_ranks(x):
    """2 * less + equal + 1 per element (twice ``scipy.stats.rankdata(x)``), as Python-int-safe int64."""
    x = np.asarray(x, dtype=f32).reshape(-1)
    s = np.sort(x)
    less = np.searchsorted(s, x, side='left')
    le = np.searchsorted(s, x, side='right')
    return (2 * less + (le - less) + 1).astype(np.int64)


def rank_row(pred, label):
    a, b = (doubled_ranks(v).astype(object) for v in (pred, label))           # object dtype: Python integers, no overflow
    return [int(a.sum()) if len(a) else 0, int(b.sum()) if len(b) else 0, int((a * a).sum()) if len(a) else 0,
            int((b * b).sum()) if len(a) else 0, int((a * b).sum()) if len(a) else 0]


def rank_table(pred, label, grp=None):
    pred, label = np.asarray(pred, dtype=f32).reshape(-1), np.asarray(label, dtype=f32).reshape(-1)
    g = groups(label) if grp is None else np.asarray(grp)
    return [rank_row(pred[g == r], label[g == r]) for r in range(3)] + [rank_row(pred, label)]


def metrics(moments, ranks, metric=ALL_METRICS):
    """The host half, restated on its own: the reference's dict (util.py:142-163)."""
    out = {}
    for r, shot in enumerate(ROWS):
        num, zero, se, ae, ln, sp, sl, spp, sll, spl = (float(v) for v in moments[r])
        n = int(num)
        sa, sb, saa, sbb, sab = (int(v) for v in ranks[r])
        va, vb = n * saa - sa * sa, n * sbb - sb * sb
        m = {}
        if 'mse' in metric:
            m['mse'] = se / num if n else 0.
        if 'l1' in metric:
            m['l1'] = ae / num if n else 0.
        if 'gmean' in metric:
            m['gmean'] = math.exp((ln + zero * math.log(1e-10)) / num) if n else 0.
        if 'pearsonr' in metric:
            if n <= 1:
                m['pearsonr'] = 0.
            elif va == 0 or vb == 0:
                m['pearsonr'] = float('nan')
            else:
                m['pearsonr'] = (num * spl - sp * sl) / math.sqrt((num * spp - sp * sp) * (num * sll - sl * sl))
        if 'spearmanr' in metric:
            if n <= 1:
                m['spearmanr'] = 0.
            elif va == 0 or vb == 0:
                m['spearmanr'] = float('nan')
            else:
                m['spearmanr'] = (n * sab - sa * sb) / math.sqrt(va * vb)
        m['num_samples'] = n
        out[shot] = m
    return out


def evaluate(pred, label, metric=ALL_METRICS):
    return metrics(moment_table(pred, label)["table"], rank_table(pred, label), metric)


def as_rows(d):
    """dict -> float64 [4, 6], rows ROWS, columns KEYS: the layout of tests/golden/stsb_eval_ref.npz."""
    return np.array([[float(d[s][k]) for k in KEYS] for s in ROWS], dtype=np.float64)


# ---- LDS weights over histogram buckets (sts-b-dir/tasks.py:44-73), the reference's own numpy / scipy calls ----------------------
def lds_weights(labels, reweight, lds=False, window=None, bins=NUM_BINS):
    from scipy.ndimage import convolve1d
    targs = list(np.asarray(labels, dtype=f32))
    value_lst, bins_edges = np.histogram(targs, bins=bins, range=(0., 5.))
    idx = np.minimum(np.searchsorted(bins_edges, np.asarray(targs, dtype=f32), side='right') - 1, bins - 1)
    if reweight == 'sqrt_inv':
        value_lst = [np.sqrt(x) for x in value_lst]
    num_per_label = [value_lst[i] for i in idx]
    if lds:
        smoothed_value = convolve1d(value_lst, weights=window, mode='constant')
        num_per_label = [smoothed_value[i] for i in idx]
    with np.errstate(divide='ignore'):
        weights = [f32(1 / x) for x in num_per_label]
    scaling = len(weights) / np.sum(weights)
    return np.array([scaling * x for x in weights], dtype=f32)
