"""Float64 restatement of the balanced age evaluator (``dirhip/eval_age.py`` / ``dir_age_eval_accumulate``) and the bars its tests use.

Per-sample terms are formed in numpy **float32**, one rounding per operation, exactly as the kernel forms them (the library is built
with ``-ffp-contract=off``) and as the reference does (``err = np.abs(preds - labels)`` on float32 arrays, train.py:286-391), so
apart from ``log`` they are the kernel's terms bit for bit:

    row    = int(label) if label is integral and 0 <= label < num_labels, else num_labels   (fractional, negative, NaN, too large)
    e      = |pred - label|
    terms  = e * e,  e                      float32
    ln     = log(float64(e)) if e > 0       float64
    counts = [e == 0], 1

and summed per row in float64 (``np.add.at`` on float64 copies: sequential, sample order). Samples with a zero ``valid`` byte are in
no sum.

Bars
----
* counts (zero-error column, NUM): exact. Every comparison is on float32 values both sides form identically.
* e * e, e: the terms are identical float32 numbers; kernel and restatement differ only in the ORDER of a float64 sum. Reordering n
  float64 additions moves the sum by at most (n - 1) * 2^-53 * sum|terms| (Higham, Accuracy and Stability, §4.2); the bar
  ``1e-12 * sum|terms|`` is that bound for n <= 9 000 per row and far above the typical sqrt(n) * 2^-53 growth of larger rows. A
  float32 running sum misses it by orders of magnitude (2^-24 per addition).
* ln: ``e`` is a float32 and so exactly representable in float64: both sides take the logarithm of the SAME number. The device's
  double-precision ``log`` is documented to within 1 ulp of the true value (HIP math API), numpy's to within 0.5 ulp, so one term
  differs by at most 1.5 units of 2^-53 * |ln e| (the figure the evaluator's specification uses; counting an ulp at its widest,
  2^-52 * |ln e|, would double it) and a row by 1.5 * 2^-53 * sum|ln e|. The terms have both signs, so reordering is bounded against
  sum|ln e| as well: ``ln_bound = (1.5 * 2^-53 + 1e-12) * sum|ln e|`` per row. The reordering share is four orders of magnitude the
  larger: the constant in front of 2^-53 does not decide any comparison.
"""
import numpy as np

f32 = np.float32
COLUMNS = ("SE", "AE", "LN", "ZERO", "NUM")
SHOTS = ("many", "median", "low")


def row_of(labels, num_labels):
    lab = np.asarray(labels, dtype=f32).reshape(-1)
    with np.errstate(all="ignore"):
        ok = (lab >= 0) & (lab < f32(num_labels)) & (lab == np.trunc(lab))
    return np.where(ok, np.where(ok, lab, 0).astype(np.int64), num_labels)


def table(pred, label, num_labels, valid=None, acc_dtype=np.float64):
    """Flat float32 pred / label of equal size -> dict with ``table`` [num_labels + 1, 5] float64, ``abs`` [num_labels + 1, 3] (the
    row's sum of |terms| of the three summed columns, for the reordering bar) and ``ln_bound`` [num_labels + 1].
    ``acc_dtype=np.float32`` exists only to emulate the float32-accumulation defect."""
    pred, label = np.asarray(pred, dtype=f32).reshape(-1), np.asarray(label, dtype=f32).reshape(-1)
    assert pred.shape == label.shape
    if valid is not None:
        keep = np.asarray(valid).reshape(-1) != 0
        pred, label = pred[keep], label[keep]
    r = row_of(label, num_labels)
    with np.errstate(all="ignore"):
        e = np.abs((pred - label).astype(f32))
        se = (e * e).astype(f32)
        pos = e > 0
        ln = np.where(pos, np.log(np.where(pos, e, f32(1)).astype(np.float64)), 0.0)
        out = np.zeros((num_labels + 1, 5), dtype=acc_dtype)
        np.add.at(out[:, 0], r, se.astype(acc_dtype))
        np.add.at(out[:, 1], r, e.astype(acc_dtype))
        np.add.at(out[:, 2], r, ln.astype(acc_dtype))
        np.add.at(out[:, 3], r, (e == 0).astype(acc_dtype))
        np.add.at(out[:, 4], r, np.ones(r.shape, dtype=acc_dtype))
        tabs = np.zeros((num_labels + 1, 3))
        for k, t in enumerate((se, e, np.abs(ln))):
            np.add.at(tabs[:, k], r, np.abs(t.astype(np.float64)))
    return {"table": out.astype(np.float64), "abs": tabs, "ln_bound": (1.5 * 2.0 ** -53 + 1e-12) * tabs[:, 2]}


def shot_of_rows(train_labels, num_labels=None, many_shot_thr=100, low_shot_thr=20):
    """train.py:340-357: per row the shot of its label by the label's count among ``train_labels.astype(int)``; the last ("other")
    row has count 0. Returns (shots [num_labels + 1] of str, num_labels)."""
    hist = np.bincount(np.array(train_labels).astype(int).reshape(-1))
    if num_labels is None:
        num_labels = hist.shape[0]
    counts = np.zeros(num_labels + 1, dtype=np.int64)
    counts[:min(num_labels, hist.shape[0])] = hist[:num_labels]
    return np.array(["many" if c > many_shot_thr else ("low" if c < low_shot_thr else "median") for c in counts]), num_labels


def metrics(row):
    """One pooled row (5 numbers) -> mse / l1 / gmean / num, nan for an empty pool (train.py:375-389)."""
    if row[4] == 0:
        return {"mse": float("nan"), "l1": float("nan"), "gmean": float("nan"), "num": 0}
    return {"mse": float(row[0] / row[4]), "l1": float(row[1] / row[4]),
            "gmean": 0.0 if row[3] > 0 else float(np.exp(row[2] / row[4])), "num": int(row[4])}


def results(tab, shots):
    tab = np.asarray(tab, dtype=np.float64)
    out = {"overall": metrics(tab.sum(axis=0))}
    for s in SHOTS:
        out[s] = metrics(tab[shots == s].sum(axis=0))
    return out


def golden_rows(res):
    """results dict -> (validate triple [3], shot rows [3, 3]) in the layout of tests/golden/validate.npz."""
    tri = np.array([res["overall"][k] for k in ("mse", "l1", "gmean")])
    return tri, np.array([[res[s][k] for k in ("mse", "l1", "gmean")] for s in SHOTS])
