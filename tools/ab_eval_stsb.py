"""STS-B-DIR balanced scorer: ``dirhip.eval_stsb.STSShotAverage.get_metric`` against a host scorer that makes the calls the
reference's ``STSShotAverage`` makes (lists on the host, a numpy bin lookup per label, ``np.mean`` / ``gmean`` / ``pearsonr`` /
``spearmanr`` per shot group), on the same tensors, same process (``--out profiles/stsb_eval.txt``).

    python tools/ab_eval_stsb.py [--n 1000 --batch 16 --reps 11 --out F]

Not measured yet: no figure of this tool exists, and nothing may quote one until it has run on an MI355X. In particular there is no
time for the O(n^2) rank pass at the n = 65536 cap.

Inputs: ``--n`` seeded (prediction, label) pairs, labels on the 0.2 grid of STS-B, every seventh prediction rounded (ties), resident on
the device and fed in batches of ``--batch``.
  (a) device  ``__call__`` per batch (device-to-device copies) + ``get_metric()`` (three launches, one 480-byte read-back)
  (b) host    ``.tolist()`` per batch (one device-to-host copy each) + the numpy / scipy scorer
A repetition is one whole evaluation inside a host clock that ends after the metrics are on the host; medians over ``--reps``
repetitions after a warm-up repetition of each arm. The two dicts are compared."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "imbalanced-regression_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.stats import gmean, pearsonr, spearmanr  # noqa: E402

from dirhip.eval_stsb import STSShotAverage  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("ab_eval_stsb.py measures on the GPU; none found")
dev = torch.device("cuda:0")
METRICS = ['mse', 'l1', 'gmean', 'pearsonr', 'spearmanr']

rng = np.random.default_rng(0)
label_h = (rng.integers(0, 26, a.n) / 5).astype(np.float32)
pred_h = np.clip(label_h / 5 + rng.normal(0, 0.12, a.n), 0, 1).astype(np.float32)
pred_h[::7] = np.round(pred_h[::7], 1)
pred, label = torch.tensor(pred_h, device=dev), torch.tensor(label_h, device=dev)
scorer = STSShotAverage(metric=METRICS)


def device_arm():
    scorer.reset()
    for s in range(0, a.n, a.batch):
        scorer(pred[s:s + a.batch], label[s:s + a.batch])
    return scorer.get_metric()


def host_arm():
    ps, ls = [], []
    for s in range(0, a.n, a.batch):
        ps += pred[s:s + a.batch].tolist()
        ls += label[s:s + a.batch].tolist()
    edges = np.histogram(a=np.array([], dtype=np.float32), bins=50, range=(0., 5.))[1]
    bins = [49 if l == 5. else int(np.where(edges > l)[0][0]) - 1 for l in ls]
    shot = np.array(['many' if b in scorer._shot_idx['many'] else 'medium' if b in scorer._shot_idx['medium'] else 'few' for b in bins])
    out = {}
    for s in ('overall', 'many', 'medium', 'few'):
        p = np.array(ps) * 5. if s == 'overall' else np.array(ps)[shot == s] * 5.
        l = np.array(ls) if s == 'overall' else np.array(ls)[shot == s]
        d = np.abs(p - l)
        d0 = np.where(d == 0., 1e-10, d)
        out[s] = {'mse': np.mean(d ** 2) if p.size else 0., 'l1': np.mean(d) if p.size else 0., 'gmean': gmean(d0) if p.size else 0.,
                  'pearsonr': pearsonr(p, l)[0] if p.size > 1 else 0., 'spearmanr': spearmanr(p, l)[0] if p.size > 1 else 0.,
                  'num_samples': p.size}
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


arms = {"device": device_arm, "host": host_arm}
for fn in arms.values():
    timed(fn)
rows = {k: [] for k in arms}
for _ in range(a.reps):
    for k, fn in arms.items():
        rows[k].append(timed(fn))
med = lambda v: sorted(v)[len(v) // 2]
da, ha = device_arm(), host_arm()
worst = max(abs(float(da[s][k]) - float(ha[s][k])) / max(abs(float(ha[s][k])), 1e-300) for s in da for k in METRICS if float(ha[s][k]) == float(ha[s][k]))
out = {"n": a.n, "batch": a.batch, "repetitions": a.reps,
       "median_wall_ms_per_evaluation": {k: round(med(v) * 1e3, 3) for k, v in rows.items()},
       "wall_ms_all": {k: [round(x * 1e3, 3) for x in v] for k, v in rows.items()},
       "host_over_device_wall": med(rows["host"]) / med(rows["device"]),
       "largest_relative_difference_of_a_metric": worst, "overall_device": da["overall"],
       "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
text = json.dumps(out, indent=1, default=float)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
