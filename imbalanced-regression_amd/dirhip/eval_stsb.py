"""Balanced STS-B evaluation — ``STSShotAverage`` of ``sts-b-dir/util.py:101-172`` behind the reference's surface.

The reference appends every batch to two python lists, bins each label with a numpy call of its own and hands four slices to
numpy / scipy (``np.mean``, ``gmean``, ``pearsonr``, ``spearmanr``). Here ``__call__`` appends float32 GPU tensors to a growing
device buffer and ``get_metric`` makes ONE ``ops.stsb_eval`` call over the whole set (``dir_stsb_eval``: the per-group moment sums
in float64, and the rank sums as integers from an O(n^2) compare pass with no sort) and ONE read-back of 60 numbers; the host
turns those into the reference's dict. There is no CPU fallback.

What a caller can see differently from the reference:
  * sums are fixed-order float64 sums on the device instead of numpy's pairwise ones: MSE / L1 / G-Mean / Pearson agree to float64
    rounding. Spearman is computed from exact integer rank sums (ties get average ranks, as ``scipy.stats.rankdata``);
  * a label outside [0, 5], a NaN label or a NaN prediction raises ``DirHipError`` (the reference raises ``IndexError`` above 5 and
    silently counts a negative label as "few");
  * at most 65536 samples (``DirHipError`` above);
  * no sharding over ranks: Spearman's rho is not additive over shards (ranks are taken over the whole set), so a sharded
    evaluation would need an all-gather of the (pred, label) pairs. Out of scope here: evaluate on one rank.
"""
import math

import numpy as np
import torch

from . import _lib as L
from . import ops

MOMENT_COLUMNS = ("NUM", "ZERO", "SE", "AE", "LN", "SP", "SL", "SPP", "SLL", "SPL")      # columns of the device moment table
RANK_COLUMNS = ("SA", "SB", "SAA", "SBB", "SAB")                                          # columns of the device rank table
ROWS = ("many", "medium", "few", "overall")                                               # rows of both
MAX_SAMPLES = 65536
LN_ZERO = math.log(1e-10)            # util.py:153-156: a zero error enters the geometric mean as 1e-10


def metrics_of(moments, ranks, metric):
    """The host half of ``get_metric``: moments [4, 10] float64 and ranks [4, 5] integers -> {'many' | 'medium' | 'few' | 'overall':
    {every name of ``metric`` among mse / l1 / gmean / pearsonr / spearmanr, 'num_samples'}} (util.py:142-163)."""
    out = {}
    for r, shot in enumerate(ROWS):
        num, zero, se, ae, ln, sp, sl, spp, sll, spl = (float(v) for v in moments[r])
        n = int(num)
        m = {}
        sa, sb, saa, sbb, sab = (int(v) for v in ranks[r])                                            # python integers: exact
        cov_r, va, vb = n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb
        constant = va == 0 or vb == 0            # all ranks equal <=> all values equal: scipy's own test for a constant input, exactly
        if 'mse' in metric:
            m['mse'] = se / num if n > 0 else 0.
        if 'l1' in metric:
            m['l1'] = ae / num if n > 0 else 0.
        if 'gmean' in metric:
            m['gmean'] = math.exp((ln + zero * LN_ZERO) / num) if n > 0 else 0.
        if 'pearsonr' in metric:
            if n > 1:
                cov, vp, vl = num * spl - sp * sl, num * spp - sp * sp, num * sll - sl * sl
                ok = not constant and vp > 0 and vl > 0                                               # a constant input: nan, as scipy
                m['pearsonr'] = cov / math.sqrt(vp * vl) if ok else float('nan')
            else:
                m['pearsonr'] = 0.
        if 'spearmanr' in metric:
            if n > 1:
                m['spearmanr'] = cov_r / math.sqrt(va * vb) if not constant else float('nan')
            else:
                m['spearmanr'] = 0.
        m['num_samples'] = n
        out[shot] = m
    return out


class STSShotAverage:
    def __init__(self, metric):
        self._count = 0
        self._metric = metric
        self._num_bins = 50
        # under np.float32 division
        self._shot_idx = {
            'many': [0, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 49],
            'medium': [2, 4, 6, 8, 27, 35, 37],
            'few': [1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 29, 31, 33, 39, 41, 43, 45, 47]
        }
        # util.py:115-116: the reference's own call; float32 edges under numpy >= 2
        _, edges = np.histogram(a=np.array([], dtype=np.float32), bins=self._num_bins, range=(0., 5.))
        self._edges_host = np.asarray(edges, dtype=np.float32)
        group = np.full(self._num_bins, 2, dtype=np.uint8)                         # util.py:130-136: neither many nor medium is few
        group[self._shot_idx['many']] = 0
        group[self._shot_idx['medium']] = 1
        self._group_host = group
        self._pred = self._label = None          # device buffers [capacity] float32; the first _count entries are the set
        self._tables = None                      # (edges, group_of_bin) on the buffers' device

    def _get_bin_idx(self, label):
        """Host restatement for single labels (API compatibility; the hot path bins inside ``dir_stsb_eval``)."""
        if label == 5.:
            return self._num_bins - 1
        return int(np.where(self._edges_host > label)[0][0]) - 1

    def __call__(self, pred, label):
        """``pred`` / ``label``: float32 GPU tensors of equal element count ([B] or [B, 1]). Appends; enqueue only."""
        pred, label = L.require_device_f32(pred, "pred").detach().reshape(-1), L.require_device_f32(label, "label").detach().reshape(-1)
        if pred.numel() != label.numel():
            raise ValueError(f"pred and label differ in size: {pred.numel()} vs {label.numel()}")
        if pred.device != label.device:
            raise L.DirHipError(f"pred is on {pred.device}, label on {label.device}")
        k = pred.numel()
        if self._pred is not None and self._pred.device != pred.device:
            raise L.DirHipError(f"STSShotAverage holds its samples on {self._pred.device}, got tensors on {pred.device}")
        if self._count + k > MAX_SAMPLES:
            raise L.DirHipError(f"{self._count + k} samples: dir_stsb_eval ranks at most {MAX_SAMPLES} (no CPU fallback)")
        if self._pred is None or self._count + k > self._pred.numel():
            cap = min(MAX_SAMPLES, max(1024, 2 * (self._count + k)))
            grown = [torch.empty(cap, dtype=torch.float32, device=pred.device) for _ in range(2)]
            if self._count:
                grown[0][:self._count].copy_(self._pred[:self._count])
                grown[1][:self._count].copy_(self._label[:self._count])
            self._pred, self._label = grown
        self._pred[self._count:self._count + k].copy_(pred)
        self._label[self._count:self._count + k].copy_(label)
        self._count += k

    def _tables_on(self, device):
        if self._tables is None or self._tables[0].device != device:
            self._tables = (torch.tensor(self._edges_host, device=device), torch.tensor(self._group_host, device=device))
        return self._tables

    def device_tables(self):
        """(moments [4, 10] float64, ranks [4, 5] int64) as numpy arrays: one ``ops.stsb_eval`` call, one read-back."""
        if self._count == 0:
            return np.zeros((4, len(MOMENT_COLUMNS))), np.zeros((4, len(RANK_COLUMNS)), dtype=np.int64)
        edges, group = self._tables_on(self._pred.device)
        moments, ranks = ops.stsb_eval(self._pred[:self._count], self._label[:self._count], edges, group)
        both = ranks._base.cpu().numpy()                                           # the 60-word buffer both tables are views of
        moments, ranks = both[:40].view(np.float64).reshape(4, 10), both[40:].reshape(4, 5)
        if ranks[3, 0] < 0:
            raise L.DirHipError(f"STSShotAverage: {-int(ranks[3, 0])} of {self._count} samples have a label outside [0, 5], a NaN label "
                                f"or a NaN prediction")
        return moments, ranks

    def get_metric(self, reset=False, type=None):
        metric = metrics_of(*self.device_tables(), self._metric)
        if reset:
            self.reset()
        return metric['overall'] if type == 'overall' else metric

    def reset(self):
        self._count = 0                          # the buffers are kept for the next evaluation
