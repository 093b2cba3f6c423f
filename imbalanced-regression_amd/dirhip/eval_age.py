"""Balanced age evaluation of IMDB-WIKI-DIR / AgeDB-DIR — ``validate`` and ``shot_metrics`` of ``imdb-wiki-dir/train.py:286-391``.

The reference keeps every prediction of the validation set, copies them to the host and, for each distinct validation label, rescans
all training labels and slices the predictions. Here each ``update`` only enqueues ``dir_age_eval_accumulate`` on a persistent
``[num_labels + 1, 5]`` float64 table on the device (per integer label: sum e^2, sum e, sum ln e over e > 0, the number of e == 0,
the sample count; the last row collects every label that is no training label: fractional, negative, >= num_labels);
``results()`` reads those numbers once and pools the rows by the training-set frequency of their label. Because the table adds,
a validation set can be sharded over the ranks of the one-process-per-GPU engine: ``merge_across_ranks()`` is one ``all_reduce``.

Differences from the reference that a caller can see:
  * sums are float64 (the reference's are float32 numpy / torch sums, and its G-Mean takes a float32 ``log``);
  * the overall MSE / L1 are sum / NUM over the whole set, not the batch-size-weighted average of per-batch float32 means
    (``AverageMeter``): they agree to float32 rounding, not bit for bit.
"""
import numpy as np
import torch

from . import _lib as L
from . import ops
from ._eval_table import TableEvaluator

COLUMNS = ("SE", "AE", "LN", "ZERO", "NUM")        # column order of the device table
SHOTS = ("many", "median", "low")
MAX_ROWS = 256                                     # the kernel's LDS layout: num_labels + 1 <= 256


class ShotEvaluator(TableEvaluator):
    def __init__(self, train_labels, many_shot_thr=100, low_shot_thr=20):
        # train.py:340, :350-357: the training labels cast with astype(int), a label's shot by its count among them
        train = np.array(train_labels).astype(int).reshape(-1)
        if train.size == 0 or train.min() < 0:
            raise ValueError("train_labels must be a non-empty list of non-negative labels")
        self.train_hist = np.bincount(train)
        self.num_labels = int(self.train_hist.shape[0])
        if self.num_labels + 1 > MAX_ROWS:
            raise L.DirHipError(f"largest training label {self.num_labels - 1}: dir_age_eval_accumulate holds at most {MAX_ROWS - 1} "
                                f"label rows (no CPU fallback)")
        counts = np.append(self.train_hist, 0)                                     # the "other" row: no training sample has such a label
        self.shot_of_row = np.where(counts > many_shot_thr, "many", np.where(counts < low_shot_thr, "low", "median"))
        super().__init__(self.num_labels + 1, len(COLUMNS), first="update")

    def update(self, preds, labels, valid=None):
        """``preds`` / ``labels``: float32 GPU tensors of equal element count ([B] or [B, 1]); ``valid`` (bool / uint8, same count):
        samples to keep, e.g. False at the wrap-around padding of ``parallel.shard_indices``. Enqueue only."""
        preds, labels = L.require_device_f32(preds, "preds").contiguous(), L.require_device_f32(labels, "labels").contiguous()
        if preds.numel() != labels.numel():
            raise ValueError(f"preds and labels differ in size: {preds.numel()} vs {labels.numel()}")
        if valid is not None:
            if not isinstance(valid, torch.Tensor) or not valid.is_cuda:
                raise L.DirHipError("valid must be a GPU tensor (no CPU fallback)")
            if valid.dtype not in (torch.bool, torch.uint8):
                raise TypeError(f"valid must be bool or uint8, got {valid.dtype}")
            if valid.numel() != labels.numel():
                raise ValueError(f"valid and labels differ in size: {valid.numel()} vs {labels.numel()}")
            valid = valid.contiguous()
        if labels.numel():
            ops.age_eval_accumulate(preds, labels, valid, self._table_on(labels.device))

    @staticmethod
    def _metrics(row):
        """One pooled table row (5 float64) -> mse / l1 / gmean / num; an empty pool gives nan like ``train_main.shot_metrics``."""
        num = int(row[4])
        if num == 0:
            return {'mse': float('nan'), 'l1': float('nan'), 'gmean': float('nan'), 'num': 0}
        gmean = 0.0 if row[3] > 0 else float(np.exp(row[2] / row[4]))              # one zero error makes the geometric mean zero
        return {'mse': float(row[0] / row[4]), 'l1': float(row[1] / row[4]), 'gmean': gmean, 'num': num}

    def metrics_of(self, table):
        """The host half of ``results()``: a [num_labels + 1, 5] table -> the four dicts."""
        table = np.asarray(table, dtype=np.float64)
        if table.shape != (self.num_labels + 1, len(COLUMNS)):
            raise ValueError(f"table must be {(self.num_labels + 1, len(COLUMNS))}, got {table.shape}")
        out = {'overall': self._metrics(table.sum(axis=0))}
        for shot in SHOTS:
            out[shot] = self._metrics(table[self.shot_of_row == shot].sum(axis=0))
        return out

    def results(self):
        """{'overall' | 'many' | 'median' | 'low': {'mse', 'l1', 'gmean', 'num'}} — the only synchronisation."""
        table = np.zeros((self.num_labels + 1, len(COLUMNS))) if self.table is None else self.table.cpu().numpy()
        return self.metrics_of(table)
