"""Balanced depth evaluation of NYUD2-DIR — ``nyud2-dir/util.py:35-133`` (``Evaluator``) and the loop of ``nyud2-dir/test.py:39-59``.

The reference keeps every masked pixel of the test set on the host (two float32 vectors of ~2 x 0.7 GB), maps ``get_bin_idx`` over
them in Python and evaluates the nine metrics four times (overall / many / medium / few-shot depth buckets). Here each call only
enqueues ``dir_depth_eval_accumulate`` on a persistent ``[100, 8]`` float64 table on the device (per 0.1 m bucket: sum d^2, sum d,
sum d/depth, sum |lg10 pred - lg10 depth|, the three delta counts, the pixel count); ``evaluate_shot()`` reads those 800 numbers
once and adds bucket rows. ``update(pred_lowres, depth, mask)`` also replaces ``F.interpolate(..., align_corners=True)`` and the
boolean indexing of test.py:52-54: the upsampled prediction is formed in registers and never stored.

Differences from the reference that a caller can see: sums are float64 (the reference's are torch float32 sums), so metrics agree
to float32 summation error, not bit for bit; a depth <= 0 counts into bucket 0 (the reference's negative index belongs to no shot).
"""
import logging

import numpy as np
import torch

from . import _lib as L
from . import ops
from ._eval_table import TableEvaluator

COLUMNS = ("MSE", "MAE", "ABS_REL", "LG10", "DELTA1", "DELTA2", "DELTA3", "NUM")        # column order of the device table


class Evaluator(TableEvaluator):
    def __init__(self, bucket_num=100, mult=10.0):
        # nyud2-dir/util.py:37-43: depth buckets (0.1 m) by the number of training pixels they hold
        self.shot_idx = {
            'many': [9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27,
                     28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 47, 49],
            'medium': [7, 8, 46, 48, 50, 51, 52, 53, 54, 55, 56, 58, 60, 61, 63],
            'few': [0, 1, 2, 3, 4, 5, 6, 57, 59, 62, 64, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77,
                    78, 79, 80, 81, 82, 83, 84, 85, 86, 87, 88, 89, 90, 91, 92, 93, 94, 95, 96, 97, 98, 99]
        }
        self.bucket_num, self.mult = int(bucket_num), float(mult)
        super().__init__(self.bucket_num, len(COLUMNS))

    def __call__(self, output, depth):
        """The reference's call form: two tensors of equal element count (``output[mask], depth[mask]`` in test.py). Enqueue only."""
        output = L.require_device_f32(output, "output").contiguous().view(1, 1, -1)
        depth = L.require_device_f32(depth, "depth").contiguous().view(1, 1, -1)
        if output.numel() != depth.numel():
            raise ValueError(f"output and depth differ in size: {output.numel()} vs {depth.numel()}")
        if depth.numel():
            ops.depth_eval_accumulate(output, depth, None, self._table_on(depth.device), self.mult)

    def update(self, pred, depth, mask=None):
        """Fused form of test.py:52-54: ``pred`` [N, 1, h, w] (or [N, h, w]) is the network output, ``depth`` [N, 1, H, W] the ground
        truth, ``mask`` (bool / uint8, depth's shape) the pixels to keep. Equivalent to
        ``self(F.interpolate(pred, (H, W), mode='bilinear', align_corners=True)[mask], depth[mask])`` without any of the intermediates."""
        pred, depth = L.require_device_f32(pred, "pred").contiguous(), L.require_device_f32(depth, "depth").contiguous()
        if pred.dim() == 4 and pred.shape[1] == 1:
            pred = pred[:, 0]
        if depth.dim() == 4 and depth.shape[1] == 1:
            depth = depth[:, 0]
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
                raise L.DirHipError("mask must be a GPU tensor (no CPU fallback)")
            if mask.dtype not in (torch.bool, torch.uint8):
                raise TypeError(f"mask must be bool or uint8, got {mask.dtype}")
            mask = mask.contiguous()
            if mask.dim() == 4 and mask.shape[1] == 1:
                mask = mask[:, 0]
        if pred.dim() != 3 or depth.dim() != 3:
            raise ValueError(f"pred / depth must be [N, 1, h, w] / [N, 1, H, W], got {tuple(pred.shape)} / {tuple(depth.shape)}")
        ops.depth_eval_accumulate(pred, depth, mask, self._table_on(depth.device), self.mult)

    @staticmethod
    def get_bin_idx(x):
        return min(int(x * np.float32(10)), 99)

    @staticmethod
    def _metrics(row):
        """One summed table row (8 float64) -> the reference's dict (util.py:89-133)."""
        errors = {'MSE': 0, 'RMSE': 0, 'ABS_REL': 0, 'LG10': 0, 'MAE': 0, 'DELTA1': 0, 'DELTA2': 0, 'DELTA3': 0, 'NUM': 0}
        num = float(row[7])
        if num > 0:
            for k, name in enumerate(COLUMNS[:7]):
                errors[name] = float(row[k] / num)
            errors['NUM'] = int(num)
        errors['RMSE'] = float(np.sqrt(errors['MSE']))
        return errors

    @staticmethod
    def evaluate(output, target):
        """util.py:89-133 on device tensors: the metrics of all pixels whose target is not NaN (one kernel, one read-back)."""
        ev = Evaluator()
        ev(output, target)
        if ev.table is None:
            return Evaluator._metrics(np.zeros(8))
        return Evaluator._metrics(ev.table.cpu().numpy().sum(axis=0))

    def evaluate_shot(self):
        table = np.zeros((self.bucket_num, 8)) if self.table is None else self.table.cpu().numpy()      # the only synchronisation
        metric_dict = {'overall': self._metrics(table.sum(axis=0))}
        for shot in ('many', 'medium', 'few'):
            metric_dict[shot] = self._metrics(table[[i for i in self.shot_idx[shot] if i < self.bucket_num]].sum(axis=0))

        logging.info('\n***** TEST RESULTS *****')
        for shot in ['Overall', 'Many', 'Medium', 'Few']:
            logging.info(f" * {shot}: RMSE {metric_dict[shot.lower()]['RMSE']:.3f}\t"
                         f"ABS_REL {metric_dict[shot.lower()]['ABS_REL']:.3f}\t"
                         f"LG10 {metric_dict[shot.lower()]['LG10']:.3f}\t"
                         f"MAE {metric_dict[shot.lower()]['MAE']:.3f}\t"
                         f"DELTA1 {metric_dict[shot.lower()]['DELTA1']:.3f}\t"
                         f"DELTA2 {metric_dict[shot.lower()]['DELTA2']:.3f}\t"
                         f"DELTA3 {metric_dict[shot.lower()]['DELTA3']:.3f}\t"
                         f"NUM {metric_dict[shot.lower()]['NUM']}")

        return metric_dict
