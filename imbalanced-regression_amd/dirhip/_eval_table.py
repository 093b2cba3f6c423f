"""The persistent float64 device table of the additive evaluators (``eval_age.ShotEvaluator``, ``eval_nyud2.Evaluator``): created on
the device of the first call, accumulated into by every call, summed over ranks by one ``all_reduce``."""
import torch

from . import _lib as L


class TableEvaluator:
    def __init__(self, rows, cols, first="call"):
        self._table_shape = (int(rows), int(cols))
        self._first = first                    # what the subclass calls its accumulating method, for the message below
        self.table = None                      # [rows, cols] float64 on the device of the first call

    def _table_on(self, device):
        if self.table is None:
            self.table = torch.zeros(*self._table_shape, dtype=torch.float64, device=device)
        elif self.table.device != device:
            raise L.DirHipError(f"{type(self).__name__} holds its table on {self.table.device}, got tensors on {device}")
        return self.table

    def reset(self):
        if self.table is not None:
            self.table.zero_()

    def merge_across_ranks(self, group=None):
        """Sum the table over the ranks of ``group`` (a validation / test set sharded over the one-process-per-GPU engine):
        afterwards every rank reads the same results. No-op without an initialised process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return
        if self.table is None:
            raise L.DirHipError(f"merge_across_ranks before the first {self._first}: the table's device is not known yet")
        dist.all_reduce(self.table, group=group)
