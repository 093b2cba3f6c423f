"""NYUD2-DIR training loss — ``nyud2-dir/train.py:200``: ``loss = torch.mean(((output - depth) ** 2) * weight)`` with the per-pixel
LDS weight of ``loaddata.py:57-69`` (``bucket_weights[min(int(d * 10), 99)]``) looked up inside the kernel.

One hand-written HIP launch (``dir_depth_loss``, plus its one-workgroup fold) emits the scalar loss and d loss / d output together,
instead of the binning kernel, the gather that writes a weight map, four element-wise torch kernels forward, as many in the autograd
backward and a float32 library reduction. The sum is float64 in a fixed order: the loss is bit-reproducible. No CPU fallback.
"""
import numpy as np
import torch

from . import _lib as L
from . import ops

MULT = 10.0                 # 0.1 m buckets (loaddata.py:58)
_TABLES = {}                # (bucket weights as bytes, device) -> device table


class _DepthLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, depth, table, need_grad):
        loss, dx_unit = ops.depth_loss(output, depth, table, MULT, need_grad)
        if need_grad:
            ctx.save_for_backward(dx_unit)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (dx_unit,) = ctx.saved_tensors
        grad_out = grad_out.contiguous().to(torch.float32)
        return ops.scale_by_device_scalar(dx_unit, grad_out), None, None, None


def device_table(bucket_weights, device):
    """The bucket weights as a float32 tensor on ``device``, uploaded once per (weights, device)."""
    if bucket_weights is None:
        return None
    if isinstance(bucket_weights, torch.Tensor):
        return L.require_device_tensor(bucket_weights, torch.float32, "bucket_weights")
    host = np.ascontiguousarray(bucket_weights, dtype=np.float32)
    key = (host.tobytes(), device)
    table = _TABLES.get(key)
    if table is None:
        table = _TABLES[key] = torch.tensor(host, device=device)
    return table


def weighted_depth_mse_loss(output, depth, bucket_weights=None):
    """``torch.mean(((output - depth) ** 2) * weight)``, ``weight = bucket_weights[min(int(depth * 10), 99)]`` per pixel (1 without
    bucket weights). ``output`` / ``depth``: float32 device tensors of one shape ([B, 1, H, W] or any other); ``bucket_weights``: the
    list of ``get_bucket_weights`` (or a float32 tensor already on the device), or None. Differentiable in ``output``."""
    if not isinstance(output, torch.Tensor) or not isinstance(depth, torch.Tensor):
        raise TypeError("output and depth must be torch tensors")
    if not output.is_cuda or not depth.is_cuda:
        raise L.DirHipError(f"weighted_depth_mse_loss: output on {output.device}, depth on {depth.device}; the loss runs only as a "
                            f"HIP kernel on an AMD GPU (no CPU fallback)")
    if depth.requires_grad:
        raise NotImplementedError("the gradient w.r.t. depth is not produced (the reference never uses it)")
    if output.shape != depth.shape:
        raise ValueError(f"output and depth differ in shape: {tuple(output.shape)} vs {tuple(depth.shape)}")
    if output.dtype != torch.float32 or depth.dtype != torch.float32:
        raise TypeError("output and depth must be float32 (the reference asserts it, loaddata.py:64)")
    need_grad = output.requires_grad and torch.is_grad_enabled()          # under no_grad no gradient buffer is written
    return _DepthLossFn.apply(output.contiguous(), depth.contiguous(), device_table(bucket_weights, output.device), need_grad)
