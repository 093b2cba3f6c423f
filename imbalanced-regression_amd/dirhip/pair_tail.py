"""Fused STS-B-DIR pair head — what ``HeadlessPairEncoder.forward`` does after the LSTM plus ``MultiTaskModel.forward`` up to the
loss (reference ``sts-b-dir/models.py:155-166`` and ``:84-114``): dropout on the two sentence encodings ``[B, T, D]``, padding to
``-inf``, max over time, ``cat[u, v, |u - v|, u * v]``, ``FDS.smooth`` in place, ``Linear(4D, 1)``. Two launches forward
(``dir_pair_tail_fwd``) and ONE autograd node whose backward is three (``dir_pair_tail_bwd``): the encodings are read once and never
rewritten, the calibrated ``[B, 4D]`` embedding is written once and its gradient never, ``ds1`` / ``ds2`` are written by one streaming
pass, weight / bias gradients by a fixed-order two-stage reduction. The STS-B counterpart of ``dirhip.tail``; float32, deterministic,
no atomics. No CPU fallback.

``pair_tail_forward(s1_enc, s2_enc, mask1, mask2, linear, fds, labels, dropout)`` returns ``(logits [B, 1], pair_emb [B, 4D])`` with
``pair_emb`` the CALIBRATED embedding when ``fds`` is given (the reference calibrates in place, so its ``out['embs']`` is that tensor).
``PairHead`` wraps it with the regressor, the train / eval and ``start_smooth`` rules and the weighted loss of ``dirhip.loss_stsb``.
The dropout mask is Philox4x32-10 of a (seed, offset) pair per sentence drawn from the device's default generator
(``tail.draw_philox``), regenerated in the backward, never stored; it is not ``nn.Dropout``'s random stream.
"""
import torch
import torch.nn as nn

from . import _lib as L
from . import gradsink
from . import loss_stsb
from .tail import draw_philox

_NO_DROP = (0, 0, 0, 0.0)


def _mask_u8(mask, b, t, name):
    """[B, T] (or [B, T, 1]) mask of any dtype -> contiguous uint8 view / copy, non-zero = a token."""
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not mask.is_cuda:
        raise L.DirHipError(f"{name} is on {mask.device}: the pair head runs only as HIP kernels on an AMD GPU (no CPU fallback)")
    mask = mask.reshape(b, t)
    if mask.dtype not in (torch.bool, torch.uint8):
        mask = mask != 0                                       # the reference passes .long() masks (models.py:145)
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _workspace(b, d, dev):
    return torch.empty(max(int(L.lib().dir_pair_tail_workspace(b, d)), 256), dtype=torch.uint8, device=dev)


class _PairTailFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s1, s2, mask1, mask2, weight, bias, bins, m1, scale, m2, drop):
        ctx.set_materialize_grads(False)
        b, t1, d = s1.shape
        t2 = s2.shape[1]
        dev = s1.device
        w32 = weight.detach().reshape(-1)
        if w32.dtype != torch.float32 or not w32.is_contiguous():
            w32 = w32.float().contiguous()
        b32 = bias.detach().reshape(-1).float().contiguous()
        emb = torch.empty((b, 4 * d), dtype=torch.float32, device=dev)
        uv = torch.empty((b, 2 * d), dtype=torch.float32, device=dev)
        arg1 = torch.empty((b, d), dtype=torch.int32, device=dev)
        arg2 = torch.empty((b, d), dtype=torch.int32, device=dev)
        logits = torch.empty((b, 1), dtype=torch.float32, device=dev)
        ws = _workspace(b, d, dev)
        nb = 0 if m1 is None else m1.shape[0]
        drop = _NO_DROP if drop is None else drop
        L.check(L.lib().dir_pair_tail_fwd(L.ptr(s1), L.ptr(s2), L.ptr(mask1), L.ptr(mask2), b, t1, t2, d, L.ptr(bins), nb, L.ptr(m1),
                                          L.ptr(scale), L.ptr(m2), L.ptr(w32), L.ptr(b32), *drop, L.ptr(emb), L.ptr(uv), L.ptr(arg1),
                                          L.ptr(arg2), L.ptr(logits), L.ptr(ws), ws.numel(), L.stream_ptr(dev)), "dir_pair_tail_fwd")
        ctx.save_for_backward(emb, uv, arg1, arg2, bins, scale, w32)
        ctx.drop, ctx.nb = drop, nb
        ctx.dims = (b, t1, t2, d)
        ctx.w_shape, ctx.b_shape = weight.shape, bias.shape
        ctx.sinks = (gradsink.lookup(weight), gradsink.lookup(bias))
        ctx.mark_non_differentiable(arg1, arg2)
        return logits, emb, arg1, arg2

    @staticmethod
    def backward(ctx, dlogits, demb, _da1, _da2):
        emb, uv, arg1, arg2, bins, scale, w32 = ctx.saved_tensors
        b, t1, t2, d = ctx.dims
        dev = emb.device
        if dlogits is None:
            dlogits = torch.zeros(b, dtype=torch.float32, device=dev)
        dlogits = dlogits.reshape(-1).float().contiguous()
        if demb is not None:
            demb = demb.float().contiguous()
        need_w = ctx.needs_input_grad[4] or ctx.needs_input_grad[5]
        ds1 = torch.empty((b, t1, d), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        ds2 = torch.empty((b, t2, d), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        dw = gradsink.out_for(ctx.sinks[0], (4 * d,), dev) if need_w else None  # (bucket slots of the data-parallel engine, if any)
        db = gradsink.out_for(ctx.sinks[1], (1,), dev) if need_w else None
        ws = _workspace(b, d, dev) if need_w else None
        L.check(L.lib().dir_pair_tail_bwd(L.ptr(dlogits), L.ptr(demb), L.ptr(bins), ctx.nb, L.ptr(scale), L.ptr(w32), L.ptr(emb),
                                          L.ptr(uv), L.ptr(arg1), L.ptr(arg2), b, t1, t2, d, *ctx.drop, L.ptr(ds1), L.ptr(ds2),
                                          L.ptr(dw), L.ptr(db), L.ptr(ws), 0 if ws is None else ws.numel(), L.stream_ptr(dev)),
                "dir_pair_tail_bwd")
        return (ds1, ds2, None, None, None if dw is None else dw.reshape(ctx.w_shape), None if db is None else db.reshape(ctx.b_shape),
                None, None, None, None, None)


def _encoding(x, name):
    x = L.require_device_tensor(x, torch.float32, name, contiguous=False)
    if x.dim() != 3:
        raise ValueError(f"{name} must be [B, T, D], got {tuple(x.shape)}")
    return x if x.is_contiguous() else x.contiguous()


def pair_tail_apply(s1_enc, s2_enc, mask1, mask2, weight, bias, bins=None, m1=None, scale=None, m2=None, drop=None):
    """The autograd node on raw tensors: ``bins`` [B] int32 and the three ``[nb, 4D]`` tables (all four or none), ``drop`` =
    ``(seed, offset1, offset2, p)`` or None. Returns ``(logits [B, 1], pair_emb [B, 4D], arg1 [B, D], arg2 [B, D])``; the two int32
    argmax maps (lowest t of the maximum, -1 for an all-padding sample) are what the backward routes the gradient by."""
    s1, s2 = _encoding(s1_enc, "s1_enc"), _encoding(s2_enc, "s2_enc")
    if s1.shape[0] != s2.shape[0] or s1.shape[2] != s2.shape[2]:
        raise ValueError(f"s1_enc {tuple(s1.shape)} and s2_enc {tuple(s2.shape)} must agree in B and D")
    b, t1, d = s1.shape
    if weight.numel() != 4 * d or bias is None or bias.numel() != 1:
        raise ValueError(f"the regressor must be Linear({4 * d}, 1) with a bias")
    return _PairTailFn.apply(s1, s2, _mask_u8(mask1, b, t1, "mask1"), _mask_u8(mask2, b, s2.shape[1], "mask2"), weight, bias,
                             bins, m1, scale, m2, drop)


def pair_tail_forward(s1_enc, s2_enc, mask1, mask2, linear, fds=None, labels=None, dropout=None):
    """``fds``: the ``dirhip.fds_stsb.FDS`` module when its calibration is live for this call (training, epoch >= start_smooth), else
    None; ``labels`` [B] or [B, 1] then. ``dropout``: the drop probability when dropout is live (training mode), else None / 0."""
    drop = None
    if dropout:
        dev = s1_enc.device
        if not s1_enc.is_cuda:
            raise L.DirHipError(f"s1_enc is on {dev}: the pair head runs only as HIP kernels on an AMD GPU (no CPU fallback)")
        (seed, off1), (_, off2) = draw_philox(dev), draw_philox(dev)
        drop = (seed, off1, off2, float(dropout))
    if fds is None:
        return pair_tail_apply(s1_enc, s2_enc, mask1, mask2, linear.weight, linear.bias, drop=drop)[:2]
    assert labels is not None and labels.numel() == s1_enc.shape[0] and fds.feature_dim == 4 * s1_enc.shape[2]
    m1 = fds.running_mean_last_epoch if fds.running_mean_last_epoch.is_contiguous() else fds.running_mean_last_epoch.contiguous()
    m2 = fds.smoothed_mean_last_epoch if fds.smoothed_mean_last_epoch.is_contiguous() else fds.smoothed_mean_last_epoch.contiguous()
    return pair_tail_apply(s1_enc, s2_enc, mask1, mask2, linear.weight, linear.bias, fds._bins(labels), m1, fds._scale_table(), m2,
                           drop)[:2]


class PairHead(nn.Module):
    """Everything of the reference's STS-B-DIR model after the sentence encoder: ``HeadlessPairEncoder``'s dropout / masked max-pool /
    pair features (models.py:155-166) and ``MultiTaskModel.forward`` (models.py:84-114: FDS.smooth, the regressor, the loss).
    ``d_pair`` is the width D of one sentence encoding (the reference's ``d_pair``; the regressor is ``Linear(4 * d_pair, 1)``);
    ``fds`` a ``dirhip.fds_stsb.FDS(feature_dim=4 * d_pair)`` or None. ``forward`` returns the reference's dict: ``logits``, ``loss``
    (targets ``label / 5``) and, when training with FDS, ``embs`` / ``labels`` for the epoch's ``update_running_stats``. The scorer
    call of models.py:109-111 is the caller's (``dirhip.eval_stsb.STSShotAverage``)."""

    def __init__(self, d_pair, fds=None, start_smooth=1, loss='mse', huber_beta=0.5, dropout=0.2):
        super().__init__()
        if not hasattr(loss_stsb, f"weighted_{loss}_loss"):
            raise ValueError(f"unknown loss {loss!r}")
        self.d_pair = d_pair
        self.FDS = fds
        self.start_smooth = start_smooth
        self.loss = loss
        self.huber_beta = huber_beta
        self.dropout = dropout
        self.pred_layer = nn.Linear(4 * d_pair, 1)

    def forward(self, s1_enc, s2_enc, mask1, mask2, label, epoch=None, weight=None):
        with_fds = self.training and self.FDS is not None
        smooth = with_fds and epoch is not None and epoch >= self.start_smooth and epoch >= self.FDS.start_smooth   # models.py:89-91, fds.py:128
        logits, emb = pair_tail_forward(s1_enc, s2_enc, mask1, mask2, self.pred_layer, self.FDS if smooth else None,
                                        label if smooth else None, self.dropout if self.training else None)
        out = {}
        if with_fds:
            out['embs'] = emb
            out['labels'] = label
        targets = label / 5.
        fn = getattr(loss_stsb, f"weighted_{self.loss}_loss")
        if self.loss == 'huber':
            out_loss = fn(inputs=logits, targets=targets, weights=weight, beta=self.huber_beta)
        else:
            out_loss = fn(inputs=logits, targets=targets, weights=weight)
        out['logits'] = logits
        out['loss'] = out_loss
        return out
