"""Weighted regression losses with STS-B-DIR's defaults — drop-in for ``sts-b-dir/loss.py``.

The same five names, signatures and ``dir_weighted_loss`` kernel as ``dirhip.loss`` (value and d loss / d inputs in one launch); only
the defaults differ from the age projects': ``weighted_huber_loss(beta=0.5)`` (age: 1.) and ``weighted_focal_*_loss(beta=20.)``
(age: .2), as the labels live in [0, 5] and the model's output in [0, 1]. No CPU fallback.
"""
import torch  # noqa: F401
import torch.nn.functional as F  # noqa: F401  (re-exported: reference modules rely on star-imports)

from .loss import _weighted


def weighted_mse_loss(inputs, targets, weights=None):
    return _weighted('mse', inputs, targets, weights)


def weighted_l1_loss(inputs, targets, weights=None):
    return _weighted('l1', inputs, targets, weights)


def weighted_huber_loss(inputs, targets, weights=None, beta=0.5):
    return _weighted('huber', inputs, targets, weights, beta)


def weighted_focal_mse_loss(inputs, targets, weights=None, activate='sigmoid', beta=20., gamma=1):
    return _weighted('focal_mse', inputs, targets, weights, beta, gamma, activate)


def weighted_focal_l1_loss(inputs, targets, weights=None, activate='sigmoid', beta=20., gamma=1):
    return _weighted('focal_l1', inputs, targets, weights, beta, gamma, activate)
