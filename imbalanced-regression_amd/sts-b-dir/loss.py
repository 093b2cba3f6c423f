"""Drop-in for the reference's ``sts-b-dir/loss.py`` (huber beta=0.5, focal beta=20.; also re-exports torch / F)."""
import _path  # noqa: F401
import torch  # noqa: F401
import torch.nn.functional as F  # noqa: F401
from dirhip.loss_stsb import (weighted_focal_l1_loss, weighted_focal_mse_loss, weighted_huber_loss,  # noqa: F401
                              weighted_l1_loss, weighted_mse_loss)
