"""Drop-in for the FDS / LDS / evaluation part of the reference's ``sts-b-dir/util.py``: ``calibrate_mean_var`` (clip [0.5, 2]),
``get_lds_kernel_window`` and the balanced scorer ``STSShotAverage`` (device tensors in, the reference's dict out).
The AllenNLP model / trainer helpers of that file are out of scope."""
import _path  # noqa: F401
from dirhip.eval_stsb import STSShotAverage  # noqa: F401
from dirhip.fds_stsb import calibrate_mean_var  # noqa: F401
from dirhip.utils import get_lds_kernel_window  # noqa: F401
