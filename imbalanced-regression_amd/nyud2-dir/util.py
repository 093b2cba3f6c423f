"""Drop-in for the reference's ``nyud2-dir/util.py``: ``Evaluator`` (one fused HIP pass per batch instead of per-pixel host work),
``calibrate_mean_var`` (clip [0.2, 5]), ``get_lds_kernel_window`` and ``query_yes_no``."""
import _path  # noqa: F401
from dirhip.eval_nyud2 import Evaluator  # noqa: F401
from dirhip.fds_nyud2 import calibrate_mean_var  # noqa: F401
from dirhip.utils import get_lds_kernel_window, query_yes_no  # noqa: F401
