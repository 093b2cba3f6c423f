"""Label Distribution Smoothing weights of STS-B-DIR (host) — the arithmetic of ``sts-b-dir/tasks.py:44-73`` (``load_tsv``).

The labels are bucketed by the edges of ``np.histogram(targs, bins=bucket_num, range=(0., 5.))`` (50 buckets of [0, 5]) instead of
``int(label)``, the ``inverse`` counts are not clipped to 5..1000, and everything else is the age projects' recipe: the numbers come
from the native host routine ``dir_lds_weights_binned`` in ``libdir_hip.so`` (bit-exact with numpy / scipy's accumulation orders,
SURVEY Appendix E); the edges and the smoothing window come from numpy / scipy on the host like the reference.
"""
import logging

import numpy as np

from . import ops
from .utils import get_lds_kernel_window

print = logging.info


def prepare_weights(targs, reweight, lds=False, lds_kernel='gaussian', lds_ks=5, lds_sigma=2, bucket_num=50):
    """``targs``: the training labels (the reference's are ``np.float32``, tasks.py:92; anything else is cast to float32 first).
    Returns a list of ``np.float32`` like the reference, or ``None`` when ``reweight == 'none'`` (the reference then returns no
    weights at all)."""
    assert reweight in {'none', 'inverse', 'sqrt_inv'}
    assert reweight != 'none' if lds else True, "Set reweight to \'inverse\' (default) or \'sqrt_inv\' when using LDS"
    labels = np.asarray(targs, dtype=np.float32).reshape(-1)
    if not len(labels) or reweight == 'none':
        return None
    _, edges = np.histogram(np.array([], dtype=np.float32), bins=bucket_num, range=(0., 5.))      # tasks.py:49, float32 edges
    print(f"Using re-weighting: [{reweight.upper()}]")
    window = None
    if lds:
        window = get_lds_kernel_window(lds_kernel, lds_ks, lds_sigma)
        print(f'Using LDS: [{lds_kernel.upper()}] ({lds_ks}/{lds_sigma})')
    return list(ops.lds_weights_binned(labels, edges, reweight, lds, window))
