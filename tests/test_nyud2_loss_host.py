"""CPU-side tests of the NYUD2-DIR training loss (``dir_depth_loss`` / ``dirhip.loss_nyud2``): the two C-ABI entry points (declared,
exported, bound; argument errors without a GPU), and the float32 numpy restatement of the kernel's per-pixel arithmetic, ``restate``,
which the GPU tests (tests/test_hip_nyud2_loss.py) use as their yardstick. The restatement is held here to torch's CPU
``torch.mean(((o - d) ** 2) * w)``: terms and autograd gradient bit for bit, the mean within the error bounds derived below.

Bounds (u = 2^-24, the unit round-off of float32; every weight is positive, so every term is >= 0 and |sum| = sum of |terms|):
  TERM_REL   a float32 term (d * d) * w with d = fl(p - z) differs from the real ((p - z)^2) w by at most (1 + u)^4 - 1 relatively
             (the rounding of d counts twice, then one rounding per product): 4.000001 u.  The float64 sum of the float32 terms divided
             by n and rounded to float32 therefore sits within (4.000001 + 1) u (+ float64 summation, < 1e-11) of the real mean.
  SUM32_REL  torch's float32 mean adds n non-negative terms in some order: whatever the order, the result is within (n - 1) u (1 + tiny)
             of the exact sum of those terms, plus one rounding for the division.  n u is used."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NEW_SYMBOLS = ("dir_depth_loss_workspace", "dir_depth_loss")
U = 2.0 ** -24
TERM_REL = 5.1 * U
PLANTED = [0.0, 0.05, 0.7, 1.0, 9.9, 9.95, 10.0, 12.0, -0.3]
SHAPES = [(1, 1, 1, 1), (1, 1, 3, 5), (3, 1, 7, 9), (5, 1, 57, 77), (2, 1, 114, 152)]


def tables():
    """name -> bucket weights as float32 [100], or None: the three the GPU tests use."""
    from dirhip.lds_nyud2 import get_bucket_weights
    return {"inverse_lds": np.asarray(get_bucket_weights("inverse", lds=True), dtype=np.float32),
            "sqrt_inv": np.asarray(get_bucket_weights("sqrt_inv"), dtype=np.float32), "none": None}


def make_case(shape, seed):
    """(pred, depth) float32 of ``shape``: depths uniform in [0.7, 10), then as many as fit of the planted values and of the float32
    neighbours of 0.7, 1.0 and 9.9 (where the float32 product decides the bucket) at seeded positions; the [1, 1, 1, 1] case takes 9.9."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    z = rng.uniform(0.7, 10.0, n).astype(np.float32)
    plant = [np.float32(v) for v in PLANTED]
    for v in (0.7, 1.0, 9.9):
        plant += [np.nextafter(np.float32(v), np.float32(-np.inf)), np.nextafter(np.float32(v), np.float32(np.inf))]
    if n == 1:
        plant = [np.float32(9.9)]
    pos = rng.permutation(n)[:len(plant)]
    z[pos] = np.asarray(plant[:len(pos)], dtype=np.float32)
    p = (z * rng.uniform(0.7, 1.45, n) + rng.normal(0, 0.05, n)).astype(np.float32)
    return p.reshape(shape), z.reshape(shape)


def bucket_of(z, mult=10.0, bucket_num=100):
    """clamp(int(z * mult), 0, bucket_num - 1): float32 product, truncated; NaN -> -1 (no bucket)."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(z, dtype=np.float32) * np.float32(mult)
        b = np.where(np.isnan(v), -1.0, np.clip(np.trunc(v), 0, bucket_num - 1))
    return b.astype(np.int64)


def restate(pred, depth, table, mult=10.0):
    """The kernel's arithmetic in numpy float32, one rounding per operation. Returns dict: w, t (terms), dx [shape of pred], sum64 (the
    float64 sum of the float32 terms, correctly rounded: math.fsum), loss (float32 of sum64 / n)."""
    p, z = np.asarray(pred, dtype=np.float32), np.asarray(depth, dtype=np.float32)
    n = p.size
    if table is None:
        w = np.ones(z.shape, np.float32)
    else:
        table = np.asarray(table, dtype=np.float32)
        b = bucket_of(z, mult, len(table))
        w = np.where(b >= 0, table[np.maximum(b, 0)], np.float32(1.0)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        d = p - z
        t = (d * d) * w
        inv_n = np.float32(1.0) / np.float32(n)
        dx = (inv_n * w) * (np.float32(2.0) * d)
    assert t.dtype == np.float32 and dx.dtype == np.float32
    s = math.fsum(t.astype(np.float64).ravel().tolist()) if not np.isnan(t).any() else float("nan")
    return {"w": w, "t": t, "dx": dx, "sum64": s, "loss": np.float32(s / n)}


def exact_mean(pred, depth, w):
    """mean of ((p - z)^2) w with every operation in float64 on the float32 inputs (exact to ~1e-15 relative)."""
    p, z = np.asarray(pred, np.float64).ravel(), np.asarray(depth, np.float64).ravel()
    return math.fsum((((p - z) ** 2) * np.asarray(w, np.float64).ravel()).tolist()) / p.size


# ---- C-ABI -------------------------------------------------------------------------------------------------------------------------
def test_loss_entry_points_exported_declared_and_bound():
    from dirhip import _lib, ops
    header = open(os.path.join(ROOT, "include", "dir_hip.h")).read()
    declared = set(re.findall(r"\b(dir_[a-z0-9_]+)\s*\(", header))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(handle, name), name
    assert _lib.SIGNATURES["dir_depth_loss_workspace"] == (ctypes.c_size_t, [ctypes.c_longlong])
    res, args = _lib.SIGNATURES["dir_depth_loss"]
    assert res is ctypes.c_int and len(args) == 11 and args[2] is ctypes.c_longlong and args[3] is ctypes.c_float and args[9] is ctypes.c_size_t
    assert "#define DIR_ABI_VERSION 4" in header and _lib.lib().dir_abi_version() == _lib.ABI_VERSION == 4
    assert "train.py:200" in header and "loaddata.py:57-69" in header
    assert callable(ops.depth_loss)


def test_loss_argument_errors_without_gpu():
    from dirhip import _lib
    L = _lib.lib()
    einval, eunsup = -1, -2
    assert L.dir_depth_loss_workspace(-1) == 0 and L.dir_depth_loss_workspace(0) == 0
    ws = L.dir_depth_loss_workspace(34656)
    assert ws > 0 and ws % 8 == 0
    assert L.dir_depth_loss_workspace(1) > 0
    assert L.dir_depth_loss_workspace(10 ** 9) == L.dir_depth_loss_workspace(2 * 10 ** 9) <= 1 << 16      # the grid is capped
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = L.dir_depth_loss
    assert call(None, None, 4, 10.0, None, 0, None, None, None, 0, None) == einval
    assert call(None, p, 4, 10.0, p, 100, p, p, p, 1 << 15, None) == einval                    # no prediction
    assert call(p, None, 4, 10.0, p, 100, p, p, p, 1 << 15, None) == einval                    # no depth
    assert call(p, p, 4, 10.0, p, 100, None, p, p, 1 << 15, None) == einval                    # no loss
    assert call(p, p, 0, 10.0, p, 100, p, p, p, 1 << 15, None) == einval
    assert call(p, p, -5, 10.0, p, 100, p, p, p, 1 << 15, None) == einval
    assert call(p, p, 4, 10.0, p, 0, p, p, p, 1 << 15, None) == einval                         # a table of no buckets
    assert call(p, p, 4, 10.0, p, 100, p, p, None, 0, None) == einval                          # no workspace
    assert call(p, p, 34656, 10.0, p, 100, p, p, p, ws - 1, None) == einval                    # workspace one byte short
    assert call(p, p, 4, 10.0, p, 257, p, p, p, 1 << 15, None) == eunsup                       # beyond the LDS table
    assert call(p, p, 2_100_000_001, 10.0, p, 100, p, p, p, 1 << 15, None) == eunsup           # 32-bit pixel indices


# ---- the restatement against torch on the CPU ------------------------------------------------------------------------------------------
def test_bucket_rule_by_hand():
    from dirhip.lds_nyud2 import get_bin_idx
    z = np.array(PLANTED + [np.inf, np.nan, 3.0e9], np.float32)
    assert bucket_of(z).tolist() == [0, 0, 7, 10, 99, 99, 99, 99, 0, 99, -1, 99]
    for v in (0.7, 1.0, 9.9):                                  # the float32 product decides: 0.7f * 10 rounds up to 7, its lower neighbour does not
        lo, hi = np.nextafter(np.float32(v), np.float32(-np.inf)), np.nextafter(np.float32(v), np.float32(np.inf))
        for x in (lo, np.float32(v), hi):
            assert bucket_of(x) == get_bin_idx(x) == min(int(np.float32(x) * np.float32(10)), 99)
    assert bucket_of(np.nextafter(np.float32(0.7), np.float32(-np.inf))) == 6 and bucket_of(np.float32(0.7)) == 7
    tab = np.arange(1, 101, dtype=np.float32)
    r = restate(np.array([2.0, 1.0, 5.0], np.float32), np.array([1.5, np.nan, -0.3], np.float32), tab)
    assert r["w"].tolist() == [16.0, 1.0, 1.0]                                                   # NaN depth: weight 1; negative: bucket 0
    assert r["t"][0] == 4.0 and np.isnan(r["t"][1]) and np.isnan(r["loss"]) and np.isnan(r["dx"][1])
    assert r["dx"][0] == (np.float32(1) / np.float32(3)) * np.float32(16)                        # ((1/3) * 16) * (2 * 0.5)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("tname", ["inverse_lds", "sqrt_inv", "none"])
def test_restatement_against_torch_cpu(shape, tname):
    """Terms and gradient bit-equal to torch's CPU kernels and autograd (mean backward -> mul backward -> pow backward, i.e.
    ((1 / n) * w) * (2 * d)); the float32 mean within SUM32_REL; the restated loss within TERM_REL of the float64 value."""
    table = tables()[tname]
    pred, depth = make_case(shape, 11 + len(shape) + shape[2])
    r = restate(pred, depth, table)
    n = pred.size
    o = torch.tensor(pred, requires_grad=True)
    d, w = torch.tensor(depth), torch.tensor(r["w"])
    terms = ((o - d) ** 2) * w
    loss = torch.mean(terms)
    loss.backward()
    assert np.array_equal(terms.detach().numpy(), r["t"])
    assert np.array_equal(o.grad.numpy(), r["dx"]), "torch's autograd order differs from ((1/n) * w) * (2 * d)"
    mean64 = r["sum64"] / n
    print(shape, tname, "torch f32 mean", loss.item(), "restated", float(r["loss"]), "float64", mean64)
    assert abs(loss.item() - mean64) <= (n + 1) * U * mean64
    assert abs(float(r["loss"]) - mean64) <= U * mean64                                          # one rounding
    exact = exact_mean(pred, depth, r["w"])
    assert abs(float(r["loss"]) - exact) <= TERM_REL * exact
    if table is not None:                                      # the weight map is PixelWeights' rule: table[clamp(int(z * 10), 0, 99)]
        assert np.array_equal(r["w"], table[bucket_of(depth)])
        assert len(np.unique(bucket_of(depth))) >= min(n, 4) or n < 4


# ---- Python surface ---------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused_and_surface():
    from dirhip._lib import DirHipError
    from dirhip.loss_nyud2 import weighted_depth_mse_loss
    from dirhip.lds_nyud2 import PixelWeights, get_bucket_weights
    x = torch.ones(1, 1, 3, 5)
    with pytest.raises(DirHipError, match="no CPU fallback"):
        weighted_depth_mse_loss(x, x)
    with pytest.raises(DirHipError, match="no CPU fallback"):
        weighted_depth_mse_loss(x, x, get_bucket_weights("sqrt_inv"))
    with pytest.raises(DirHipError, match="no CPU fallback"):
        PixelWeights(get_bucket_weights("inverse", lds=True)).loss(x, x)
    with pytest.raises(DirHipError, match="no CPU fallback"):
        PixelWeights(None).loss(x, x)
    with pytest.raises(TypeError):
        weighted_depth_mse_loss(np.ones(4, np.float32), x)


def test_dropin_loaddata_exports():
    import importlib.util
    import sys
    from conftest import PKG
    path = os.path.join(PKG, "nyud2-dir")
    saved_path, saved_mods = list(sys.path), {n: sys.modules.get(n) for n in ("loaddata", "_path")}
    sys.path.insert(0, path)
    try:
        for n in saved_mods:
            sys.modules.pop(n, None)
        spec = importlib.util.spec_from_file_location("loaddata", os.path.join(path, "loaddata.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        from dirhip.lds_nyud2 import PixelWeights
        from dirhip.loss_nyud2 import weighted_depth_mse_loss
        assert mod.weighted_depth_mse_loss is weighted_depth_mse_loss and mod.PixelWeights is PixelWeights
        assert callable(mod.PixelWeights.loss)
    finally:
        sys.path[:] = saved_path
        for n, old in saved_mods.items():
            if old is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = old
