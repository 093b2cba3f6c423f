"""CPU-side tests of the NYUD2-DIR evaluator: the float64 restatement against the dicts recorded from the reference's own ``Evaluator``,
its bilinear formula against torch's CPU ``F.interpolate``, the two C-ABI entry points (declared, exported, bound; argument errors
without a GPU), the ``Evaluator`` surface and the drop-in ``nyud2-dir/util.py``."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

import nyud2_eval_reference as R
from conftest import GOLDEN, PKG, ROOT

NEW_SYMBOLS = ("dir_depth_eval_workspace", "dir_depth_eval_accumulate")
REL_GOLDEN = 5e-7
BILINEAR_REL = 1e-6


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "nyud2_eval_ref.npz"))


def _rows(d, keys):
    return np.array([[float(d[s][k]) for k in keys] for s in ("overall", "many", "medium", "few")])


def test_restatement_matches_reference_goldens(g):
    """The reference sums float32 terms in float32 (torch.sum) and divides in float32; the restatement sums the same terms in float64.
    Measured here on the four golden cases (torch 2.10 CPU), max over metrics and shot groups of |reference - restatement| / |reference|:
    up 1.17e-7 (own bilinear) / 1.22e-7 (torch's upsampled map), up2 1.20e-7 / 1.24e-7, flat 8.9e-8, nan 6.0e-8 -> 1.25e-7.
    Bar: 4 x that = 5e-7 (torch's float32 summation order may change between builds). NUM and, where the per-pixel inputs are
    identical (flat, nan, and the upsampled cases fed torch's recorded map), the delta counts must match exactly."""
    keys = [str(k) for k in g["keys"]]
    num, deltas = keys.index("NUM"), [keys.index(k) for k in ("DELTA1", "DELTA2", "DELTA3")]
    cont = [keys.index(k) for k in ("MSE", "RMSE", "ABS_REL", "LG10", "MAE")]
    worst = 0.0
    for case in ("up", "up2", "flat"):
        depth = g[case + "_depth"]
        mask = g[case + "_mask"] if case + "_mask" in g else None
        sources = [("recorded", g[case + "_pred"] if case == "flat" else g[case + "_out"])]
        if case != "flat":
            sources.append(("own bilinear", R.bilinear_align_corners(g[case + "_pred"], *depth.shape[1:])))
        for src, p in sources:
            got, ref = _rows(R.shot_dict(R.table(p, depth, mask)["table"]), keys), g[case + "_dict"]
            assert np.array_equal(got[:, num], ref[:, num]), (case, src)
            cnt_got, cnt_ref = np.rint(got[:, deltas] * got[:, [num]]), np.rint(ref[:, deltas] * ref[:, [num]])
            if src == "recorded":
                assert np.array_equal(cnt_got, cnt_ref), (case, src)
            else:
                cap = R.delta_flip_cap(p, depth, BILINEAR_REL)
                assert cap < 1e-3 * depth.size, (case, cap)                       # the seeded inputs keep the cap below 0.1 % of the pixels
                assert np.all(np.abs(cnt_got - cnt_ref) <= cap), (case, cap)
            rel = (np.abs(got[:, cont] - ref[:, cont]) / np.abs(ref[:, cont])).max()
            print(case, src, "max relative difference", rel)
            worst = max(worst, rel)
    m, ref = R.metrics(R.table(g["nan_pred"], g["nan_depth"])["table"].sum(axis=0)), g["nan_dict"]
    assert m["NUM"] == int(ref[num]) == int((~np.isnan(g["nan_depth"])).sum())
    for i in deltas:
        assert round(m[keys[i]] * m["NUM"]) == round(ref[i] * ref[num])
    worst = max(worst, max(abs(m[keys[i]] - ref[i]) / abs(ref[i]) for i in cont))
    print("worst", worst)
    assert worst <= REL_GOLDEN
    # every shot group of the golden scenes is populated, buckets 0-6 and the clamped bucket 99 included
    tab = R.table(R.bilinear_align_corners(g["up_pred"], 48, 64), g["up_depth"], g["up_mask"])["table"]
    assert tab[:7, 7].sum() > 0 and tab[99, 7] > 0 and tab[7:9, 7].sum() > 0 and tab[9:50, 7].sum() > 0


def test_bilinear_restatement_against_torch_cpu(g):
    """The kernel's formula (source index i * ((in - 1) / (out - 1)) in float32, hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11)) is
    kept as written; it is not bit-equal to torch's CPU kernel. Measured here against F.interpolate(bilinear, align_corners=True), torch
    2.10 CPU: 12 x 16 -> 48 x 64: 39 % of the elements differ, at most 3 ulp (2.4e-7 relative); 7 x 9 -> 31 x 45: 33 %, 2 ulp;
    114 x 152 -> 480 x 640: 28 %, 3 ulp. (Fused multiply-adds or the other axis first do not remove the difference.) The golden comparisons cap the
    delta counts with BILINEAR_REL = 1e-6; that cap is valid while the two maps agree to BILINEAR_REL / 2 relatively (the ratio to the depth
    then moves by at most that plus one rounding, 2^-24), which is what is asserted here: about twice the measured difference."""
    import torch.nn.functional as F
    rng = np.random.default_rng(0)
    cases = [(g["up_pred"], 48, 64), (g["up2_pred"], 31, 45), (rng.uniform(0.3, 9.5, (2, 114, 152)).astype(np.float32), 480, 640),
             (rng.uniform(0.3, 9.5, (1, 5, 64)).astype(np.float32), 5, 200)]
    for pred, H, W in cases:
        want = F.interpolate(torch.tensor(pred)[:, None], size=(H, W), mode="bilinear", align_corners=True)[:, 0].numpy()
        got = R.bilinear_align_corners(pred, H, W)
        ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want))
        print(pred.shape, (H, W), "differ", (got != want).mean(), "max ulp", ulps.max())
        assert (np.abs(got.astype(np.float64) - want) / np.abs(want)).max() <= BILINEAR_REL / 2
        assert np.array_equal(got[:, 0, 0], pred[:, 0, 0]) and np.array_equal(got[:, -1, -1], pred[:, -1, -1])
        if (H, W) != pred.shape[1:]:                            # the emulated defect of the GPU tests is torch's other mode, and a different map
            other = F.interpolate(torch.tensor(pred)[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0].numpy()
            half = R.bilinear_align_corners(pred, H, W, align_corners=False)
            assert np.allclose(half, other, rtol=1e-4, atol=1e-5) and not np.allclose(half, want, rtol=1e-3)
    same = R.bilinear_align_corners(g["up_pred"], 12, 16)
    assert np.array_equal(same, g["up_pred"])


def test_restatement_terms_by_hand():
    t = R.table(np.array([2.5, 1.0, 3.0], np.float32), np.array([2.0, 2.0, np.nan], np.float32))
    tab = t["table"]
    assert tab[20].tolist()[4:] == [1.0, 1.0, 1.0, 2.0] and tab.sum() == tab[20].sum()        # 2.5 / 2 = 1.25 counts; 2 / 1 = 2 passes none
    assert tab[20, 0] == 0.25 + 1.0 and tab[20, 1] == 1.5 and tab[20, 2] == 0.75
    assert abs(tab[20, 3] - (np.log10(1.25) + np.log10(2.0))) < 1e-6
    assert R.bucket_of(np.array([0.0, 0.05, 0.7, 9.99, 10.0, 55.0, -1.0, np.inf], np.float32)).tolist() == [0, 0, 7, 99, 99, 99, 0, 99]
    from dirhip.eval_nyud2 import Evaluator
    for x in (0.05, 0.7, 0.75, 3.14159, 9.95, 12.0):
        assert Evaluator.get_bin_idx(np.float32(x)) == R.bucket_of(np.float32(x))


def test_eval_entry_points_exported_declared_and_bound():
    from dirhip import _lib
    header = open(os.path.join(ROOT, "include", "dir_hip.h")).read()
    declared = set(re.findall(r"\b(dir_[a-z0-9_]+)\s*\(", header))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(handle, name), name
    assert _lib.SIGNATURES["dir_depth_eval_workspace"] == (ctypes.c_size_t, [ctypes.c_longlong, ctypes.c_int])
    res, args = _lib.SIGNATURES["dir_depth_eval_accumulate"]
    assert res is ctypes.c_int and len(args) == 14 and args[8] is ctypes.c_float and args[12] is ctypes.c_size_t
    assert "#define DIR_ABI_VERSION 4" in header
    assert _lib.lib().dir_abi_version() == _lib.ABI_VERSION == 4
    from dirhip import ops
    assert callable(ops.depth_eval_accumulate)


def test_eval_argument_errors_without_gpu():
    from dirhip import _lib
    L = _lib.lib()
    einval, eunsup, ework = -1, -2, -3
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ws100 = L.dir_depth_eval_workspace(480 * 640, 100)
    assert ws100 > 0 and ws100 % (100 * 8 * 8) == 0
    assert L.dir_depth_eval_workspace(0, 100) == 0 and L.dir_depth_eval_workspace(1000, 257) == 0
    assert L.dir_depth_eval_workspace(1, 100) == 100 * 8 * 8                                   # one workgroup
    assert L.dir_depth_eval_workspace(10 ** 9, 100) == L.dir_depth_eval_workspace(2 * 10 ** 9, 100)   # the grid is capped
    call = L.dir_depth_eval_accumulate
    assert call(None, None, None, 0, 4, 4, 8, 8, 10.0, 100, None, None, 0, None) == 0          # empty batch: nothing to launch
    assert call(None, p, None, 1, 4, 4, 8, 8, 10.0, 100, p, p, 1 << 20, None) == einval       # no prediction
    assert call(p, None, None, 1, 4, 4, 8, 8, 10.0, 100, p, p, 1 << 20, None) == einval       # no depth
    assert call(p, p, None, 1, 4, 4, 8, 8, 10.0, 100, None, p, 1 << 20, None) == einval       # no table
    assert call(p, p, None, 1, 4, 4, 8, 8, 10.0, 100, p, None, 0, None) == einval             # no workspace
    for bad in ((0, 4, 8, 8), (4, 0, 8, 8), (4, 4, 0, 8), (4, 4, 8, -1)):
        assert call(p, p, None, 1, *bad, 10.0, 100, p, p, 1 << 20, None) == einval
    assert call(p, p, None, -1, 4, 4, 8, 8, 10.0, 100, p, p, 1 << 20, None) == einval
    assert call(p, p, None, 1, 4, 4, 8, 8, 10.0, 0, p, p, 1 << 20, None) == einval
    assert call(p, p, None, 1, 4, 4, 8, 8, 0.0, 100, p, p, 1 << 20, None) == einval
    assert call(p, p, None, 1, 4, 4, 8, 8, float("nan"), 100, p, p, 1 << 20, None) == einval
    assert call(p, p, None, 1, 4, 4, 8, 8, 10.0, 257, p, p, 1 << 20, None) == eunsup           # beyond the LDS layout
    assert call(p, p, None, 40000, 4, 4, 480, 640, 10.0, 100, p, p, 1 << 30, None) == eunsup   # > 2.1e9 pixels: 32-bit indices
    assert call(p, p, None, 1, 4, 4, 8, 8, 10.0, 100, p, p, 100 * 8 * 8 - 1, None) == ework    # workspace one byte short
    odd = ctypes.c_void_p(p.value + 2)
    assert call(odd, p, None, 1, 4, 4, 8, 8, 10.0, 100, p, p, 1 << 20, None) == einval         # misaligned float pointer


def test_evaluator_surface_and_cpu_refusal():
    from dirhip._lib import DirHipError
    from dirhip.eval_nyud2 import Evaluator
    ev = Evaluator()
    for name in ("__call__", "update", "evaluate_shot", "reset", "get_bin_idx", "evaluate", "merge_across_ranks"):
        assert callable(getattr(ev, name)), name
    assert ev.shot_idx == R.SHOT_IDX
    allidx = sorted(i for v in ev.shot_idx.values() for i in v)
    assert allidx == list(range(100))                                                           # the three groups partition 0..99
    assert (len(ev.shot_idx["many"]), len(ev.shot_idx["medium"]), len(ev.shot_idx["few"])) == (39, 15, 46)
    x = torch.ones(8)
    with pytest.raises(DirHipError, match="no CPU fallback"):
        ev(x, x)
    with pytest.raises(DirHipError, match="no CPU fallback"):
        ev.update(torch.ones(1, 1, 2, 2), torch.ones(1, 1, 4, 4))
    with pytest.raises(DirHipError, match="no CPU fallback"):
        Evaluator.evaluate(x, x)
    with pytest.raises(TypeError):
        ev(np.ones(8, np.float32), x)
    empty = ev.evaluate_shot()                                                                  # nothing accumulated: the reference's zeros
    assert set(empty) == {"overall", "many", "medium", "few"}
    assert all(v == 0 for s in empty.values() for v in s.values()) and set(empty["few"]) == set(R.metrics(np.zeros(8)))
    ev.reset()
    ev.merge_across_ranks()                                                                     # no process group: a no-op


def test_dropin_util_exports():
    path = os.path.join(PKG, "nyud2-dir")
    saved_path, saved_mods = list(sys.path), {n: sys.modules.get(n) for n in ("util", "_path")}
    sys.path.insert(0, path)
    try:
        for n in saved_mods:
            sys.modules.pop(n, None)
        spec = importlib.util.spec_from_file_location("util", os.path.join(path, "util.py"))
        util = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(util)
        from dirhip.eval_nyud2 import Evaluator
        from dirhip.utils import get_lds_kernel_window, query_yes_no
        assert util.Evaluator is Evaluator and util.get_lds_kernel_window is get_lds_kernel_window and util.query_yes_no is query_yes_no
        assert callable(util.calibrate_mean_var)
    finally:
        sys.path[:] = saved_path
        for n, old in saved_mods.items():
            if old is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = old
