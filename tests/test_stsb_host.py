"""CPU-side tests of the STS-B-DIR pieces: the numpy / Python-int restatement of the evaluator against the numbers recorded from the
reference's own ``STSShotAverage`` (tests/golden/stsb_eval_ref.npz), the binning and shot groups, the LDS weights over histogram buckets
(bit for bit against ``tasks.load_tsv``'s recorded output), the new C-ABI entry points (declared, exported, bound; argument errors
without a GPU) and the signatures of the ``sts-b-dir/loss.py`` drop-in."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import stsb_eval_reference as R
from conftest import GOLDEN, PKG, ROOT

NEW_SYMBOLS = ("dir_stsb_eval_workspace", "dir_stsb_eval", "dir_lds_weights_binned")
CASES = ("dev", "sub65", "nomed")
ULP = 2.0 ** -52
# Relative bars per metric against the reference's recorded dicts: 4 x the largest |restatement - reference| / |reference| measured in
# test_restatement_matches_reference_goldens over the three cases (the convention of test_age_eval_host.py):
#   mse 3.96e-15, gmean 9.16e-16, pearsonr 1.65e-15, spearmanr 1.39e-16 (exact integer sums against scipy's float ranks), l1 0.0.
# l1 measured 0.0 (np.mean and the restatement's np.sum / n add the same numbers in the same pairwise order), so its bar is a floor
# instead: 16 ulps. Any two correct float64 evaluations of a mean of ~1000 positive terms may differ by that much: a tree-shaped sum is
# about 15 roundings deep on either side (numpy: 8 lanes + log2(1000 / 8) pair levels; the device: 6 butterfly levels, 4 waves, 4
# workgroups, 3 groups, the division), each at most 2^-53 of a positive partial sum, i.e. 30 * 2^-53 = 15 ulps between the two.
REL_BAR = {"mse": 4 * 3.96e-15, "l1": 16 * ULP, "gmean": 4 * 9.16e-16, "pearsonr": 4 * 1.65e-15, "spearmanr": 4 * 1.39e-16}


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "stsb_eval_ref.npz"))


def assert_rows_match(got, ref, what):
    """[4, 6] rows (R.KEYS columns) against the reference's recorded rows at REL_BAR; num_samples exact. Returns the worst ratios."""
    worst = {}
    assert np.array_equal(got[:, 5], ref[:, 5]), (what, got[:, 5], ref[:, 5])
    for c, key in enumerate(R.KEYS[:5]):
        diff = np.abs(got[:, c] - ref[:, c])
        rel = np.where(ref[:, c] != 0, diff / np.where(ref[:, c] != 0, np.abs(ref[:, c]), 1.0), diff)
        worst[key] = float(rel.max())
        assert (rel <= REL_BAR[key]).all(), (what, key, rel, REL_BAR[key])
    return worst


def test_restatement_matches_reference_goldens(g):
    """The restatement forms the reference's own float64 terms; it differs from numpy / scipy in the order of the sums, in the
    shifted-raw-moment form of Pearson and in the exact integer form of Spearman. The measured figures are beside REL_BAR."""
    for case in CASES:
        got = R.as_rows(R.evaluate(g[f"{case}_pred"], g[f"{case}_label"]))
        worst = assert_rows_match(got, g[f"{case}_dict"], case)
        print(case, {k: f"{v:.3e}" for k, v in worst.items()})
    assert g["dev_dict"][3, 5] == 1000 and g["sub65_dict"][3, 5] == 65
    assert g["nomed_dict"][1].tolist() == [0.0] * 6                              # the empty group: every metric 0
    assert len(np.unique(g["dev_label"])) == 75                                  # the heavily tied labels the issue speaks of


def test_restatement_edge_cases_follow_the_reference_rules():
    lab = np.array([0.0, 0.05, 0.2, 0.25, 0.3], np.float32)                      # bins 0, 0, 2, 2, 3: many, many, medium, medium, few
    assert R.groups(lab).tolist() == [0, 0, 1, 1, 2]
    pred = np.array([0.1, 0.1, 0.04, 0.05, 0.5], np.float32)
    d = R.evaluate(pred, lab)
    assert d["few"]["num_samples"] == 1 and d["few"]["pearsonr"] == 0. and d["few"]["spearmanr"] == 0.      # util.py:160-162
    assert np.isnan(d["many"]["pearsonr"]) and np.isnan(d["many"]["spearmanr"])                             # constant predictions: scipy's nan
    assert d["medium"]["spearmanr"] == 1.0
    exact = R.evaluate(np.array([0.5], np.float32), np.array([2.5], np.float32))
    assert exact["overall"]["gmean"] == pytest.approx(1e-10, rel=1e-12) and exact["overall"]["mse"] == 0.   # util.py:153-156
    assert R.evaluate(pred, lab, ["mse"])["overall"].keys() == {"mse", "num_samples"}


def test_host_half_of_the_product_equals_the_restatement(g):
    from dirhip import eval_stsb as E
    assert E.MOMENT_COLUMNS == R.MOMENT_COLUMNS and E.ROWS == R.ROWS
    for case in CASES:
        m, r = R.moment_table(g[f"{case}_pred"], g[f"{case}_label"])["table"], R.rank_table(g[f"{case}_pred"], g[f"{case}_label"])
        assert E.metrics_of(m, r, R.ALL_METRICS) == R.metrics(m, r)
    const = R.moment_table(np.full(4, 0.3, np.float32), np.array([1, 2, 3, 4], np.float32))["table"]
    ranks = R.rank_table(np.full(4, 0.3, np.float32), np.array([1, 2, 3, 4], np.float32))
    assert np.isnan(E.metrics_of(const, ranks, R.ALL_METRICS)["overall"]["pearsonr"])


@pytest.mark.needs_reference
def test_binning_and_groups_equal_the_reference():
    """Every float32 edge value, its two float32 neighbours, 0.0 and 5.0 against the reference's ``get_bin_idx``; all 50 bins against
    its ``bin2shot`` rule (util.py:130-136)."""
    from oracle import refshim
    ref = refshim.load_stsb().util.STSShotAverage(metric=[])
    e = R.edges()
    assert e.dtype == np.float32 and e.shape == (51,)
    probes = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf)), np.array([0.0, 5.0], np.float32)])
    probes = probes[(probes >= 0) & (probes <= 5)].astype(np.float32)
    assert probes.size == 51 * 3
    want = [int(ref._get_bin_idx(l)) for l in probes]
    assert R.bin_of(probes).tolist() == want
    shot = {'many': 0, 'medium': 1}
    want_group = [next((v for k, v in shot.items() if b in ref._shot_idx[k]), 2) for b in range(50)]
    assert R.group_of_bin().tolist() == want_group
    from dirhip.eval_stsb import STSShotAverage
    mine = STSShotAverage(metric=[])
    assert mine._shot_idx == ref._shot_idx and mine._num_bins == ref._num_bins
    assert np.array_equal(mine._edges_host, e) and mine._group_host.tolist() == want_group
    assert [mine._get_bin_idx(l) for l in probes] == want


def test_binning_literal_expectations():
    """The same rule without the reference: edges are float32(linspace(0, 5, 51)); 0.3 as float32 lies ABOVE the float32 edge 0.3."""
    e = R.edges()
    assert np.array_equal(e, np.linspace(0, 5, 51).astype(np.float32))
    assert R.bin_of(np.array([0.0, 0.099, 0.1, 4.9, 4.95, 5.0, 2.5], np.float32)).tolist() == [0, 0, 1, 49, 49, 49, 25]
    assert R.bin_of(e).tolist() == list(range(50)) + [49]
    assert R.bin_of(np.nextafter(e[1:], np.float32(0))).tolist() == list(range(50))
    for bad in (-0.001, 5.001, np.nan):
        with pytest.raises(ValueError):
            R.bin_of(np.array([bad], np.float32))
    assert (R.group_of_bin() == 0).sum() == 22 and (R.group_of_bin() == 1).sum() == 7 and (R.group_of_bin() == 2).sum() == 21


LDS_KW = {"none": {}, "gaussian": dict(lds=True, lds_kernel="gaussian", lds_ks=5, lds_sigma=2),
          "triang": dict(lds=True, lds_kernel="triang", lds_ks=9, lds_sigma=2), "laplace": dict(lds=True, lds_kernel="laplace", lds_ks=5, lds_sigma=2)}


@pytest.mark.parametrize("reweight", ["inverse", "sqrt_inv"])
@pytest.mark.parametrize("name", list(LDS_KW))
def test_weights_bit_equal_to_the_reference(reweight, name):
    from dirhip.lds_stsb import prepare_weights
    w = np.load(os.path.join(GOLDEN, "stsb_lds_weights.npz"))
    got = prepare_weights(list(w["labels"]), reweight, **LDS_KW[name])
    assert len(got) == 5249 and all(type(x) is np.float32 for x in got[:8])
    assert np.array_equal(np.array(got, np.float32).view(np.uint32), w[f"w_{reweight}_{name}"].view(np.uint32))


@pytest.mark.parametrize("n", [1, 7, 8, 129, 8193])
def test_weights_bit_equal_at_the_pairwise_sum_seams(n):
    """numpy's float32 sum changes shape at 8 (unrolled lanes), 128 (pairwise split) and 8192 (buffer chunks)."""
    from dirhip.lds_stsb import prepare_weights
    from dirhip.utils import get_lds_kernel_window
    rng = np.random.default_rng(n)
    labels = np.round(rng.beta(2, 1.3, n) * 5, 2).astype(np.float32)
    labels[0] = 5.0
    for reweight in ("inverse", "sqrt_inv"):
        for name, kw in LDS_KW.items():
            window = get_lds_kernel_window(kw["lds_kernel"], kw["lds_ks"], kw["lds_sigma"]) if kw else None
            want = R.lds_weights(labels, reweight, bool(kw), window)
            with np.errstate(all="ignore"):
                got = np.array(prepare_weights(labels, reweight, **kw), np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, reweight, name)


def test_weights_surface():
    from dirhip._lib import DirHipError
    from dirhip.lds_stsb import prepare_weights
    labels = np.array([0.0, 1.2, 5.0], np.float32)
    assert prepare_weights(labels, "none") is None
    with pytest.raises(AssertionError):
        prepare_weights(labels, "none", lds=True)
    with pytest.raises(AssertionError):
        prepare_weights(labels, "cube_root")
    for bad in (5.5, -0.1, np.nan):
        with pytest.raises(DirHipError):
            prepare_weights(np.array([1.0, bad], np.float32), "inverse")
    sig = inspect.signature(prepare_weights)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == [
        ("reweight", inspect.Parameter.empty), ("lds", False), ("lds_kernel", "gaussian"), ("lds_ks", 5), ("lds_sigma", 2), ("bucket_num", 50)]


def test_stsb_entry_points_exported_declared_and_bound():
    from dirhip import _lib, ops
    header = open(os.path.join(ROOT, "include", "dir_hip.h")).read()
    declared = set(re.findall(r"\b(dir_[a-z0-9_]+)\s*\(", header))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(handle, name), name
    c = ctypes
    assert _lib.SIGNATURES["dir_stsb_eval_workspace"] == (c.c_size_t, [c.c_longlong, c.c_int])
    assert _lib.SIGNATURES["dir_stsb_eval"] == (c.c_int, [c.c_void_p, c.c_void_p, c.c_longlong, c.c_void_p, c.c_int, c.c_void_p, c.c_void_p,
                                                          c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p])
    assert _lib.SIGNATURES["dir_lds_weights_binned"] == (c.c_int, [c.c_void_p, c.c_int64, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_void_p,
                                                                   c.c_int, c.c_void_p])
    assert "#define DIR_ABI_VERSION 4" in header and _lib.lib().dir_abi_version() == _lib.ABI_VERSION == 4
    for ref_lines in ("sts-b-dir/util.py:101-172", "sts-b-dir/tasks.py:44-73"):          # each entry cites the reference lines it implements
        assert ref_lines in header
    assert callable(ops.stsb_eval) and callable(ops.lds_weights_binned)


def test_stsb_argument_errors_without_gpu():
    from dirhip import _lib
    L = _lib.lib()
    einval, eunsup, ework = -1, -2, -3
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    per_block = 32 * 8 + 20 * 8
    ws = L.dir_stsb_eval_workspace
    assert ws(1, 50) == 256 + per_block and ws(256, 50) == 256 + per_block and ws(257, 50) == 512 + 2 * per_block
    assert ws(65536, 50) == 65536 + 256 * per_block and ws(1000, 256) == 1024 + 4 * per_block
    assert ws(0, 50) == 0 and ws(-1, 50) == 0 and ws(65537, 50) == 0 and ws(1000, 0) == 0 and ws(1000, 257) == 0
    call = L.dir_stsb_eval
    big = 1 << 20
    assert call(p, p, 0, p, 50, p, p, p, p, big, None) == einval                               # n = 0
    assert call(p, p, -5, p, 50, p, p, p, p, big, None) == einval
    assert call(p, p, 10, p, 0, p, p, p, p, big, None) == einval                               # num_bins = 0
    assert call(p, p, 65537, p, 50, p, p, p, p, 1 << 30, None) == eunsup                       # beyond the cap
    assert call(p, p, 10, p, 257, p, p, p, p, big, None) == eunsup                             # beyond the LDS edge table
    for hole in range(9):                                                                      # every pointer but the stream
        args = [p, p, 10, p, 50, p, p, p, p, big, None]
        if hole in (2, 4):
            continue
        args[hole] = None
        assert call(*args) == einval, hole
    assert call(p, p, 10, p, 50, p, p, p, p, 256 + per_block - 1, None) == ework               # workspace one byte short
    odd = ctypes.c_void_p(p.value + 2)
    assert call(odd, p, 10, p, 50, p, p, p, p, big, None) == einval                            # misaligned float pointer
    assert call(p, p, 10, p, 50, p, ctypes.c_void_p(p.value + 4), p, p, big, None) == einval   # misaligned moment table
    # the host weights entry
    lab = (ctypes.c_float * 4)(0.0, 1.0, 2.0, 5.0)
    e = R.edges()
    ep = e.ctypes.data_as(ctypes.c_void_p)
    out = (ctypes.c_float * 4)()
    win = (ctypes.c_double * 4)(1, 1, 1, 1)
    w = L.dir_lds_weights_binned
    assert w(lab, 4, ep, 50, 2, 0, None, 0, out) == 0 and abs(sum(out) - 4.0) < 1e-5
    assert w(None, 4, ep, 50, 2, 0, None, 0, out) == einval and w(lab, 4, None, 50, 2, 0, None, 0, out) == einval
    assert w(lab, 0, ep, 50, 2, 0, None, 0, out) == einval and w(lab, 4, ep, 0, 2, 0, None, 0, out) == einval
    assert w(lab, 4, ep, 50, 3, 0, None, 0, out) == einval                                     # unknown reweight
    assert w(lab, 4, ep, 50, 2, 1, win, 4, out) == einval and w(lab, 4, ep, 50, 2, 1, None, 5, out) == einval   # even ks, no window


def test_shot_average_surface_and_cpu_refusal():
    from dirhip._lib import DirHipError
    from dirhip.eval_stsb import STSShotAverage
    ev = STSShotAverage(metric=R.ALL_METRICS)
    assert list(inspect.signature(STSShotAverage.__init__).parameters) == ["self", "metric"]
    assert [(p.name, p.default) for p in inspect.signature(ev.get_metric).parameters.values()] == [("reset", False), ("type", None)]
    x = torch.ones(8)
    with pytest.raises(DirHipError, match="no CPU fallback"):
        ev(x, x)
    with pytest.raises(TypeError):
        ev(np.ones(8, np.float32), x)
    empty = ev.get_metric()                                                        # nothing appended: no kernel call, every metric 0
    assert set(empty) == set(R.ROWS) and all(v == {k: 0 for k in R.KEYS} for v in empty.values())
    assert ev.get_metric(type='overall') == {k: 0 for k in R.KEYS}
    ev.reset()
    assert "all-gather" in (__import__("dirhip.eval_stsb").eval_stsb.__doc__)      # sharding is out of scope and says why


def _load_flat(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


LOSS_SIGNATURES = {
    "weighted_mse_loss": [("inputs", None), ("targets", None), ("weights", None)],
    "weighted_l1_loss": [("inputs", None), ("targets", None), ("weights", None)],
    "weighted_huber_loss": [("inputs", None), ("targets", None), ("weights", None), ("beta", 0.5)],
    "weighted_focal_mse_loss": [("inputs", None), ("targets", None), ("weights", None), ("activate", "sigmoid"), ("beta", 20.), ("gamma", 1)],
    "weighted_focal_l1_loss": [("inputs", None), ("targets", None), ("weights", None), ("activate", "sigmoid"), ("beta", 20.), ("gamma", 1)],
}


def _signature(fn):
    return [(p.name, None if p.default is inspect.Parameter.empty else p.default) for p in inspect.signature(fn).parameters.values()]


def test_loss_dropin_signatures():
    """Names, parameter order and defaults of sts-b-dir/loss.py: a literal expectation, and the reference's own file when it is there."""
    from dirhip import loss_stsb
    import sys
    d = os.path.join(PKG, "sts-b-dir")
    sys.path.insert(0, d)
    try:
        saved = sys.modules.pop("_path", None)
        flat = _load_flat(os.path.join(d, "loss.py"), "stsb_dropin_loss")
        util = _load_flat(os.path.join(d, "util.py"), "stsb_dropin_util")
    finally:
        sys.path.remove(d)
        sys.modules.pop("_path", None)
        if saved is not None:
            sys.modules["_path"] = saved
    for name, want in LOSS_SIGNATURES.items():
        assert _signature(getattr(flat, name)) == want, name
        assert getattr(flat, name) is getattr(loss_stsb, name)
    from dirhip.eval_stsb import STSShotAverage
    from dirhip.utils import get_lds_kernel_window
    assert util.STSShotAverage is STSShotAverage and util.get_lds_kernel_window is get_lds_kernel_window and callable(util.calibrate_mean_var)
    from oracle import refshim
    if refshim.available("sts-b-dir"):
        ref = _load_flat(os.path.join(refshim.REFERENCE_ROOT, "sts-b-dir", "loss.py"), "stsb_reference_loss")
        names = sorted(n for n in dir(ref) if n.startswith("weighted_"))
        assert names == sorted(LOSS_SIGNATURES)
        for name in names:
            assert _signature(getattr(ref, name)) == _signature(getattr(flat, name)), name
