"""CPU-side tests of the balanced age evaluator: the float64 restatement against the numbers recorded from the reference's own
``validate`` / ``shot_metrics`` (tests/golden/validate.npz), the shot of every kind of label, the two C-ABI entry points (declared,
exported, bound; argument errors without a GPU), the ``ShotEvaluator`` surface and the ``--device_eval`` flag."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import age_eval_reference as R
from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ("dir_age_eval_workspace", "dir_age_eval_accumulate")
REL_GOLDEN = 9.4e-7        # 4 x the 2.35e-7 measured in test_restatement_matches_reference_goldens


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "validate.npz"))


def test_restatement_matches_reference_goldens(g):
    """The reference sums float32 errors in float32 (per-batch torch means, numpy sums per label) and its G-Mean takes a float32 log;
    the restatement sums the same float32 terms in float64 and takes a float64 log. Measured here on the three golden cases, max over
    MSE / L1 / G-Mean of |reference - restatement| / |reference|: case 0 overall 2.5e-8, shots 1.40e-7; case 1 overall 7.2e-8, shots
    2.35e-7; case 2 overall 2.5e-8, shots 6.3e-8 -> 2.35e-7. Bar: 4 x that (numpy's float32 summation order may change between builds)."""
    shots, num_labels = R.shot_of_rows(g["in_train_labels"])
    assert num_labels == int(g["in_train_labels"].max()) + 1
    worst = 0.0
    for ci in range(3):
        t = R.table(g[f"in_preds_{ci}"], g[f"in_labels_{ci}"], num_labels)
        res = R.results(t["table"], shots)
        tri, rows = R.golden_rows(res)
        ref_tri, ref_rows = g[f"ref_validate_{ci}"], g[f"ref_shot_{ci}"]
        rel_tri, rel_rows = np.abs(tri - ref_tri) / np.abs(ref_tri), np.abs(rows - ref_rows) / np.abs(ref_rows)
        print(f"case {ci}: overall max relative difference {rel_tri.max():.3e}, shots {rel_rows.max():.3e}")
        worst = max(worst, rel_tri.max(), rel_rows.max())
        assert res["overall"]["num"] == g[f"in_labels_{ci}"].size == sum(res[s]["num"] for s in R.SHOTS)
        assert t["table"][num_labels, 4] > 0                    # the goldens hold labels beyond the training range: the "other" row
    print("worst", worst)
    assert worst <= REL_GOLDEN


def _train_labels_with_counts(counts):
    return np.concatenate([np.full(c, l, dtype=np.float32) for l, c in counts.items()])


def test_shot_assignment_of_every_kind_of_label():
    """many: count > 100, low: count < 20, median otherwise — so 100 and 20 themselves are median; a label absent from the training
    set, a fractional, a negative and a too-large one all have training count 0 and are low (fractional / negative / too large share
    the "other" row). Checked against ``train_main.shot_metrics``, the reference's own per-label scan."""
    from dirhip.eval_age import ShotEvaluator
    from dirhip.train_main import shot_metrics
    counts = {0: 150, 3: 101, 4: 100, 5: 99, 7: 21, 8: 20, 9: 19, 12: 1, 30: 400}        # 1, 2, 6, 10, 11, 13..29 absent
    train = _train_labels_with_counts(counts)
    ev = ShotEvaluator(train)
    shots, num_labels = R.shot_of_rows(train)
    assert ev.num_labels == num_labels == 31 and np.array_equal(ev.shot_of_row, shots) and len(shots) == 32
    want = {0: "many", 3: "many", 4: "median", 5: "median", 7: "median", 8: "median", 9: "low", 12: "low", 30: "many", 6: "low", 31: "low"}
    for row, shot in want.items():
        assert ev.shot_of_row[row] == shot, (row, shot)
    thr = ShotEvaluator(train, many_shot_thr=99, low_shot_thr=21)
    assert thr.shot_of_row[4] == "many" and thr.shot_of_row[8] == "low" and thr.shot_of_row[7] == "median"
    labels = np.array([4, 4, 8, 9, 6, 25.5, -3, 31, 200, 0, 30, 30, 5, 3, -0.5, 7, 12], dtype=np.float32)
    assert R.row_of(labels, num_labels).tolist() == [4, 4, 8, 9, 6, 31, 31, 31, 31, 0, 30, 30, 5, 3, 31, 7, 12]
    assert R.row_of(np.array([np.nan, np.inf, 30.000002, 1e9], np.float32), num_labels).tolist() == [31] * 4
    rng = np.random.default_rng(0)
    preds = (labels + rng.normal(0, 3, labels.size)).astype(np.float32)
    t = R.table(preds, labels, num_labels)
    got = ev.metrics_of(t["table"])
    assert got == R.results(t["table"], shots)
    ref = shot_metrics(preds, labels, train)
    for s in R.SHOTS:
        for k in ("mse", "l1", "gmean"):
            assert abs(got[s][k] - ref[s][k]) <= REL_GOLDEN * abs(ref[s][k]), (s, k)
    assert (got["many"]["num"], got["median"]["num"], got["low"]["num"]) == (4, 5, 8) and got["overall"]["num"] == 17
    # one exact prediction: the G-Mean of its shot and of the whole set is 0, as scipy's gmean of a zero is
    preds[0] = labels[0]
    z = ev.metrics_of(R.table(preds, labels, num_labels)["table"])
    assert z["median"]["gmean"] == 0.0 and z["overall"]["gmean"] == 0.0 and z["many"]["gmean"] > 0
    # an empty shot is nan, as in shot_metrics
    only_many = ev.metrics_of(R.table(preds[9:12], labels[9:12], num_labels)["table"])
    assert only_many["many"]["num"] == 3 and all(np.isnan(only_many[s][k]) for s in ("median", "low") for k in ("mse", "l1", "gmean"))
    assert np.isnan(shot_metrics(preds[9:12], labels[9:12], train)["low"]["gmean"])
    # valid = 0 rows are in no sum
    keep = np.ones(labels.size, np.uint8)
    keep[[1, 5]] = 0
    assert np.array_equal(R.table(preds, labels, num_labels, keep)["table"], R.table(np.delete(preds, [1, 5]), np.delete(labels, [1, 5]), num_labels)["table"])


def test_age_entry_points_exported_declared_and_bound():
    from dirhip import _lib
    header = open(os.path.join(ROOT, "include", "dir_hip.h")).read()
    declared = set(re.findall(r"\b(dir_[a-z0-9_]+)\s*\(", header))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(handle, name), name
    assert _lib.SIGNATURES["dir_age_eval_workspace"] == (ctypes.c_size_t, [ctypes.c_longlong, ctypes.c_int])
    res, args = _lib.SIGNATURES["dir_age_eval_accumulate"]
    assert res is ctypes.c_int and len(args) == 9 and args[3] is ctypes.c_longlong and args[4] is ctypes.c_int and args[7] is ctypes.c_size_t
    assert "#define DIR_ABI_VERSION 4" in header
    assert _lib.lib().dir_abi_version() == _lib.ABI_VERSION == 4
    from dirhip import ops
    assert callable(ops.age_eval_accumulate)


def test_age_argument_errors_without_gpu():
    from dirhip import _lib
    L = _lib.lib()
    einval, eunsup, ework = -1, -2, -3
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    row = 5 * 8
    assert L.dir_age_eval_workspace(1, 101) == 102 * row                                       # one workgroup
    assert L.dir_age_eval_workspace(1019, 101) == 102 * row and L.dir_age_eval_workspace(1022, 101) == 2 * 102 * row   # 3 slots of lead-in
    assert L.dir_age_eval_workspace(0, 101) == 0 and L.dir_age_eval_workspace(1000, 256) == 0 and L.dir_age_eval_workspace(1000, 0) == 0
    assert L.dir_age_eval_workspace(1000, 255) == 256 * row
    assert L.dir_age_eval_workspace(10 ** 9, 101) == L.dir_age_eval_workspace(10 ** 12, 101) == 1024 * 102 * row   # the grid is capped
    call = L.dir_age_eval_accumulate
    assert call(None, None, None, 0, 101, None, None, 0, None) == 0                            # empty batch: no pointer is touched
    assert call(None, p, None, 1, 101, p, p, 1 << 20, None) == einval                          # no prediction
    assert call(p, None, None, 1, 101, p, p, 1 << 20, None) == einval                          # no label
    assert call(p, p, None, 1, 101, None, p, 1 << 20, None) == einval                          # no table
    assert call(p, p, None, 1, 101, p, None, 0, None) == einval                                # no workspace
    assert call(p, p, None, -1, 101, p, p, 1 << 20, None) == einval
    assert call(p, p, None, 1, 0, p, p, 1 << 20, None) == einval
    assert call(p, p, None, 1, 256, p, p, 1 << 20, None) == eunsup                             # 257 rows: beyond the LDS layout
    assert call(None, None, None, 0, 256, None, None, 0, None) == eunsup
    assert call(p, p, None, 1, 101, p, p, 102 * row - 1, None) == ework                        # workspace one byte short
    odd = ctypes.c_void_p(p.value + 2)
    assert call(odd, p, None, 1, 101, p, p, 1 << 20, None) == einval                           # misaligned float pointer
    assert call(p, p, None, 1, 101, ctypes.c_void_p(p.value + 4), p, 1 << 20, None) == einval  # misaligned table


def test_shot_evaluator_surface_and_cpu_refusal():
    from dirhip._lib import DirHipError
    from dirhip.eval_age import COLUMNS, ShotEvaluator
    assert COLUMNS == R.COLUMNS
    train = _train_labels_with_counts({20: 150, 40: 30, 60: 5})
    ev = ShotEvaluator(train)
    for name in ("update", "reset", "merge_across_ranks", "results", "metrics_of"):
        assert callable(getattr(ev, name)), name
    assert ev.num_labels == 61 and ev.table is None
    x = torch.ones(8)
    with pytest.raises(DirHipError, match="no CPU fallback"):
        ev.update(x, x)
    with pytest.raises(TypeError):
        ev.update(np.ones(8, np.float32), x)
    with pytest.raises(DirHipError, match="label rows"):
        ShotEvaluator(np.array([0.0, 255.0]))                                                   # 256 labels + the "other" row
    assert ShotEvaluator(np.array([0.0, 254.0])).num_labels == 255
    with pytest.raises(ValueError):
        ShotEvaluator(np.array([-1.0, 3.0]))
    with pytest.raises(ValueError):
        ev.metrics_of(np.zeros((5, 5)))
    empty = ev.results()                                                                        # nothing accumulated: every pool is empty
    assert set(empty) == {"overall", "many", "median", "low"}
    assert all(v["num"] == 0 and np.isnan(v["mse"]) and np.isnan(v["l1"]) and np.isnan(v["gmean"]) for v in empty.values())
    ev.reset()
    ev.merge_across_ranks()                                                                     # no process group: a no-op
    # the reference's cast: 20.7 counts as a training sample of label 20 (astype(int))
    assert ShotEvaluator(np.array([20.7] * 101 + [3.0])).shot_of_row[20] == "many"


def test_device_eval_flag_defaults_off_and_shards_only_with_it():
    from dirhip.train_main import build_parser, eval_shard
    for ds in ("imdb_wiki", "agedb"):
        args = build_parser(ds).parse_args([])
        assert args.device_eval is False
        assert build_parser(ds).parse_args(["--device_eval"]).device_eval is True
    idx, valid = eval_shard(7, 1, 2, device_eval=False)
    assert valid is None and torch.equal(idx, torch.arange(7))                                  # the default path walks the whole set on every rank
    idx, valid = eval_shard(7, 0, 1, device_eval=True)
    assert valid is None and torch.equal(idx, torch.arange(7))
    got = [eval_shard(7, r, 2, device_eval=True) for r in range(2)]
    assert [len(i) for i, _ in got] == [4, 4] and sum(int(v.sum()) for _, v in got) == 7
    assert sorted(torch.cat([i[v] for i, v in got]).tolist()) == list(range(7))
