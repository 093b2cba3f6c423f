"""CPU-side tests of tests/fds_stats_reference.py, the references the -m gpu tests of tests/test_hip_fds_stats.py hold K2
(``dir_fds_scatter_stats``) and K3 (``dir_fds_finalize_update[_groups]``) to:

* ``stats_ref`` -> ``finalize_ref`` chained over every epoch of the golden FDS traces reproduce the tables the reference itself recorded;
* ``finalize_ref`` equals ``FDSOracle.update_running_stats`` bit for bit when fed the float64 statistics the oracle forms;
* ``stats_ref`` (long double) agrees with the plain float64 two-pass on the shared population within a tenth of the K2 bars.
"""
import json

import numpy as np
import pytest

import fds_stats_reference as R
from conftest import assert_close
from oracle import fds_oracle

TRACES = ["imdb", "agedb", "absent", "nomomentum", "frac", "fracnomom"]


def factor_mode(kw, epoch):
    """FDS.apply_stats: fds.py:105-107."""
    if epoch == kw["start_update"]:
        return 0, 0.0
    if kw["momentum"] is not None:
        return 1, float(kw["momentum"])
    return 2, 0.0


@pytest.mark.parametrize("name", TRACES)
def test_chained_references_reproduce_golden_traces(golden, name):
    from dirhip.fds import value_groups
    g = golden(f"fds_trace_{name}.npz")
    kw = json.loads(str(g["kw"]))
    start, num = kw["bucket_start"], kw["bucket_num"]
    nb = num - start
    rm = np.zeros((nb, kw["feature_dim"]), np.float32)
    rv = np.ones((nb, kw["feature_dim"]), np.float32)
    tr = np.zeros(nb, np.float32)
    fds_epoch = kw["start_update"]                        # the module's `epoch` buffer (fds.py:28, :78-82, :85)
    updates = 0
    for epoch in range(5):
        if epoch == fds_epoch + 1:
            fds_epoch += 1
        if epoch >= fds_epoch:
            feats, labels = g[f"e{epoch}_in_feats"], g[f"e{epoch}_in_labels"]
            if name.startswith("frac"):
                gid, bin_ptr, ngroups = value_groups(labels, start, num)
                assert ngroups == int(g[f"e{epoch}_n_distinct_in_range"]) > nb
                count, mean, m2 = R.stats_ref(feats, gid, ngroups)
            else:
                bin_ptr = None
                count, mean, m2 = R.stats_ref(feats, fds_oracle.bin_index(labels, start, num), nb)
            mode, mom = factor_mode(kw, epoch)
            rm, rv, tr = R.finalize_ref(count, mean, m2, bin_ptr, mode, mom, rm, rv, tr)
            updates += 1
        assert_close(rm, g[f"e{epoch}_post_running_mean"], msg=f"{name} e{epoch} running_mean")
        assert_close(rv, g[f"e{epoch}_post_running_var"], msg=f"{name} e{epoch} running_var")
        assert np.array_equal(tr, g[f"e{epoch}_post_num_samples_tracked"]), f"{name} e{epoch}"
    assert updates >= 4


@pytest.mark.parametrize("momentum,start_update", [(0.9, 0), (None, 0), (None, 1)])
def test_finalize_ref_bit_equal_fds_oracle(momentum, start_update):
    """The oracle's own float64 mean and m2 (numpy's mean / var: sum / n, sum((x - mean)^2) / (n - ddof)) through finalize_ref."""
    rng = np.random.default_rng(11)
    c, start, num = 9, 2, 14
    nb = num - start
    O = fds_oracle.FDSOracle(c, bucket_num=num, bucket_start=start, start_update=start_update, momentum=momentum)
    rm, rv, tr = O.running_mean.copy(), O.running_var.copy(), O.num_samples_tracked.copy()
    for epoch in range(start_update, start_update + 3):
        n = 400
        labels = rng.integers(0, 17, n).astype(np.float32)
        labels[labels == 5] = 6                            # an empty bin
        labels[0] = 9.0
        labels[1:n][labels[1:n] == 9] = 8                  # a bin of one row (ddof = 0 branch)
        feats = (rng.normal(0.5, 0.3, (n, c)) * (1 + labels[:, None] % 3)).astype(np.float32)
        feats[:, 1] = R.CONST
        O.update_last_epoch_stats(epoch)
        O.update_running_stats(feats, labels, epoch)
        bins = fds_oracle.bin_index(labels, start, num)
        count = np.zeros(nb)
        mean = np.zeros((nb, c))
        m2 = np.zeros((nb, c))
        for b in range(nb):
            cur = feats[bins == b].astype(np.float64)
            count[b] = cur.shape[0]
            if cur.shape[0]:
                mean[b] = cur.mean(0)
                d = cur - cur.mean(0, keepdims=True)
                m2[b] = (d * d).sum(0)
        assert (count == 0).any() and (count == 1).any()
        mode = 0 if epoch == start_update else (1 if momentum is not None else 2)
        rm, rv, tr = R.finalize_ref(count, mean, m2, None, mode, momentum or 0.0, rm, rv, tr)
        assert np.array_equal(rm, O.running_mean)
        assert np.array_equal(rv, O.running_var)
        assert np.array_equal(tr, O.num_samples_tracked)


def test_finalize_ref_leaves_untouched_bins_alone():
    c = 3
    count = np.array([0.0, 2.0, 0.0])
    mean, m2 = np.ones((3, c)), np.ones((3, c))
    rm = np.array([[np.nan] * c, [1.0] * c, [-0.0] * c], np.float32)
    bin_ptr = np.array([0, 1, 2, 3, 3], np.int32)          # bin 3 has no group, bins 0 and 2 a zero-count group
    rm4 = np.vstack([rm, np.full((1, c), np.nan, np.float32)])
    got_rm, got_rv, got_tr = R.finalize_ref(count, mean, m2, bin_ptr, 1, 0.9, rm4, rm4, np.array([3, 0, 5, 7], np.float32))
    for b in (0, 2, 3):
        assert np.array_equal(got_rm[b].view(np.uint32), rm4[b].view(np.uint32))
        assert np.array_equal(got_rv[b].view(np.uint32), rm4[b].view(np.uint32))
    assert np.array_equal(got_tr, np.array([3, 2, 5, 7], np.float32))
    assert np.array_equal(got_rm[1], np.full(c, np.float32(1.0 - 0.9) * np.float32(1) + np.float32(0.9) * np.float32(1), np.float32))


@pytest.mark.parametrize("kind", R.DATA_KINDS)
def test_stats_ref_vs_float64_two_pass_on_population(kind):
    bins = R.population_bins()
    assert bins.shape[0] == 11535 and np.array_equal(np.bincount(bins[(bins >= 0) & (bins < R.P_NB)], minlength=R.P_NB), R.P_COUNTS)
    feats = R.population_feats(kind, bins, width=24)
    count, mean, m2 = R.stats_ref(feats, bins, R.P_NB)
    count64, mean64, m264 = R.stats_f64(feats, bins, R.P_NB)
    assert np.array_equal(count, count64) and np.array_equal(count, R.P_COUNTS)
    assert not mean[0].any() and not m2[0].any()
    tenth = lambda bar: {k: v / 10 for k, v in bar.items()}
    for b in range(1, R.P_NB):
        assert_close(mean64[b], mean[b], msg=f"{kind} mean b={b}", **tenth(R.MEAN_BAR))
        assert_close(m264[b], m2[b], msg=f"{kind} m2 b={b}", **tenth(R.M2_BAR))
        assert m2[b, 1] == 0.0 and mean[b, 1] == R.CONST
    if kind == "outlier_first":
        first = np.array([np.nonzero(bins == b)[0][0] for b in range(1, R.P_NB)])
        assert (feats[first][:, [0, 2]] == 1e4).all() and (np.abs(np.delete(feats, first, 0)) < 10).all()
