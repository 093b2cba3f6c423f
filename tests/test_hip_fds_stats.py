"""-m gpu: the FDS statistics pass K2 (``dir_fds_scatter_stats``: counting sort, piece sums, combine) and the momentum blends K3
(``dir_fds_finalize_update[_groups]``) in every launch form, against the numpy references of tests/fds_stats_reference.py, plus the
bin-assignment and fill kernels the STS-B / NYUD2 variants put in front of them.

K2 is held to a long-double two-pass per bin at the bars of test_scatter_stats_vs_float64_numpy (mean 1e-12 / 1e-13, m2 1e-9 / 1e-12,
counts exact, a constant column exact); the achieved worst error of every case, as a fraction of its bar, goes to
``records_dir()/fds_stats_bar_fractions.json``. K3 is held bit for bit to ``finalize_ref``. The bin kernels are exact integers.

Shapes are the smallest that reach each branch: the population P of fds_stats_reference (bin sizes on each side of the piece size 256,
PIECE_UNROLL 8, the wavefront 64 and the combine unroll of 4 pieces) at every row form, the grouping edges (last-chunk break, nb > 256,
nb at the LDS cap), and one input of more than 4096 tiles for the second pass of the tile scan.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import fds_stats_reference as R
from conftest import assert_close, records_dir
from test_hip_fds_forms import dev, dev_offset4

pytestmark = pytest.mark.gpu
_RECORD = {}


def record(case, worst):
    _RECORD[case] = worst
    with open(os.path.join(records_dir(), "fds_stats_bar_fractions.json"), "w") as fh:
        json.dump(_RECORD, fh, indent=1, sort_keys=True)


def run_stats(feats_dev, bins_dev, nb):
    from dirhip import ops
    return tuple(t.cpu().numpy() for t in ops.scatter_stats(feats_dev, bins_dev, nb))


def check_stats(case, got, want, const_col=None):
    """Counts exact, empty bins all zero, every non-empty bin's mean and m2 rows inside the bars; records the worst bar fractions first."""
    cnt, mean, m2 = got
    wcnt, wmean, wm2 = want
    assert np.array_equal(cnt, wcnt), case
    assert not np.isnan(mean).any() and not np.isnan(m2).any(), case
    live = np.nonzero(wcnt > 0)[0]
    worst = {"mean": 0.0, "m2": 0.0}
    for b in live:
        worst["mean"] = max(worst["mean"], R.bar_fraction(mean[b], wmean[b], **R.MEAN_BAR))
        worst["m2"] = max(worst["m2"], R.bar_fraction(m2[b], wm2[b], **R.M2_BAR))
    record(case, worst)
    print(f"{case}: worst fraction of the bar: mean {worst['mean']:.3g}, m2 {worst['m2']:.3g}")
    assert not mean[wcnt == 0].any() and not m2[wcnt == 0].any(), case
    for b in live:
        assert_close(mean[b], wmean[b], msg=f"{case} mean b={b}", **R.MEAN_BAR)
        assert_close(m2[b], wm2[b], msg=f"{case} m2 b={b}", **R.M2_BAR)
    if const_col is not None:
        assert (m2[live, const_col] == 0.0).all() and (mean[live, const_col] == R.CONST).all(), case


# ---- K2 on the shared population, every row form ---------------------------------------------------
@pytest.fixture(scope="module")
def population():
    """bins, {kind: (feats [n, 2048], stats_ref of them)}: one reference per data kind; a case of C columns takes the leading C."""
    bins = R.population_bins()
    data = {}
    for kind in R.DATA_KINDS:
        feats = R.population_feats(kind, bins)
        data[kind] = (feats, R.stats_ref(feats, bins, R.P_NB))
    return bins, data


def population_case(population, kind, c, put=dev):
    bins, data = population
    feats, (wcnt, wmean, wm2) = data[kind]
    got = run_stats(put(R.columns(feats, c)), dev(bins), R.P_NB)
    return got, (wcnt, R.columns(wmean, c), R.columns(wm2, c))


@pytest.mark.parametrize("c", [
    1, 7,                 # scalar form, C % 4 != 0
    257,                  # scalar form, second column tile with one live lane
    4,                    # narrow, tpr = 1, rl = 256: every lane has at most one row
    8, 64,                # narrow, middle rl
    128,                  # narrow, rl = 8 (the dense NYUD2 variant's form)
    512,                  # narrow, tpr = 128, rl = 2: the unrolled loop runs 32 times per piece
    12,                   # vec4 because 256 % 3 != 0; 3 live lanes of 256
    516,                  # vec4 because tpr = 129 > 128
    1028,                 # vec4, second column tile with one live lane
    2048,                 # the age variants' feature width
])
def test_population_every_row_form(population, c):
    for kind in R.DATA_KINDS:
        got, want = population_case(population, kind, c)
        check_stats(f"P C={c} {kind}", got, want, const_col=1 % c)


def test_population_misaligned_feats_takes_scalar_form(population):
    """C = 128 with feats starting 4 bytes into its buffer: the scalar form chosen by alignment. Same statistics as the aligned
    (narrow) run within the bars; not bit for bit, the lane fold order differs."""
    for kind in R.DATA_KINDS:
        got, want = population_case(population, kind, 128, put=dev_offset4)
        check_stats(f"P C=128 offset4 {kind}", got, want, const_col=1)
        aligned, _ = population_case(population, kind, 128)
        check_stats(f"P C=128 offset4 vs aligned {kind}", got, aligned, const_col=1)


# ---- K2 grouping edges (C = 8, the normal data) ----------------------------------------------------
def normal_feats(rng, bins, c):
    x = (rng.normal(0.5, 0.3, (bins.shape[0], c)) * (1 + bins[:, None] % 3)).astype(np.float32)
    x[:, 1 % c] = R.CONST
    return x


def edge_bins(rng, n, nb, sparse):
    if sparse:                                            # most bins empty; the first, the last and both sides of a 256-bin chunk are not
        ids = np.unique(np.concatenate([rng.choice(nb, nb // 8, replace=False), [0, 255, 256, nb - 1]]))
        bins = rng.choice(ids, n).astype(np.int32)
        bins[:4] = (0, 255, 256, nb - 1)
    else:
        bins = rng.integers(-1, nb, n).astype(np.int32)
        bins[0] = nb - 1
    return bins


@pytest.mark.parametrize("n,nb,sparse", [
    (1, 5, False), (63, 5, False), (64, 5, False), (65, 5, False),          # the place kernel's early break,
    (255, 5, False), (256, 5, False), (257, 5, False), (320, 5, False),     # full and partial last chunk
    (300, 1, False),                                                        # nbits = 0
    (300, 2, False),
    (3000, 64, False), (3000, 65, False), (3000, 256, False), (3000, 257, False), (3000, 300, False),
    (9000, 8000, True),                                   # dirhip.fds.MAX_VALUE_GROUPS: 32 chunks of the bin scan, nbits = 13
    (2000, 16384, True),                                  # the cap: one LDS counter per bin, 64 KB per grouping wavefront
])
def test_grouping_edges(n, nb, sparse):
    rng = np.random.default_rng(1000 * nb + n)
    bins = edge_bins(rng, n, nb, sparse)
    feats = normal_feats(rng, bins, 8)
    want = R.stats_ref(feats, bins, nb)
    assert want[0].sum() > 0 and want[0][nb - 1] > 0
    if sparse:
        assert (want[0] == 0).sum() > nb // 2
    check_stats(f"edges n={n} nb={nb}", run_stats(dev(feats), dev(bins), nb), want, const_col=1)


def test_more_bins_than_lds_counters_is_refused():
    from dirhip import _lib as L
    from dirhip import ops
    feats = torch.zeros(16, 8, device="cuda")
    bins = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(L.DirHipError, match="unsupported"):
        ops.scatter_stats(feats, bins, 16385)


def test_every_row_outside_every_bin():
    rng = np.random.default_rng(5)
    n, nb, c = 300, 5, 8
    bins = np.full(n, -1, np.int32)
    bins[::3] = nb + 2
    cnt, mean, m2 = run_stats(dev(rng.normal(0, 1, (n, c)).astype(np.float32)), dev(bins), nb)
    for t in (cnt, mean, m2):
        assert not np.isnan(t).any() and not t.any()


def test_no_rows_zeroes_the_outputs():
    from dirhip import _lib as L
    nb, c = 5, 8
    cnt = torch.full((nb,), float("nan"), dtype=torch.float64, device="cuda")
    mean = torch.full((nb, c), float("nan"), dtype=torch.float64, device="cuda")
    m2 = torch.full((nb, c), float("nan"), dtype=torch.float64, device="cuda")
    L.check(L.lib().dir_fds_scatter_stats(None, L.DIR_F32, None, 0, c, nb, L.ptr(cnt), L.ptr(mean), L.ptr(m2), None, 0,
                                          L.stream_ptr(cnt.device)), "dir_fds_scatter_stats")
    for t in (cnt, mean, m2):
        assert not t.cpu().numpy().any() and not torch.isnan(t).any()


def test_more_than_4096_tiles():
    """n = 2^20 + 300 rows: 4098 grouping tiles, the second pass of the tile scan and its carry; about 1024 pieces per bin in the combine."""
    rng = np.random.default_rng(8)
    n, c, nb = 1048576 + 300, 4, 3
    bins = rng.integers(-1, nb, n).astype(np.int32)
    feats = normal_feats(rng, bins, c)
    check_stats(f"tiles n={n}", run_stats(dev(feats), dev(bins), nb), R.stats_ref(feats, bins, nb), const_col=1)


# ---- K2 workspace ----------------------------------------------------------------------------------
def test_workspace_contents_do_not_matter_and_guard_survives(population):
    from dirhip import _lib as L
    bins, data = population
    c, nb, n = 128, R.P_NB, bins.shape[0]
    feats, dbins = dev(R.columns(data["normal"][0], c)), dev(bins)
    nbytes = L.lib().dir_fds_scatter_stats_workspace(n, c, nb)
    assert nbytes > 0 and nbytes % 256 == 0

    def call(fill, offset=0, claim=nbytes):
        buf = torch.empty(nbytes + 256 + offset, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 256 == 0
        buf[:offset + nbytes] = fill
        buf[offset + nbytes:] = 0xA5
        out = [torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((nb,), (nb, c), (nb, c))]
        rc = L.lib().dir_fds_scatter_stats(L.ptr(feats), L.DIR_F32, L.ptr(dbins), n, c, nb, *(L.ptr(t) for t in out),
                                           ctypes.c_void_p(buf.data_ptr() + offset), claim, L.stream_ptr(feats.device))
        torch.cuda.synchronize()
        assert (buf[offset + nbytes:] == 0xA5).all()
        return rc, [t.cpu().numpy() for t in out]

    rc_a, a = call(0xFF)
    rc_b, b = call(0x00)
    assert rc_a == 0 and rc_b == 0
    for u, v in zip(a, b):
        assert not np.isnan(u).any() and np.array_equal(u, v)
    wcnt, wmean, wm2 = data["normal"][1]
    check_stats("P C=128 workspace 0xFF", tuple(a), (wcnt, R.columns(wmean, c), R.columns(wm2, c)), const_col=1)
    # host-side refusals: nothing is launched, the outputs keep their NaN fill
    rc, out = call(0x00, claim=nbytes - 1)
    assert rc == -3 and all(np.isnan(t).all() for t in out)                 # DIR_EWORKSPACE
    rc, out = call(0x00, offset=128)
    assert rc == -1 and all(np.isnan(t).all() for t in out)                 # DIR_EINVAL


# ---- K3, bit for bit -------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def finalize_inputs(rng, count, c, tracked0):
    """Statistics per group and start tables per bin; rows of bins that no blend touches are seeded by the caller."""
    ng, nb = count.shape[0], tracked0.shape[0]
    mean = rng.normal(0, 1, (ng, c))
    m2 = rng.uniform(0, 4, (ng, c)) * np.maximum(count, 1)[:, None]
    rm0 = rng.normal(0, 1, (nb, c)).astype(np.float32)
    rv0 = rng.uniform(0.5, 2, (nb, c)).astype(np.float32)
    return mean, m2, rm0, rv0


def run_finalize(count, mean, m2, bin_ptr, mode, rm0, rv0, tr0):
    from dirhip import ops
    rm, rv, tr = dev(rm0), dev(rv0), dev(tr0)
    if bin_ptr is None:
        ops.finalize_update(dev(count), dev(mean), dev(m2), mode, 0.9, rm, rv, tr)
    else:
        ops.finalize_update_groups(dev(count), dev(mean), dev(m2), dev(bin_ptr), mode, 0.9, rm, rv, tr)
    want = R.finalize_ref(count, mean, m2, bin_ptr, mode, 0.9, rm0, rv0, tr0)
    for got, ref, start, what in zip((rm, rv, tr), want, (rm0, rv0, tr0), ("running_mean", "running_var", "num_samples_tracked")):
        got = got.cpu().numpy()
        assert np.array_equal(bits(got), bits(ref)), f"{what}: {int((bits(got) != bits(ref)).sum())} elements differ"
    return want


GROUP_COUNTS = np.array([5,                               # bin 1
                         0, 1, 100000,                    # bin 2: a zero-count and a one-row group first
                         0, 0,                            # bin 3: every group empty
                         3,                               # bin 4
                         1, 0, 99999, 100001], np.float64)    # bin 5 starts at 16 777 216: + 1 rounds back, then every sum is a tie
GROUPS_PER_BIN = (0, 1, 3, 2, 1, 4)
TWO24 = np.float32(16777216)


@pytest.mark.parametrize("c", [1, 5, 300, 16385])          # 16 385: gy caps at 64, the column loop strides
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_finalize_groups_bit_equal_reference(c, mode):
    rng = np.random.default_rng(100 * c + mode)
    bin_ptr = np.concatenate([[0], np.cumsum(GROUPS_PER_BIN)]).astype(np.int32)
    tr0 = np.array([7, 7, 0, 5, 0, TWO24], np.float32)
    mean, m2, rm0, rv0 = finalize_inputs(rng, GROUP_COUNTS, c, tr0)
    rm0[0], rv0[0] = np.nan, -0.0                         # bin 0 has no group, bin 3 only empty ones: both keep their bits
    rm0[3], rv0[3] = -0.0, np.nan
    rm, rv, tr = run_finalize(GROUP_COUNTS, mean, m2, bin_ptr, mode, rm0, rv0, tr0)
    for b in (0, 3):
        assert np.array_equal(bits(rm[b]), bits(rm0[b])) and np.array_equal(bits(rv[b]), bits(rv0[b])) and tr[b] == tr0[b]
    assert TWO24 + np.float32(1) == TWO24                 # the first blend of bin 5 sees tracked unchanged
    assert tr[5] == np.float32(np.float32(TWO24 + np.float32(99999)) + np.float32(100001)) == 16977216 != 16777216 + 1 + 99999 + 100001
    assert not np.isnan(rm[[1, 2, 4, 5]]).any() and not np.array_equal(rm[[1, 2, 4, 5]], rm0[[1, 2, 4, 5]])


@pytest.mark.parametrize("c", [1, 5, 300, 16385])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_finalize_update_bit_equal_reference(c, mode):
    """dir_fds_finalize_update: the same counts, one group per bin (so each rounding case of `tracked` gets a bin of its own)."""
    rng = np.random.default_rng(100 * c + mode + 7)
    tr0 = np.array([7, 5, 0, 0, 3, 9, TWO24, TWO24, 1, TWO24, 0], np.float32)
    mean, m2, rm0, rv0 = finalize_inputs(rng, GROUP_COUNTS, c, tr0)
    empty = np.nonzero(GROUP_COUNTS == 0)[0]
    rm0[empty[::2]], rv0[empty[::2]] = np.nan, -0.0
    rm0[empty[1::2]], rv0[empty[1::2]] = -0.0, np.nan
    rm, rv, tr = run_finalize(GROUP_COUNTS, mean, m2, None, mode, rm0, rv0, tr0)
    assert np.array_equal(bits(rm[empty]), bits(rm0[empty])) and np.array_equal(bits(rv[empty]), bits(rv0[empty]))
    assert np.array_equal(tr[empty], tr0[empty])
    assert tr[6] == 16777220 and tr[7] == 16777216        # + 3 is a tie that goes to even, + 1 rounds back


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_finalize_second_workgroup_of_tracked(grouped, mode):
    """nb = 257, C = 5: bin 256 is the tracked kernel's second workgroup."""
    rng = np.random.default_rng(257 + mode)
    nb, c = 257, 5
    per_bin = rng.integers(0, 3, nb) if grouped else np.ones(nb, np.int64)
    per_bin[nb - 1] = 2 if grouped else 1
    bin_ptr = np.concatenate([[0], np.cumsum(per_bin)]).astype(np.int32) if grouped else None
    count = rng.integers(0, 40, int(per_bin.sum())).astype(np.float64)
    count[-1] = 17
    tr0 = rng.integers(0, 1000, nb).astype(np.float32)
    mean, m2, rm0, rv0 = finalize_inputs(rng, count, c, tr0)
    rm, rv, tr = run_finalize(count, mean, m2, bin_ptr, mode, rm0, rv0, tr0)
    assert tr[nb - 1] > tr0[nb - 1] and not np.array_equal(rm[nb - 1], rm0[nb - 1])


# ---- the bin-assignment and fill kernels in front of K2 --------------------------------------------
def neighbours(v):
    """float32 values, the value below and the value above each."""
    v = np.asarray(v, np.float32)
    return np.concatenate([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))])


def test_bin_scaled_exact():
    """ops.bin_scaled(mult 10, start 7, num 100) against nyud2-dir/models/fds.py:51-53 as the oracle restates it."""
    from dirhip import ops
    from oracle import fds_nyud2_oracle as no
    start, num = 7, 100
    grid = neighbours(neighbours((np.arange(0, 121) / 10.0).astype(np.float32)))       # k / 10 and two float32 steps to either side
    f32_bucket = np.trunc(grid * np.float32(10))
    f64_bucket = np.trunc(grid.astype(np.float64) * 10.0)
    assert (f32_bucket != f64_bucket).any()               # the float32 product rounds across an integer somewhere
    special = np.array([0.0, -0.0, -0.05, -3.5, -1e30, 1e30, np.inf, -np.inf], np.float32)
    n = 1048576 + 5                                       # past 4096 workgroups: the grid-stride loop runs
    rng = np.random.default_rng(9)
    labels = np.concatenate([grid, special, rng.uniform(-1, 12, n - grid.size - special.size).astype(np.float32)])
    labels[-5:] = (0.7, 9.95, 12.0, -0.0, 1e30)
    want = (no.bucket_idx(labels, start, num) - start).astype(np.int32)
    assert want.min() == 0 and want.max() == num - 1 - start and want[grid.size + 5] == num - 1 - start
    got = ops.bin_scaled(dev(labels), 10.0, start, num).cpu().numpy()
    assert np.array_equal(got, want)
    nan = ops.bin_scaled(dev(np.array([0.75, np.nan, 1.0], np.float32)), 10.0, start, num).cpu().numpy()
    assert np.array_equal(nan, [0, -1, 3])


def edges_ref(labels, edges, start, num):
    """sts-b-dir/fds.py:51-57 vectorised: (first edge > label) - 1 = (number of edges <= label) - 1."""
    b = np.maximum(np.searchsorted(edges, labels, side="right") - 1, start)
    return (np.where(labels == edges[-1], num - 1, b) - start).astype(np.int32)


@pytest.mark.parametrize("num,start,n", [
    (50, 0, None), (50, 3, None),
    (299, 0, None),                                       # 300 edges: second trip of the LDS load loop
    (50, 3, 262144 + 7),                                  # past 1024 workgroups: the grid-stride loop runs
])
def test_bin_edges_exact(num, start, n):
    from dirhip import ops
    from oracle import fds_stsb_oracle as so
    edges = so.stsb_edges(num)
    assert edges.size == num + 1 and edges[-1] == np.float32(5.0)
    labels = neighbours(edges)
    labels = labels[labels <= np.float32(5.0)]            # (the neighbour above 5.0 is asserted separately: the reference raises there)
    assert (labels < 0).any() and (labels == np.float32(5.0)).any()
    want = (so.bucket_idx(labels, start, num) - start).astype(np.int32)
    assert np.array_equal(edges_ref(labels, edges, start, num), want)
    assert want[labels < 0][0] == 0 and want.max() == num - 1 - start
    if n is not None:
        rng = np.random.default_rng(n)
        labels = np.concatenate([labels, rng.uniform(0, 5, n - labels.size).astype(np.float32)])
        labels[-7:] = (5.0, 0.0, 4.9999995, 2.5, -1.0, 0.1, 5.0)
        want = edges_ref(labels, edges, start, num)
    got = ops.bin_edges(dev(labels), dev(edges), start, num).cpu().numpy()
    assert np.array_equal(got, want)
    outside = np.array([np.nextafter(np.float32(5.0), np.float32(np.inf)), np.nan, np.inf, 2.5], np.float32)
    assert np.array_equal(ops.bin_edges(dev(outside), dev(edges), start, num).cpu().numpy(),
                          [-1, -1, -1, edges_ref(outside[3:], edges, start, num)[0]])


def fill_ref(count, rm, rv):
    """sts-b-dir/fds.py:112-125 in float32, buckets in increasing order; nb = 1 moves nothing."""
    rm, rv = rm.copy(), rv.copy()
    nb = count.shape[0]
    for b in range(nb):
        if count[b] > 0:
            continue
        for t in (rm, rv):
            if b == 0:
                if nb > 1:
                    t[0] = t[1]
            elif b == nb - 1:
                t[b] = t[b - 1]
            else:
                t[b] = (t[b - 1] + t[b + 1]) / np.float32(2.0)
    return rm, rv


@pytest.mark.parametrize("c", [5, 300])
@pytest.mark.parametrize("count", [
    (0, 0, 3, 1, 2, 5, 1, 4),                             # left edge: buckets 0 and 1 both empty
    (2, 1, 3, 1, 2, 5, 0, 0),                             # right edge
    (1, 2, 0, 0, 0, 3, 1, 2),                             # a run of three in the middle: the fill propagates from the left
    (0, 2, 0, 0, 0, 3, 0, 0),
    (0, 0, 0, 0, 0, 0, 0, 0),
    (1, 2, 3, 4, 5, 6, 7, 8),
    (0,), (4,),
    (0, 1), (1, 0), (0, 0),
])
def test_fill_empty_buckets_bit_equal(c, count):
    from dirhip import ops
    count = np.array(count, np.float64)
    nb = count.shape[0]
    rng = np.random.default_rng(10 * nb + c)
    rm0 = rng.normal(0, 1, (nb, c)).astype(np.float32)
    rv0 = rng.uniform(0.5, 2, (nb, c)).astype(np.float32)
    rm, rv = dev(rm0), dev(rv0)
    ops.fill_empty_buckets(dev(count), rm, rv)
    want_rm, want_rv = fill_ref(count, rm0, rv0)
    assert np.array_equal(bits(rm.cpu().numpy()), bits(want_rm))
    assert np.array_equal(bits(rv.cpu().numpy()), bits(want_rv))
    if (count > 0).all() or nb == 1:
        assert np.array_equal(want_rm, rm0) and np.array_equal(want_rv, rv0)
