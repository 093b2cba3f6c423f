"""numpy restatement of the FDS statistics pass (K2, ``dir_fds_scatter_stats``) and of the momentum blends (K3,
``dir_fds_finalize_update[_groups]``), the shared test population of ``tests/test_hip_fds_stats.py`` and the bars those tests use.
Plain numpy, no torch.

K2: ``stats_ref``
-----------------
For every bin the rows are cast to ``np.longdouble`` (64-bit significand on x86-64); count, mean = sum / n and the two-pass
``sum((x - mean)^2)`` are formed there and returned as float64. Rows with ``bin < 0`` or ``bin >= nb`` belong to no bin, an empty bin
gives count 0, mean 0, m2 0.

Bars (``tests/test_hip_parity.py::test_scatter_stats_vs_float64_numpy``, through ``conftest.assert_close`` per bin):
    mean  rtol = 1e-12, atol_scale = 1e-13          m2  rtol = 1e-9, atol_scale = 1e-12          counts exact
    a constant column: m2 == 0.0 and mean == the constant, exactly.
The kernel sums float64 differences to the bin's first row (stable order) in pieces of 256 rows and adds the pieces in order. A float64
emulation of that order (the scalar and vec4 forms follow it exactly) on the population below, 2048 columns, bars applied per bin:
    normal         mean 2.1e-4 of its bar, m2 2.1e-5          offset  mean 1.0e-4, m2 1.1e-6
    outlier first  mean 0.74, m2 1.9e-3
"Outlier first" is the near case by construction: the shift is 1e4 away from every other row, so s1 / n is rounded at 1e4 (half an ulp
is 0.9e-12) while the bin's mean is 1e4 / n, 4.9 for the largest bin, whose bar is 1.1e-12 * 4.9. (Applied to the whole [nb, C] table,
whose scale is the one-row bin's 1e4, the same errors are 3.9e-3 of the bar.)

K3: ``finalize_ref``
--------------------
One operation per rounding, exactly as the kernel and imdb-wiki-dir/fds.py:101-111 do it; for every group g of bin b with
n = count[g] > 0, in order:
    tr = f32(tr + f32(n))
    factor = 0.0 | momentum | 1.0 - n / f64(tr)                       (float64)
    a = f32(1.0 - factor);  f = f32(factor)
    cm = f32(mean[g]);      cv = 0 if n == 1 else f32(m2[g] / (n - 1.0))
    rm = f32(f32(a * cm) + f32(f * rm));  rv likewise
The library is compiled with -ffp-contract=off, so the device result is held to ``np.array_equal``.
"""
import numpy as np

f32 = np.float32
MEAN_BAR = dict(rtol=1e-12, atol_scale=1e-13)
M2_BAR = dict(rtol=1e-9, atol_scale=1e-12)
CONST = 0.37109375                                        # 95 / 256: exact in float32, sums of it exact in float64


# ---- K2 -------------------------------------------------------------------------------------------
def _bin_rows(bins, nb):
    """(row indices grouped by bin in stable order, start of every bin in that list [nb + 1])."""
    bins = np.asarray(bins).reshape(-1).astype(np.int64)
    key = np.where((bins >= 0) & (bins < nb), bins, nb)
    order = np.argsort(key, kind="stable")
    starts = np.searchsorted(key[order], np.arange(nb + 1))
    return order, starts


def stats_ref(feats, bins, nb):
    """feats [n, C] float32, bins [n] int -> count [nb], mean [nb, C], m2 [nb, C] float64 (long-double two-pass per bin)."""
    feats = np.asarray(feats, dtype=np.float32)
    n, c = feats.shape
    order, starts = _bin_rows(bins, nb)
    count = np.zeros(nb, np.float64)
    mean = np.zeros((nb, c), np.float64)
    m2 = np.zeros((nb, c), np.float64)
    for b in np.nonzero(np.diff(starts))[0]:
        x = feats[order[starts[b]:starts[b + 1]]].astype(np.longdouble)
        k = x.shape[0]
        mu = x.sum(0) / np.longdouble(k)
        d = x - mu
        count[b] = k
        mean[b] = mu.astype(np.float64)
        m2[b] = (d * d).sum(0).astype(np.float64)
    return count, mean, m2


def stats_f64(feats, bins, nb):
    """The plain float64 two-pass of test_scatter_stats_vs_float64_numpy (checks stats_ref, not the kernel)."""
    feats = np.asarray(feats, dtype=np.float32)
    bins = np.asarray(bins)
    count = np.zeros(nb, np.float64)
    mean = np.zeros((nb, feats.shape[1]), np.float64)
    m2 = np.zeros_like(mean)
    for b in range(nb):
        rows = feats[bins == b].astype(np.float64)
        count[b] = rows.shape[0]
        if rows.shape[0]:
            mean[b] = rows.mean(0)
            m2[b] = ((rows - rows.mean(0)) ** 2).sum(0)
    return count, mean, m2


def bar_fraction(got, want, rtol, atol_scale):
    """max |got - want| / (rtol * |want| + atol_scale * max|want|) over one bin's row: conftest.assert_close passes iff this is <= 1."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = rtol * np.abs(want) + atol_scale * np.max(np.abs(want))
    err = np.abs(got - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(err == 0, 0.0, err / tol)
    return float(np.max(frac))


# ---- the shared population P ----------------------------------------------------------------------
P_COUNTS = (0, 1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1281, 2055)
P_NB = len(P_COUNTS)
P_WIDTH = 2048                                            # widest case; narrower cases take the leading columns
DATA_KINDS = ("normal", "offset", "outlier_first")


def population_bins(seed=20261018):
    """Bin of every row of P: P_COUNTS rows per bin, 200 rows of bin -1, 50 of bin nb, 50 of bin nb + 7, shuffled."""
    bins = np.concatenate([np.full(k, b, np.int32) for b, k in enumerate(P_COUNTS)]
                          + [np.full(200, -1, np.int32), np.full(50, P_NB, np.int32), np.full(50, P_NB + 7, np.int32)])
    np.random.default_rng(seed).shuffle(bins)
    return bins


def population_feats(kind, bins, width=P_WIDTH, seed=3):
    """[n, width] float32 in one of the three data kinds; column 1 is the constant CONST (a one-column case takes that column)."""
    rng = np.random.default_rng(seed)
    n = bins.shape[0]
    if kind == "normal":                                  # the data of test_scatter_stats_vs_float64_numpy
        x = (rng.normal(0.5, 0.3, (n, width)) * (1 + bins[:, None] % 3)).astype(np.float32)
    elif kind == "offset":
        x = (1000.0 + 1e-2 * rng.normal(0.0, 1.0, (n, width))).astype(np.float32)
    elif kind == "outlier_first":
        x = rng.normal(0.0, 1.0, (n, width)).astype(np.float32)
        order, starts = _bin_rows(bins, P_NB)
        first = order[starts[:-1][np.diff(starts) > 0]]   # lowest row index of every non-empty bin = the kernel's shift row
        x[first] = 1e4
    else:
        raise ValueError(kind)
    x[:, 1] = CONST
    return x


def columns(table, c):
    """The columns of a [*, P_WIDTH] array that the C = c case holds: the leading c, or the constant column alone for c = 1."""
    return np.ascontiguousarray(table[:, 1:2] if c == 1 else table[:, :c])


# ---- K3 -------------------------------------------------------------------------------------------
def finalize_ref(count, mean, m2, bin_ptr, factor_mode, momentum, rm, rv, tracked):
    """Returns new (running_mean, running_var, num_samples_tracked); bin_ptr None = group b is the one group of bin b."""
    count = np.asarray(count, np.float64)
    mean = np.asarray(mean, np.float64)
    m2 = np.asarray(m2, np.float64)
    rm = np.array(rm, dtype=np.float32, copy=True)
    rv = np.array(rv, dtype=np.float32, copy=True)
    tracked = np.array(tracked, dtype=np.float32, copy=True)
    for b in range(rm.shape[0]):
        g0, g1 = (b, b + 1) if bin_ptr is None else (int(bin_ptr[b]), int(bin_ptr[b + 1]))
        tr = f32(tracked[b])
        for g in range(g0, g1):
            n = float(count[g])
            if n <= 0.0:
                continue
            tr = f32(tr + f32(n))
            if factor_mode == 0:
                factor = 0.0
            elif factor_mode == 1:
                factor = float(momentum)
            else:
                factor = 1.0 - n / float(tr)
            a, f = f32(1.0 - factor), f32(factor)
            cm = mean[g].astype(np.float32)
            cv = np.zeros_like(cm) if n == 1.0 else (m2[g] / (n - 1.0)).astype(np.float32)
            rm[b] = a * cm + f * rm[b]
            rv[b] = a * cv + f * rv[b]
        tracked[b] = tr
    return rm, rv, tracked
