"""-m gpu: every launch form of the FDS calibration, multiplier-table and finalize kernels at the smallest shape that reaches it,
bit-equal (np.array_equal) to a numpy float32 restatement with one operation per rounding:

    forward   np.where(s < 0, x, (x - m1) * s + m2)   on the table rows the bins gather
    backward  np.where(s < 0, g, g * s)
    bin < 0   the row / pixel is returned unchanged

Tables have nb = 5 rows unless stated, bins include -1, about 5 % of the multipliers are -1 ("column untouched").
"""
import numpy as np
import pytest
import torch

from oracle import fds_oracle

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def dev_offset4(a):
    """A contiguous device copy of float32 ``a`` that starts 4 bytes into its buffer (no 16-byte accesses possible)."""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(a.shape)
    v.copy_(torch.as_tensor(np.ascontiguousarray(a)))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def make_tables(rng, nb, c):
    m1 = rng.normal(0, 1, (nb, c)).astype(np.float32)
    m2 = rng.normal(0, 1, (nb, c)).astype(np.float32)
    s = rng.uniform(0.5, 1.5, (nb, c)).astype(np.float32)
    s[rng.random((nb, c)) < 0.05] = -1.0
    s[0, 2] = s[nb - 1, 1] = -1.0                         # untouched columns in rows every case's bins use
    return m1, s, m2


def make_bins(rng, n, nb):
    bins = rng.integers(-1, nb, n).astype(np.int32)
    bins[0] = nb - 1
    bins[n // 2] = -1
    return bins


def fwd_ref(x, bins, m1, s, m2):
    b = np.maximum(bins, 0)
    y = np.where(s[b] < 0, x, (x - m1[b]) * s[b] + m2[b])
    return np.where(bins[:, None] < 0, x, y).astype(np.float32)


def bwd_ref(g, bins, s):
    b = np.maximum(bins, 0)
    return np.where(bins[:, None] < 0, g, np.where(s[b] < 0, g, g * s[b])).astype(np.float32)


def to_rows(a):                                           # [N, C, H, W] -> [N*H*W, C]
    return a.transpose(0, 2, 3, 1).reshape(-1, a.shape[1])


def from_rows(r, shape):
    n, c, h, w = shape
    return r.reshape(n, h, w, c).transpose(0, 3, 1, 2)


# ---- row forms: dir_fds_calibrate_fwd / dir_fds_calibrate_bwd --------------------------------------
@pytest.mark.parametrize("b,c,misalign", [
    (5, 7, False),        # scalar: C % 4 != 0
    (5, 8, True),         # scalar by misalignment
    (130, 8, False),      # narrow, tpr = 2, ragged second row pass
    (3, 512, False),      # narrow, tpr = 128
    (3, 24, False),       # tpr = 6 does not divide 256: vec4 wide
    (2, 1028, False),     # vec4 wide, second column block partial
])
def test_row_forms_fwd_bwd(b, c, misalign):
    from dirhip import _lib as L
    nb = 5
    rng = np.random.default_rng(1000 * b + c)
    m1, s, m2 = make_tables(rng, nb, c)
    bins = make_bins(rng, b, nb)
    x = rng.normal(0, 1, (b, c)).astype(np.float32)
    g = rng.normal(0, 1, (b, c)).astype(np.float32)
    put = dev_offset4 if misalign else dev
    dm1, ds, dm2, dbins = dev(m1), dev(s), dev(m2), dev(bins)
    xd = put(x)
    L.check(L.lib().dir_fds_calibrate_fwd(L.ptr(xd), L.DIR_F32, L.ptr(dbins), b, c, L.ptr(dm1), L.ptr(ds), L.ptr(dm2),
                                          L.stream_ptr(xd.device)), "dir_fds_calibrate_fwd")
    assert np.array_equal(xd.cpu().numpy(), fwd_ref(x, bins, m1, s, m2))
    gd = put(g)
    dx = torch.empty(b, c, device="cuda")
    L.check(L.lib().dir_fds_calibrate_bwd(L.ptr(gd), L.ptr(dx), L.DIR_F32, L.ptr(dbins), b, c, L.ptr(ds),
                                          L.stream_ptr(gd.device)), "dir_fds_calibrate_bwd")
    assert np.array_equal(dx.cpu().numpy(), bwd_ref(g, bins, s))
    assert np.array_equal(gd.cpu().numpy(), g)


# ---- LDS-staged form -------------------------------------------------------------------------------
@pytest.mark.parametrize("b,c,nb", [
    (37, 136, 5),         # second column tile partial, rows ragged against the 4-rows-in-flight loop
    (37, 32, 300),        # table too tall for a 128-column tile: 32-column tile
])
def test_lds_staged_form(b, c, nb):
    from dirhip import ops
    rng = np.random.default_rng(1000 * b + c + nb)
    m1, s, m2 = make_tables(rng, nb, c)
    bins = make_bins(rng, b, nb)
    x = rng.normal(0, 1, (b, c)).astype(np.float32)
    got = ops.calibrate_fwd_lds_(dev(x), dev(bins), dev(m1), dev(s), dev(m2))
    assert np.array_equal(got.cpu().numpy(), fwd_ref(x, bins, m1, s, m2))


# ---- dir_fds_smooth_fwd ----------------------------------------------------------------------------
BUCKET_START, BUCKET_NUM = 2, 7                           # nb = 5; labels 2 and 6 are the boundary values


def _smooth_labels(case):
    if case == "fused_scalar":                            # lower boundary present (1 -> row 0), upper absent (8 -> untouched)
        return np.array([1.0, 2.0, 8.0], np.float32)
    if case == "fused_vec4":                              # lower boundary absent (0 -> untouched), upper present (9 -> row 4)
        return np.array([0.0, 6.0, 9.0], np.float32)
    lab = np.random.default_rng(7).integers(0, 10, 2049).astype(np.float32)
    lab[lab == BUCKET_START] = BUCKET_START + 1           # lower boundary absent, upper present
    assert (lab < BUCKET_START).any() and (lab > BUCKET_NUM - 1).any() and (lab == BUCKET_NUM - 1).any()
    return lab


@pytest.mark.parametrize("case,b,c", [
    ("fused_scalar", 3, 7),
    ("fused_vec4", 3, 8),
    ("bin_index_then_rows", 2049, 8),                     # past SMOOTH_FUSED_MAX_B, below the LDS threshold
])
def test_smooth_fwd_forms(case, b, c):
    from dirhip import ops
    nb = BUCKET_NUM - BUCKET_START
    rng = np.random.default_rng(1000 * b + c)
    m1, s, m2 = make_tables(rng, nb, c)
    labels = _smooth_labels(case)
    x = rng.normal(0, 1, (b, c)).astype(np.float32)
    xd = dev(x)
    bins = ops.smooth_fwd_(xd, dev(labels), BUCKET_START, BUCKET_NUM, dev(m1), dev(s), dev(m2))[:b].cpu().numpy()
    want_bins = fds_oracle.bin_index(labels, BUCKET_START, BUCKET_NUM)
    assert (want_bins < 0).any() and (want_bins >= 0).any()
    assert np.array_equal(bins, want_bins)
    assert np.array_equal(xd.cpu().numpy(), fwd_ref(x, want_bins, m1, s, m2))


# ---- NCHW, forward and backward --------------------------------------------------------------------
@pytest.mark.parametrize("shape,nb,bin_values", [
    ((2, 3, 5, 820), 5, None),                            # plane chunks: HW = 4100, two chunks, the second holds four pixels
    ((1, 32, 4, 4), 129, (0, 64, 128, -1)),               # nb > 128: channel-group kernel
])
def test_nchw_forms_fwd_bwd(shape, nb, bin_values):
    from dirhip import ops
    n, c, h, w = shape
    rng = np.random.default_rng(n * c * h * w + nb)
    m1, s, m2 = make_tables(rng, nb, c)
    if bin_values is None:
        bins = make_bins(rng, n * h * w, nb)
        bins[-4:] = (nb - 1, -1, 0, 1)                    # the four pixels of the last chunk
    else:
        bins = rng.choice(np.array(bin_values, np.int32), n * h * w).astype(np.int32)
        bins[:4] = bin_values
    x = rng.normal(0, 1, shape).astype(np.float32)
    g = rng.normal(0, 1, shape).astype(np.float32)
    dbins, ds = dev(bins), dev(s)
    xd = dev(x)
    y = ops.calibrate_nchw(xd, dbins, dev(m1), ds, dev(m2))
    assert y is not None
    assert np.array_equal(xd.cpu().numpy(), x)
    assert np.array_equal(y.cpu().numpy(), from_rows(fwd_ref(to_rows(x), bins, m1, s, m2), shape))
    dx = ops.calibrate_bwd_nchw(dev(g), dbins, ds)
    assert dx is not None
    assert np.array_equal(dx.cpu().numpy(), from_rows(bwd_ref(to_rows(g), bins, s), shape))


# ---- multiplier table: dir_fds_prepare_scale == dir_fds_prepare_scale_ex(mode 0) == oracle ---------
@pytest.mark.parametrize("c", [5, 300])
def test_prepare_scale_both_entries(c):
    from dirhip import _lib as L
    nb = 4
    rng = np.random.default_rng(c)
    v1 = rng.uniform(0.5, 2, (nb, c)).astype(np.float32)
    v2 = rng.uniform(0.01, 30, (nb, c)).astype(np.float32)     # quotients on both sides of the clip [0.1, 10]
    v1[0] = 0.0                                           # zero-sum row
    v1[1] = 1e-15                                         # sum below 1e-10
    v1[2, 0] = 0.0
    v1[3, ::3] = 0.0                                      # zero columns
    v2[2, 1] = np.nan
    d1, d2 = dev(v1), dev(v2)
    a, b = torch.empty_like(d1), torch.empty_like(d1)
    L.check(L.lib().dir_fds_prepare_scale(L.ptr(d1), L.ptr(d2), nb, c, 0.1, 10.0, L.ptr(a), L.stream_ptr(d1.device)),
            "dir_fds_prepare_scale")
    L.check(L.lib().dir_fds_prepare_scale_ex(L.ptr(d1), L.ptr(d2), nb, c, 0.1, 10.0, 0, L.ptr(b), L.stream_ptr(d1.device)),
            "dir_fds_prepare_scale_ex")
    want = np.stack([fds_oracle.calibrate_scale(v1[r], v2[r], 0.1, 10.0) for r in range(nb)])
    assert np.isnan(want[2, 1]) and (want[0] == -1).all() and (want[1] == -1).all() and (want[3, ::3] == -1).all()
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    assert np.array_equal(a.cpu().numpy(), want, equal_nan=True)


# ---- finalize: one group per bin == the per-bin entry ----------------------------------------------
@pytest.mark.parametrize("c", [5, 300])
@pytest.mark.parametrize("factor_mode", [0, 1, 2])
def test_finalize_update_equals_groups_with_identity_bin_ptr(c, factor_mode):
    from dirhip import ops
    nb = 4
    rng = np.random.default_rng(10 * c + factor_mode)
    count = dev(np.array([0, 1, 3, 2], np.float64))
    mean = dev(rng.normal(0, 1, (nb, c)))
    m2 = dev(rng.uniform(0, 4, (nb, c)))
    rm0 = rng.normal(0, 1, (nb, c)).astype(np.float32)
    rv0 = rng.uniform(0.5, 2, (nb, c)).astype(np.float32)
    tr0 = np.array([3, 0, 5, 7], np.float32)
    rm_a, rv_a, tr_a = dev(rm0), dev(rv0), dev(tr0)
    rm_b, rv_b, tr_b = dev(rm0), dev(rv0), dev(tr0)
    ops.finalize_update(count, mean, m2, factor_mode, 0.9, rm_a, rv_a, tr_a)
    ops.finalize_update_groups(count, mean, m2, dev(np.arange(nb + 1, dtype=np.int32)), factor_mode, 0.9, rm_b, rv_b, tr_b)
    for a, b, start in ((rm_a, rm_b, rm0), (rv_a, rv_b, rv0), (tr_a, tr_b, tr0)):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(a, b)
        assert np.array_equal(a[0], start[0])             # the empty bin keeps its rows
        assert not np.array_equal(a[1:], start[1:])
