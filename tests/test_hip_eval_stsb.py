"""GPU tests of the STS-B-DIR evaluator (``dir_stsb_eval`` / ``dirhip.eval_stsb.STSShotAverage``) and of the ``sts-b-dir/loss.py``
drop-in, against the numpy / Python-int restatement of tests/stsb_eval_reference.py and the reference's recorded dicts
(tests/golden/stsb_eval_ref.npz). The rank table is compared as integers, the moment table at the derived reordering bound."""
import os

import numpy as np
import pytest
import torch

import stsb_eval_reference as R
from conftest import GOLDEN, assert_close
from test_stsb_host import CASES, assert_rows_match

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513, 1000)          # one below, at and above a wavefront, a workgroup tile, two tiles; the dev set


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "stsb_eval_ref.npz"))


@pytest.fixture(scope="module")
def tables():
    dev = torch.device("cuda")
    return torch.tensor(R.edges(), device=dev), torch.tensor(R.group_of_bin(), device=dev)


def run(pred, label, tables):
    """numpy float32 pred / label -> (moments [4, 10] float64, ranks [4][5] python ints) from the device."""
    from dirhip import ops
    p, l = torch.tensor(np.asarray(pred, np.float32), device="cuda"), torch.tensor(np.asarray(label, np.float32), device="cuda")
    m, r = ops.stsb_eval(p, l, *tables)
    return m.cpu().numpy(), [[int(v) for v in row] for row in r.cpu().numpy()]


def inputs(kind, n, g):
    """The input families of the issue; ``dev`` cut or tiled to n samples."""
    rng = np.random.default_rng(1000 + n)
    idx = np.arange(n) % 1000
    label, pred = g["dev_label"][idx].copy(), g["dev_pred"][idx].copy()
    if kind == "dev":
        pass
    elif kind == "pred_equal":
        pred[:] = np.float32(0.37)
    elif kind == "one_bin":
        label = rng.uniform(2.0, 2.09, n).astype(np.float32)                     # bin 20 (many) only: two groups are empty
    elif kind == "permutation":
        pred = (rng.permutation(n).astype(np.float32) + 0.5) / np.float32(n)     # no two equal
    elif kind == "on_edges":
        label = R.edges()[rng.integers(0, 51, n)].copy()                         # exactly on edges, 5.0 among them
        label[0] = np.float32(5.0)
    return pred, label


@pytest.mark.parametrize("n", SIZES)
def test_rank_table_is_exact(n, g, tables):
    for kind in ("dev", "pred_equal", "one_bin", "permutation", "on_edges"):
        pred, label = inputs(kind, n, g)
        m, r = run(pred, label, tables)
        assert r == R.rank_table(pred, label), (kind, n)
        assert m[:, 0].tolist() == R.moment_table(pred, label)["table"][:, 0].tolist(), (kind, n)
        perm = np.random.default_rng(n).permutation(n)                           # the order of the samples changes no bit of the table
        assert run(pred[perm], label[perm], tables)[1] == r, (kind, n)


@pytest.mark.parametrize("n", SIZES)
def test_moment_table_within_the_reordering_bound(n, g, tables):
    for kind in ("dev", "on_edges", "one_bin"):
        pred, label = inputs(kind, n, g)
        if kind == "dev" and n >= 8:
            pred[3] = label[3] / np.float32(5)                                   # zero errors where 5 * pred == label exactly
            label[5], pred[5] = np.float32(2.5), np.float32(0.5)
        want = R.moment_table(pred, label)
        m, _ = run(pred, label, tables)
        assert np.array_equal(m[:, :2], want["table"][:, :2]), (kind, n)         # the counts are exact
        diff = np.abs(m[:, 2:] - want["table"][:, 2:])
        print(kind, n, "max |diff| / bound", float(np.max(diff / np.maximum(want["bound"][:, 2:], 1e-300))))
        assert (diff <= want["bound"][:, 2:]).all(), (kind, n, diff, want["bound"][:, 2:])
        again, _ = run(pred, label, tables)
        assert np.array_equal(m.view(np.uint64), again.view(np.uint64)), (kind, n)       # two runs: bit-identical


def test_unaligned_views_give_the_same_tables(g, tables):
    """The kernels load element-wise; views that start 1 to 3 elements into a buffer must not change a bit."""
    from dirhip import ops
    pred, label = g["dev_pred"], g["dev_label"]
    want_m, want_r = run(pred, label, tables)
    for off in (1, 2, 3):
        p = torch.zeros(1000 + off, device="cuda")
        l = torch.zeros(1000 + off + 1, device="cuda")
        p[off:] = torch.tensor(pred, device="cuda")
        l[off + 1:] = torch.tensor(label, device="cuda")
        m, r = ops.stsb_eval(p[off:], l[off + 1:], *tables)
        assert np.array_equal(m.cpu().numpy().view(np.uint64), want_m.view(np.uint64)), off
        assert [[int(v) for v in row] for row in r.cpu().numpy()] == want_r, off


def test_many_tiles_and_large_counters(tables):
    """n = 8192 with 50-valued labels: 32 tiles, counters and doubled ranks past 2^13, against ``np.searchsorted`` ranks."""
    rng = np.random.default_rng(8192)
    label = (rng.integers(0, 50, 8192) / 10).astype(np.float32)
    pred = np.round(np.clip(label / 5 + rng.normal(0, 0.1, 8192), 0, 1), 3).astype(np.float32)
    m, r = run(pred, label, tables)
    assert r == R.rank_table(pred, label)
    assert max(r[3][0], r[3][1]) == 8192 * 8193                                  # sum of doubled ranks = n (n + 1), ties or not
    assert m[:, 0].tolist() == R.moment_table(pred, label)["table"][:, 0].tolist()


def _feed(ev, pred, label, batch):
    for a in range(0, len(pred), batch):
        ev(torch.tensor(pred[a:a + batch], device="cuda"), torch.tensor(label[a:a + batch], device="cuda").view(-1, 1))


def test_shot_average_matches_the_reference_dicts(g):
    from dirhip.eval_stsb import STSShotAverage
    for case in CASES:
        pred, label = g[f"{case}_pred"], g[f"{case}_label"]
        ev = STSShotAverage(metric=R.ALL_METRICS)
        _feed(ev, pred, label, len(pred))
        one = ev.get_metric()
        worst = assert_rows_match(R.as_rows(one), g[f"{case}_dict"], case)
        print(case, {k: f"{v:.3e}" for k, v in worst.items()})
        assert ev.get_metric(type='overall') == one['overall']
        for batch in (1, 7, 256):
            if batch == 1 and len(pred) > 100:
                continue                                                         # 1000 single-sample appends add nothing over 65 of them
            again = STSShotAverage(metric=R.ALL_METRICS)
            _feed(again, pred, label, batch)
            assert again.get_metric() == one, (case, batch)                      # bit-identical, however the set arrived
        assert ev.get_metric(reset=True) == one
        assert ev.get_metric()['overall']['num_samples'] == 0
        _feed(ev, pred[:65], label[:65], 65)
        assert ev.get_metric()['overall']['num_samples'] == 65
    assert g["nomed_dict"][1, 5] == 0                                            # 'nomed': the empty group gave 0 above


def test_shot_average_edge_cases():
    from dirhip._lib import DirHipError
    from dirhip.eval_stsb import STSShotAverage
    ev = STSShotAverage(metric=R.ALL_METRICS)
    label = np.array([0.0, 0.05, 0.2, 0.25, 0.3], np.float32)                     # many, many, medium, medium, few
    pred = np.array([0.1, 0.1, 0.04, 0.05, 0.5], np.float32)
    _feed(ev, pred, label, 5)
    d = ev.get_metric()
    assert np.isnan(d['many']['pearsonr']) and np.isnan(d['many']['spearmanr'])   # a constant group: nan, as scipy
    assert d['few']['pearsonr'] == 0. and d['few']['spearmanr'] == 0. and d['few']['num_samples'] == 1
    assert d['medium']['spearmanr'] == 1.0
    only = STSShotAverage(metric=['mse', 'spearmanr'])
    _feed(only, pred[:2], label[:2], 2)
    assert only.get_metric()['medium'] == {'mse': 0., 'spearmanr': 0., 'num_samples': 0}      # an empty group: 0
    for bad_label, bad_pred in ((5.001, 0.5), (-0.001, 0.5), (np.nan, 0.5), (1.0, np.nan)):
        ev = STSShotAverage(metric=R.ALL_METRICS)
        _feed(ev, np.array([0.2, bad_pred, 0.4], np.float32), np.array([1.0, bad_label, 3.0], np.float32), 3)
        with pytest.raises(DirHipError, match="1 of 3 samples"):
            ev.get_metric()
    with pytest.raises(TypeError):
        ev(torch.ones(3, device="cuda", dtype=torch.float64), torch.ones(3, device="cuda"))
    with pytest.raises(DirHipError, match="at most 65536"):
        big = STSShotAverage(metric=['mse'])
        big(torch.zeros(65537, device="cuda"), torch.zeros(65537, device="cuda"))


@pytest.mark.parametrize("B", [1, 8, 256])
def test_stsb_losses_match_torch_compositions(B):
    """sts-b-dir/loss.py with its own defaults (huber beta=0.5, focal beta=20.) and [B, 1] weights against the reference's torch
    compositions on the CPU (in float64), at the bars test_hip_parity.py holds losses.npz to (assert_close rtol 1e-5, atol_scale 1e-6)."""
    from dirhip import loss_stsb
    rng = np.random.default_rng(B)
    x = torch.tensor(rng.uniform(0, 1, (B, 1)).astype(np.float32))
    y = torch.tensor(rng.uniform(0, 5, (B, 1)).astype(np.float32) / 5)
    y[0] = x[0] + 0.7                                                            # one sample surely on the linear side of huber beta=0.5
    w = torch.tensor(rng.uniform(0.2, 3.0, (B, 1)).astype(np.float32))

    def focal(base, xx, beta=20., gamma=1):
        return base * (2 * torch.sigmoid(beta * torch.abs(xx - y)) - 1) ** gamma

    def huber(xx, beta=0.5):
        e = torch.abs(xx - y)
        return torch.where(e < beta, 0.5 * e ** 2 / beta, e - 0.5 * beta)

    compositions = {
        "weighted_mse_loss": lambda xx: (xx - y) ** 2,
        "weighted_l1_loss": lambda xx: torch.abs(xx - y),
        "weighted_huber_loss": huber,
        "weighted_focal_mse_loss": lambda xx: focal((xx - y) ** 2, xx),
        "weighted_focal_l1_loss": lambda xx: focal(torch.abs(xx - y), xx),
    }
    for name, comp in compositions.items():
        for weights in (None, w):
            xc = x.double().requires_grad_(True)
            ref = comp(xc)
            if weights is not None:
                ref = ref * weights.double()
            ref = ref.mean()
            ref.backward()
            xg = x.cuda().requires_grad_(True)
            got = getattr(loss_stsb, name)(xg, y.cuda(), None if weights is None else weights.cuda())
            got.backward()
            assert_close(float(got), float(ref), rtol=1e-5, atol_scale=1e-6, msg=f"{name} B={B} value")
            assert_close(xg.grad.cpu().numpy(), xc.grad.numpy(), rtol=1e-5, atol_scale=1e-6, msg=f"{name} B={B}")
    # the STS-B defaults are not the age projects': the same inputs give other values under dirhip.loss
    from dirhip import loss as age_loss
    if B > 1:
        for name in ("weighted_huber_loss", "weighted_focal_mse_loss", "weighted_focal_l1_loss"):
            a, s = getattr(age_loss, name)(x.cuda(), y.cuda(), w.cuda()), getattr(loss_stsb, name)(x.cuda(), y.cuda(), w.cuda())
            assert abs(float(a) - float(s)) > 1e-3 * abs(float(s)), name
