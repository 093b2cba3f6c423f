"""-m gpu: the fused STS-B-DIR pair head (dir_pair_tail_fwd / dir_pair_tail_bwd, dirhip.pair_tail) against the numpy restatement of
tests/pair_tail_reference.py: emb, arg1, arg2, ds1, ds2 bit for bit against its float32 form on every shape, with and without
calibration and dropout; logits, dweight, dbias against float64 within the bound of a reordered float32 sum; determinism; the rules
of include/dir_hip.h one by one; PairHead end to end against float64 autograd."""
import functools

import numpy as np
import pytest
import torch

import pair_tail_reference as R
from conftest import assert_close

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24                                                  # unit roundoff of float32
# (B, T1, T2, D): one element; the element-wise path (D % 4 != 0); 16-byte path, T1 != T2; the product width (three column tiles, the
# last one partial); more samples than one batch slice of the dweight reduction (29 slices of 9 rows, the last one short)
SHAPES = [(1, 1, 1, 1), (3, 5, 2, 6), (2, 4, 7, 8), (3, 5, 3, 3000), (257, 3, 2, 64)]
SEED, OFF1, OFF2 = 0x1234_5678_9abc, 8, 2 ** 32 + 12
NB = 7


@pytest.fixture(autouse=True)
def _restore_global_rng():
    """PairHead draws from torch's global generators; later test files draw their weights from them."""
    with torch.random.fork_rng(devices=[torch.cuda.current_device()]):
        yield


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bit_equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(bits(got), bits(want)), (what, int((bits(got) != bits(want)).sum()), got.size)


@functools.lru_cache(maxsize=None)
def case(shape, calib, p):
    """Inputs of one case (numpy, computed once and never written to): random encodings, masks with prefixes and holes, tables with
    untouched rows and columns, and the keep masks of (SEED, OFF1 / OFF2, p) from the device."""
    from dirhip.tail import dropout_mask
    b, t1, t2, d = shape
    rng = np.random.default_rng(b * 1000 + d)
    c = dict(s1=rng.normal(0, 1, (b, t1, d)).astype(np.float32), s2=rng.normal(0, 1, (b, t2, d)).astype(np.float32),
             weight=rng.normal(0, 0.3, 4 * d).astype(np.float32), bias=rng.normal(0, 0.3, 1).astype(np.float32),
             dlogits=rng.normal(0, 1, b).astype(np.float32), demb=rng.normal(0, 0.1, (b, 4 * d)).astype(np.float32))
    for k, t in (("mask1", t1), ("mask2", t2)):
        m = np.arange(t)[None, :] < rng.integers(1, t + 1, b)[:, None]
        m &= rng.random((b, t)) < 0.7                              # holes
        m[np.arange(b), rng.integers(0, t, b)] = True
        c[k] = m
    c["keep1"] = c["keep2"] = None
    c["factor"] = R.keep_factor(p)
    c["drop"] = None
    if p:
        dev = torch.device("cuda")
        c["keep1"] = dropout_mask(SEED, OFF1, p, b * t1, d, dev).cpu().numpy().reshape(b, t1, d)
        c["keep2"] = dropout_mask(SEED, OFF2, p, b * t2, d, dev).cpu().numpy().reshape(b, t2, d)
        c["drop"] = (SEED, OFF1, OFF2, p)
    c["bins"] = c["m1"] = c["scale"] = c["m2"] = None
    if calib:
        c["bins"] = rng.integers(-1, NB, b).astype(np.int32)
        c["bins"][0] = NB - 1
        if b > 1:
            c["bins"][1] = -1
        c["m1"], c["m2"] = rng.normal(0, 1, (NB, 4 * d)).astype(np.float32), rng.normal(0, 1, (NB, 4 * d)).astype(np.float32)
        c["scale"] = rng.uniform(0.5, 2.0, (NB, 4 * d)).astype(np.float32)
        c["scale"][:, ::3] = -1.0
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def gpu_run(c, with_demb=True, calib=True, drop="case", backward=True):
    """One forward (+ backward) of dirhip.pair_tail.pair_tail_apply on the case's tensors -> numpy outputs."""
    from dirhip.pair_tail import pair_tail_apply
    dev = torch.device("cuda")
    t = lambda a: None if a is None else torch.tensor(a, device=dev)
    s1, s2 = t(c["s1"]).requires_grad_(True), t(c["s2"]).requires_grad_(True)
    w, bias = t(c["weight"]).reshape(1, -1).requires_grad_(True), t(c["bias"]).requires_grad_(True)
    tables = [t(c[k]) for k in ("bins", "m1", "scale", "m2")] if calib else [None] * 4
    logits, emb, arg1, arg2 = pair_tail_apply(s1, s2, t(c["mask1"]), t(c["mask2"]), w, bias, *tables,
                                              drop=c["drop"] if drop == "case" else drop)
    out = dict(logits=logits.detach().cpu().numpy().reshape(-1), emb=emb.detach().cpu().numpy(), arg1=arg1.cpu().numpy(),
               arg2=arg2.cpu().numpy())
    assert logits.shape == (c["s1"].shape[0], 1) and not arg1.requires_grad
    if backward:
        obj = (logits.reshape(-1) * t(c["dlogits"])).sum()
        if with_demb:
            obj = obj + (emb * t(c["demb"])).sum()
        obj.backward()
        out.update(ds1=s1.grad.cpu().numpy(), ds2=s2.grad.cpu().numpy(), dweight=w.grad.cpu().numpy().reshape(-1),
                   dbias=bias.grad.cpu().numpy().reshape(-1))
    return out


def restated(c, with_demb=True, calib=True, dtype=np.float32):
    kw = dict(keep1=c["keep1"], keep2=c["keep2"], factor=c["factor"], bins=c["bins"] if calib else None)
    fw = R.forward(c["s1"], c["s2"], c["mask1"], c["mask2"], c["weight"], c["bias"], m1=c["m1"], scale=c["scale"], m2=c["m2"],
                   dtype=dtype, **kw)
    bw = R.backward(fw, c["dlogits"], c["weight"], c["s1"].shape[1], c["s2"].shape[1], demb=c["demb"] if with_demb else None,
                    scale=c["scale"], dtype=dtype, **kw)
    return fw, bw


def assert_elementwise_bit_equal(got, fw, bw, what):
    for k in ("emb", "arg1", "arg2"):
        assert_bit_equal(got[k], fw[k], (what, k))
    for k in ("ds1", "ds2"):
        assert_bit_equal(got[k], bw[k], (what, k))


def assert_sums_within_reordering_bound(got, c, what):
    """logits / dweight / dbias against float64 sums of the SAME float32 terms (the bit-checked emb of the device). A float32 sum of n
    terms, each the rounded product of two float32 numbers, added in any order (plus one more addend for the bias) is within
    (n + 2) * 2^-24 * sum |term| of the exact sum to first order: one rounding per product, at most n per partial-sum chain, one for
    the bias. Derived, not measured; printed before the assertion."""
    emb, w, dl = got["emb"].astype(np.float64), c["weight"].astype(np.float64), c["dlogits"].astype(np.float64)
    b, k = emb.shape
    terms = emb * w[None, :]
    want, bound = terms.sum(axis=1) + float(c["bias"][0]), (k + 2) * U32 * (np.abs(terms).sum(axis=1) + abs(float(c["bias"][0])))
    err = np.abs(got["logits"] - want)
    print(what, "logits: worst err / bound", float((err / bound).max()))
    assert (err <= bound).all(), (what, "logits", float((err / bound).max()))
    terms = dl[:, None] * emb
    want, bound = terms.sum(axis=0), (b + 2) * U32 * np.abs(terms).sum(axis=0)
    err = np.abs(got["dweight"] - want)
    print(what, "dweight: worst err / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (what, "dweight", float((err / np.maximum(bound, 1e-300)).max()))
    want, bound = dl.sum(), (b + 2) * U32 * np.abs(dl).sum()
    err = abs(float(got["dbias"][0]) - want)
    print(what, "dbias: err / bound", err / bound)
    assert err <= bound, (what, "dbias", err, bound)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("calib", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_bit_equal_to_float32_restatement_and_sums_within_bound(shape, calib, p):
    from dirhip import ops
    c = case(shape, calib, p)
    got = gpu_run(c, calib=calib)
    fw, bw = restated(c, calib=calib)
    assert_elementwise_bit_equal(got, fw, bw, (shape, calib, p))
    assert_sums_within_reordering_bound(got, c, (shape, calib, p))
    if calib:                                                    # emb = the package's own calibration kernel on the uncalibrated emb
        raw = gpu_run(c, calib=False, backward=False)["emb"]
        assert_bit_equal(raw, fw["f"], "uncalibrated emb")
        dev = torch.device("cuda")
        via = ops.calibrate_fwd_(torch.tensor(raw, device=dev), torch.tensor(c["bins"], device=dev), torch.tensor(c["m1"], device=dev),
                                 torch.tensor(c["scale"], device=dev), torch.tensor(c["m2"], device=dev))
        assert_bit_equal(got["emb"], via.cpu().numpy(), "emb vs dir_fds_calibrate_fwd")
        assert not np.array_equal(got["emb"], raw)


@pytest.mark.parametrize("shape", [(3, 5, 3, 3000), (257, 3, 2, 64)])
def test_two_runs_are_bit_identical(shape):
    c = case(shape, True, 0.5)
    a, b = gpu_run(c), gpu_run(c)
    assert a.keys() == b.keys() and len(a) == 8
    for k in a:
        assert_bit_equal(a[k], b[k], k)


@pytest.mark.parametrize("shape", [(3, 5, 2, 6), (2, 4, 7, 8)])
@pytest.mark.parametrize("with_demb", [True, False])
def test_demb_given_or_none(shape, with_demb):
    c = case(shape, True, 0.5)
    got = gpu_run(c, with_demb=with_demb)
    fw, bw = restated(c, with_demb=with_demb)
    assert_elementwise_bit_equal(got, fw, bw, (shape, with_demb))
    other = gpu_run(c, with_demb=not with_demb)
    assert not np.array_equal(got["ds1"], other["ds1"])


def _plain_case(b, t1, t2, d, seed=0):
    rng = np.random.default_rng(seed)
    return dict(s1=rng.normal(0, 1, (b, t1, d)).astype(np.float32), s2=rng.normal(0, 1, (b, t2, d)).astype(np.float32),
                mask1=np.ones((b, t1), bool), mask2=np.ones((b, t2), bool), weight=rng.normal(0, 0.3, 4 * d).astype(np.float32),
                bias=rng.normal(0, 0.3, 1).astype(np.float32), dlogits=rng.normal(0, 1, b).astype(np.float32),
                demb=rng.normal(0, 0.1, (b, 4 * d)).astype(np.float32), keep1=None, keep2=None, factor=np.float32(1.0), drop=None,
                bins=None, m1=None, scale=None, m2=None)


def test_tie_sends_the_gradient_to_the_lowest_unmasked_t():
    c = _plain_case(2, 5, 3, 8)
    c["s1"][:, 1:, :4] = 2.5                                       # columns 0..3: the maximum at t = 1, 2, 3, 4 (and t = 0 where larger)
    c["s1"][:, 0, :4] = 9.0
    c["mask1"][:, 0] = False                                       # ... but t = 0 is padding
    got = gpu_run(c, calib=False)
    fw, bw = restated(c, calib=False)
    assert_elementwise_bit_equal(got, fw, bw, "tie")
    assert (got["arg1"][:, :4] == 1).all() and (got["emb"][:, :4] == 2.5).all()
    nz = got["ds1"] != 0
    assert (nz.sum(axis=1) == 1).all() and nz[:, 1, :4].all()      # exactly one position per (sample, column) ...
    assert_bit_equal(got["ds1"].sum(axis=1), bw["du"], "du")        # ... and it holds du (the other addends are +0)
    assert (bw["du"] != 0).all()


def test_nan_propagates_from_an_unmasked_position_only():
    c = _plain_case(2, 4, 3, 6)
    c["s1"][0, 2, 1] = np.nan                                      # unmasked: u[0, 1] is NaN, arg = 2
    c["s1"][0, 3, 1] = np.nan                                      # a later NaN does not move the argmax
    c["s1"][1, 1, 2] = np.nan                                      # masked: never looked at
    c["mask1"][1, 1] = False
    c["s2"][1, 0, 0] = np.nan                                      # masked in sentence 2
    c["mask2"][1, 0] = False
    got = gpu_run(c, calib=False, backward=False)
    fw, _ = restated(c, calib=False)
    d = 6
    assert np.isnan(got["emb"][0, 1]) and got["arg1"][0, 1] == 2
    assert np.array_equal(np.isnan(got["emb"]), np.isnan(fw["emb"])) and np.isnan(got["emb"]).sum() == 3     # u, |u - v|, u * v of that column
    assert np.isnan(got["emb"][0, [1, 2 * d + 1, 3 * d + 1]]).all() and np.isnan(got["logits"][0]) and np.isfinite(got["logits"][1])
    assert np.array_equal(got["emb"], fw["emb"], equal_nan=True)
    assert np.array_equal(got["arg1"], fw["arg1"]) and np.array_equal(got["arg2"], fw["arg2"])


def test_sample_with_an_empty_mask():
    c = _plain_case(3, 4, 3, 8)
    full = gpu_run(c, calib=False)
    c["mask1"][1, :] = False
    c["mask2"][1, :] = False
    got = gpu_run(c, calib=False)
    d = 8
    assert np.isneginf(got["emb"][1, :2 * d]).all()                # u = v = -inf
    assert (got["arg1"][1] == -1).all() and (got["arg2"][1] == -1).all()
    assert not bits(got["ds1"][1]).any() and not bits(got["ds2"][1]).any()      # exactly +0, not -0 or NaN
    for k in ("ds1", "ds2", "emb", "arg1", "arg2", "logits"):
        assert_bit_equal(got[k][[0, 2]], full[k][[0, 2]], k)        # the other samples: unchanged
    fw, bw = restated(c, calib=False)
    assert_bit_equal(got["ds1"], bw["ds1"], "ds1")
    assert_bit_equal(got["ds2"], bw["ds2"], "ds2")
    assert np.array_equal(got["emb"], fw["emb"], equal_nan=True)
    one_side = _plain_case(3, 4, 3, 8)
    one_side["mask1"][1, :] = False                                # only sentence 1 empty: u = -inf, v finite, ds1 row zero
    got = gpu_run(one_side, calib=False)
    assert np.isneginf(got["emb"][1, :d]).all() and np.isfinite(got["emb"][1, d:2 * d]).all() and not bits(got["ds1"][1]).any()


def test_all_negative_encodings_put_the_maximum_at_a_dropped_element():
    shape = (3, 5, 2, 6)
    c = dict(case(shape, False, 0.5))
    c["s1"] = -np.abs(c["s1"]) - 0.1
    c["mask1"] = np.ones_like(c["mask1"])
    got = gpu_run(c, calib=False)
    fw, bw = restated(c, calib=False)
    assert_elementwise_bit_equal(got, fw, bw, "all negative")
    some_dropped = ~c["keep1"].all(axis=1)                          # [B, D]: a dropped element exists in the column
    assert some_dropped.sum() >= 4
    assert (got["emb"][:, :6][some_dropped] == 0).all() and (got["emb"][:, :6][~some_dropped] < 0).all()
    first_dropped = np.argmin(c["keep1"], axis=1)
    assert (got["arg1"][some_dropped] == first_dropped[some_dropped]).all()
    assert not got["ds1"].transpose(0, 2, 1)[some_dropped].any()    # the maximum was a dropped element: no gradient in the column
    assert (got["ds1"].transpose(0, 2, 1)[~some_dropped] != 0).sum() == (~some_dropped).sum()


def test_untouched_rows_and_columns_stay_untouched():
    shape = (3, 5, 2, 6)
    c = case(shape, True, 0.0)
    assert c["bins"][1] == -1 and c["bins"][0] >= 0 and (c["scale"][:, ::3] == -1).all()
    cal, raw = gpu_run(c, calib=True), gpu_run(c, calib=False)
    assert_bit_equal(cal["emb"][1], raw["emb"][1], "row with bins = -1")
    assert_bit_equal(cal["emb"][:, ::3], raw["emb"][:, ::3], "columns with scale = -1")
    touched = np.ones(24, bool)
    touched[::3] = False
    assert (cal["emb"][0][touched] != raw["emb"][0][touched]).all()
    # backward: a row with bins = -1 gets the gradient of the uncalibrated head (same dlogits, weight and demb)
    assert_bit_equal(cal["ds1"][1], raw["ds1"][1], "ds1 of the untouched row")
    assert_bit_equal(cal["ds2"][1], raw["ds2"][1], "ds2 of the untouched row")
    assert not np.array_equal(cal["ds1"][0], raw["ds1"][0])
    # columns with scale = -1 in EVERY segment pass their gradient through: scale -1 on all of row 0's table -> the uncalibrated gradient
    c2 = dict(c)
    c2["scale"] = np.full_like(c["scale"], -1.0)
    off = gpu_run(c2, calib=True)
    for k in ("emb", "ds1", "ds2", "logits", "dweight"):
        assert_bit_equal(off[k], raw[k], k)


@pytest.mark.parametrize("shape", [(3, 5, 2, 6), (2, 4, 7, 8), (3, 5, 3, 3000)])
def test_p_zero_equals_the_entry_without_dropout(shape):
    c = case(shape, True, 0.0)
    plain, zero = gpu_run(c, drop=None), gpu_run(c, drop=(SEED, OFF1, OFF2, 0.0))
    for k in plain:
        assert_bit_equal(zero[k], plain[k], k)
    half = gpu_run(c, drop=(SEED, OFF1, OFF2, 0.5), backward=False)
    assert not np.array_equal(half["emb"], plain["emb"])


def _head_setup(loss, d=6, b=16, t1=5, t2=4):
    from dirhip.fds_stsb import FDS
    from dirhip.pair_tail import PairHead
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(11)
    fds = FDS(feature_dim=4 * d, bucket_num=50).cuda()
    lab_all = (torch.randint(0, 26, (400,), device=dev, generator=g).float() / 5)
    fds.update_running_stats(torch.randn(400, 4 * d, device=dev, generator=g) * (0.5 + lab_all[:, None] / 5) + 0.1 * lab_all[:, None], lab_all, 0)
    fds.update_last_epoch_stats(1)
    torch.manual_seed(3)
    head = PairHead(d, fds=fds, loss=loss, dropout=0.5).cuda()
    rng = np.random.default_rng(5)
    c = dict(s1=rng.normal(0, 1, (b, t1, d)).astype(np.float32), s2=rng.normal(0, 1, (b, t2, d)).astype(np.float32))
    for k, t in (("mask1", t1), ("mask2", t2)):
        c[k] = np.arange(t)[None, :] < rng.integers(1, t + 1, b)[:, None]
    label = (rng.integers(0, 26, (b, 1)) / 5).astype(np.float32)
    label[0, 0], label[1, 0] = 5.0, 0.0
    c["label"], c["lw"] = label, rng.uniform(0.5, 2.0, (b, 1)).astype(np.float32)
    return head, fds, c


def _head_gpu(head, c, epoch):
    dev = torch.device("cuda")
    s1, s2 = torch.tensor(c["s1"], device=dev, requires_grad=True), torch.tensor(c["s2"], device=dev, requires_grad=True)
    head.zero_grad()
    out = head(s1, s2, torch.tensor(c["mask1"], device=dev).long(), torch.tensor(c["mask2"], device=dev).long(),
               torch.tensor(c["label"], device=dev), epoch=epoch, weight=torch.tensor(c["lw"], device=dev))
    return out, s1, s2


@pytest.mark.parametrize("loss", ["mse", "huber"])
def test_pair_head_end_to_end_against_float64_autograd(loss):
    from dirhip.tail import dropout_mask
    head, fds, c = _head_setup(loss)
    dev = torch.device("cuda")
    b, t1, d = c["s1"].shape
    t2 = c["s2"].shape[1]
    head.train()
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    torch.cuda.manual_seed(77)
    seed, off = gen.initial_seed(), gen.get_offset()
    out, s1, s2 = _head_gpu(head, c, epoch=1)
    assert gen.get_offset() == off + 8                              # two masks, one Philox counter block each
    assert set(out) == {"logits", "loss", "embs", "labels"} and out["logits"].shape == (b, 1) and out["embs"].shape == (b, 4 * d)
    out["loss"].backward()
    # float64 autograd of the restated chain on the same tables, bins and masks
    keep1 = dropout_mask(seed, off, 0.5, b * t1, d, dev).cpu().numpy().reshape(b, t1, d)
    keep2 = dropout_mask(seed, off + 4, 0.5, b * t2, d, dev).cpu().numpy().reshape(b, t2, d)
    bins = fds._bins(torch.tensor(c["label"], device=dev)).cpu().numpy()
    assert bins[0] == 49 and bins[1] == 0 and (bins >= 0).all()
    lin = head.pred_layer
    logits64, emb64, leaves = R.torch_chain64(c["s1"], c["s2"], c["mask1"], c["mask2"], lin.weight.detach().cpu().numpy(),
                                              lin.bias.detach().cpu().numpy(), keep1=keep1, keep2=keep2, factor=R.keep_factor(0.5),
                                              bins=bins, m1=fds.running_mean_last_epoch.cpu().numpy(),
                                              scale=fds._scale_table().cpu().numpy(), m2=fds.smoothed_mean_last_epoch.cpu().numpy())
    l64 = R.loss64(loss, logits64, torch.tensor(c["label"][:, 0], dtype=torch.float64) / 5, torch.tensor(c["lw"][:, 0], dtype=torch.float64),
                   beta=head.huber_beta)
    l64.backward()
    assert_close(out["embs"].detach().cpu().numpy(), emb64.detach().numpy(), msg="embs")
    assert_close(out["logits"].detach().cpu().numpy().reshape(-1), logits64.detach().numpy(), msg="logits")
    assert_close(np.asarray([out["loss"].item()]), np.asarray([l64.item()]), msg="loss")
    assert_close(s1.grad.cpu().numpy(), leaves["s1"].grad.numpy(), msg="ds1")
    assert_close(s2.grad.cpu().numpy(), leaves["s2"].grad.numpy(), msg="ds2")
    assert_close(lin.weight.grad.cpu().numpy().reshape(-1), leaves["weight"].grad.numpy(), msg="dweight")
    assert_close(lin.bias.grad.cpu().numpy(), leaves["bias"].grad.numpy(), msg="dbias")
    assert s1.grad.abs().sum() > 0 and out["labels"].shape == (b, 1)


def test_pair_head_tables_have_no_effect_before_start_smooth_or_in_eval():
    from dirhip.pair_tail import PairHead
    head, fds, c = _head_setup("mse")
    bare = PairHead(6, fds=None, dropout=0.5).cuda()
    bare.load_state_dict({k: v for k, v in head.state_dict().items() if k.startswith("pred_layer")})

    def run(h, epoch, train):
        h.train(train)
        torch.cuda.manual_seed(123)                                 # the same masks for every run
        out, s1, s2 = _head_gpu(h, c, epoch)
        out["loss"].backward()
        return out, s1.grad.clone(), s2.grad.clone()

    early, e1, e2 = run(head, 0, True)                               # training, epoch 0 < start_smooth = 1
    ref, r1, r2 = run(bare, 0, True)
    live, l1, _ = run(head, 1, True)
    assert "embs" in early and "embs" not in ref
    assert torch.equal(early["logits"], ref["logits"]) and torch.equal(early["loss"], ref["loss"]) and torch.equal(e1, r1) and torch.equal(e2, r2)
    assert not torch.equal(live["logits"], ref["logits"]) and not torch.equal(live["embs"], early["embs"])
    # eval mode: neither tables nor dropout, whatever the epoch; equal to a head without dropout bit for bit
    ev, v1, v2 = run(head, 5, False)
    nodrop = PairHead(6, fds=None, dropout=0).cuda()
    nodrop.load_state_dict(bare.state_dict())
    nd, n1, n2 = run(nodrop, 5, True)
    assert set(ev) == {"logits", "loss"}
    assert torch.equal(ev["logits"], nd["logits"]) and torch.equal(ev["loss"], nd["loss"]) and torch.equal(v1, n1) and torch.equal(v2, n2)
    assert not torch.equal(ev["logits"], ref["logits"])
