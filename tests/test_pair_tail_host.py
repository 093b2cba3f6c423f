"""CPU-side tests of the fused STS-B-DIR pair head: the float64 numpy restatement (tests/pair_tail_reference.py) against a plain torch
float64 autograd composition, values and every gradient; the three new C-ABI entry points (declared, bound, exported; the ABI version
stays 4); every argument error the header lists, returned before any HIP call; the drop-in module and the no-CPU-fallback rule."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import pair_tail_reference as R
from conftest import PKG, ROOT, assert_close

NEW_SYMBOLS = ("dir_pair_tail_workspace", "dir_pair_tail_fwd", "dir_pair_tail_bwd")
# Two float64 evaluations of the same chain that differ only in the order of a few additions (autograd adds the four shares of du in
# its own order; emb @ w is a BLAS dot) differ by at most about (K + 2) * 2^-53 of the sum of magnitudes, K = 4D <= 64 here: 8e-15.
# 1e-12 relative (plus 1e-13 of the array's scale for cancelled elements) leaves two orders of margin and is nine orders below any
# real disagreement (a wrong argmax, a missing scale factor, a swapped sign are errors of order 1).
TOL = dict(rtol=1e-12, atol_scale=1e-13)


def _case(b, t1, t2, d, holes, calib, p, seed):
    rng = np.random.default_rng(seed)
    c = dict(s1=rng.normal(0, 1, (b, t1, d)).astype(np.float32), s2=rng.normal(0, 1, (b, t2, d)).astype(np.float32),
             weight=rng.normal(0, 0.3, 4 * d).astype(np.float32), bias=rng.normal(0, 0.3, 1).astype(np.float32),
             dlogits=rng.normal(0, 1, b).astype(np.float32), demb=rng.normal(0, 0.1, (b, 4 * d)).astype(np.float32))
    for k, t in (("mask1", t1), ("mask2", t2)):
        n = rng.integers(1, t + 1, b)
        m = np.arange(t)[None, :] < n[:, None]                      # prefixes of length >= 1
        if holes:
            m &= rng.random((b, t)) < 0.6
            m[np.arange(b), rng.integers(0, t, b)] = True           # never empty: -inf - -inf would be NaN on both sides
        c[k] = m
    c["keep1"] = c["keep2"] = None
    c["factor"] = R.keep_factor(p)
    if p:
        c["keep1"], c["keep2"] = rng.random((b, t1, d)) >= p, rng.random((b, t2, d)) >= p
    c["bins"] = c["m1"] = c["scale"] = c["m2"] = None
    if calib:
        nb = 5
        c["bins"] = rng.integers(-1, nb, b).astype(np.int32)
        c["bins"][0] = -1
        c["m1"], c["m2"] = rng.normal(0, 1, (nb, 4 * d)).astype(np.float32), rng.normal(0, 1, (nb, 4 * d)).astype(np.float32)
        c["scale"] = rng.uniform(0.5, 2.0, (nb, 4 * d)).astype(np.float32)
        c["scale"][:, ::3] = -1.0
    return c


@pytest.mark.parametrize("b,t1,t2,d,holes", [(4, 5, 5, 6, False), (5, 6, 6, 7, True), (3, 4, 9, 8, True), (2, 1, 3, 1, False)])
@pytest.mark.parametrize("calib", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("with_demb", [False, True])
def test_float64_restatement_equals_torch_autograd(b, t1, t2, d, holes, calib, p, with_demb):
    c = _case(b, t1, t2, d, holes, calib, p, seed=b * 100 + d)
    kw = dict(keep1=c["keep1"], keep2=c["keep2"], factor=c["factor"], bins=c["bins"])
    fw = R.forward(c["s1"], c["s2"], c["mask1"], c["mask2"], c["weight"], c["bias"], m1=c["m1"], scale=c["scale"], m2=c["m2"],
                   dtype=np.float64, **kw)
    demb = c["demb"] if with_demb else None
    bw = R.backward(fw, c["dlogits"], c["weight"], t1, t2, demb=demb, scale=c["scale"], dtype=np.float64, **kw)
    logits, emb, leaves = R.torch_chain64(c["s1"], c["s2"], c["mask1"], c["mask2"], c["weight"], c["bias"], m1=c["m1"], scale=c["scale"],
                                          m2=c["m2"], **kw)
    out = (logits * torch.tensor(c["dlogits"], dtype=torch.float64)).sum()
    if with_demb:
        out = out + (emb * torch.tensor(c["demb"], dtype=torch.float64)).sum()
    out.backward()
    assert_close(fw["emb"], emb.detach().numpy(), msg="emb", **TOL)
    assert_close(fw["logits"], logits.detach().numpy(), msg="logits", **TOL)
    assert_close(bw["ds1"], leaves["s1"].grad.numpy(), msg="ds1", **TOL)
    assert_close(bw["ds2"], leaves["s2"].grad.numpy(), msg="ds2", **TOL)
    assert_close(bw["dweight"], leaves["weight"].grad.numpy(), msg="dweight", **TOL)
    assert_close(np.asarray([bw["dbias"]]), leaves["bias"].grad.numpy(), msg="dbias", **TOL)
    # the gradient lands on unmasked positions only, one per (sample, column) at most
    assert not bw["ds1"][~c["mask1"]].any() and not bw["ds2"][~c["mask2"]].any()
    assert ((bw["ds1"] != 0).sum(axis=1) <= 1).all() and ((bw["ds2"] != 0).sum(axis=1) <= 1).all()
    if calib:                                                       # row 0 has bins = -1, every third column scale = -1: untouched
        assert np.array_equal(fw["emb"][0], fw["f"][0]) and np.array_equal(fw["emb"][:, ::3], fw["f"][:, ::3])
        assert not np.array_equal(fw["emb"], fw["f"]) or b == 1


def test_float32_restatement_follows_the_stated_rules():
    """The float32 yardstick on hand-made inputs: ties go to the lowest unmasked t, a NaN wins where it is unmasked and only there, an
    empty mask gives -inf / -1 and no gradient, a dropped maximum carries no gradient."""
    s = np.array([[[1.0, -2.0], [1.0, np.nan], [0.5, 3.0], [1.0, 7.0]]], dtype=np.float32)          # [1, 4, 2]
    m, arg = R.max_over_time(s, np.array([[False, True, True, False]]))
    assert arg.tolist() == [[1, 1]] and m[0, 0] == 1.0 and np.isnan(m[0, 1])
    m, arg = R.max_over_time(s, np.array([[True, False, True, True]]))
    assert arg.tolist() == [[0, 3]] and m.tolist() == [[1.0, 7.0]]
    m, arg = R.max_over_time(s, np.zeros((1, 4), bool))
    assert arg.tolist() == [[-1, -1]] and np.isneginf(m).all()
    s1 = -np.abs(np.random.default_rng(0).normal(1, 1, (2, 3, 4))).astype(np.float32) - 0.1
    keep = np.ones((2, 3, 4), bool)
    keep[:, 1, :2] = False
    mask = np.ones((2, 3), bool)
    w, bias = np.ones(16, np.float32), np.zeros(1, np.float32)
    fw = R.forward(s1, s1, mask, mask, w, bias, keep1=keep, keep2=None, factor=np.float32(2.0))
    assert (fw["u"][:, :2] == 0).all() and (fw["arg1"][:, :2] == 1).all() and (fw["u"][:, 2:] < 0).all()
    bw = R.backward(fw, np.ones(2, np.float32), w, 3, 3, keep1=keep, keep2=None, factor=np.float32(2.0))
    assert not bw["ds1"][:, :, :2].any() and (bw["ds1"][:, :, 2:] != 0).sum() == 4
    assert fw["emb"].dtype == bw["ds1"].dtype == np.float32


def test_header_declares_and_lib_binds_the_new_entry_points():
    from dirhip import _lib
    header = open(os.path.join(ROOT, "include", "dir_hip.h")).read()
    declared = set(re.findall(r"\b(dir_[a-z0-9_]+)\s*\(", header))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(handle, name), name
    assert re.search(r"#define\s+DIR_ABI_VERSION\s+4\b", header)
    assert _lib.lib().dir_abi_version() == _lib.ABI_VERSION == 4
    assert len(_lib.SIGNATURES["dir_pair_tail_fwd"][1]) == 27 and len(_lib.SIGNATURES["dir_pair_tail_bwd"][1]) == 25
    assert _lib.SIGNATURES["dir_pair_tail_workspace"][0] is ctypes.c_size_t


class _Args:
    """Valid argument lists of the two entry points over host memory that is never touched: every call below returns before a launch."""

    def __init__(self, B=2, T1=3, T2=4, D=8):
        self.buf = (ctypes.c_char * 4096)()
        self.P = ctypes.cast(self.buf, ctypes.c_void_p)
        P = self.P
        self.fwd = dict(s1=P, s2=P, mask1=P, mask2=P, B=B, T1=T1, T2=T2, D=D, bins=P, nb=5, m1=P, scale=P, m2=P, weight=P, bias=P,
                        seed=1, offset1=0, offset2=4, p=0.5, emb=P, uv=P, arg1=P, arg2=P, logits=P, workspace=P, workspace_bytes=0,
                        stream=None)
        self.bwd = dict(dlogits=P, demb=P, bins=P, nb=5, scale=P, weight=P, emb=P, uv=P, arg1=P, arg2=P, B=B, T1=T1, T2=T2, D=D,
                        seed=1, offset1=0, offset2=4, p=0.5, ds1=P, ds2=P, dweight=P, dbias=P, workspace=P, workspace_bytes=0,
                        stream=None)


def _call(fn, base, **over):
    a = dict(base)
    a.update(over)
    return fn(*a.values())


def test_argument_errors_are_returned_without_a_gpu():
    from dirhip import _lib
    L = _lib.lib()
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    A = _Args()
    # the base lists are valid up to the workspace size (0 bytes): the last check before the launch
    assert _call(L.dir_pair_tail_fwd, A.fwd) == EWORKSPACE and _call(L.dir_pair_tail_bwd, A.bwd) == EWORKSPACE
    assert _call(L.dir_pair_tail_fwd, A.fwd, workspace=None, workspace_bytes=1 << 20) == EWORKSPACE
    need = L.dir_pair_tail_workspace(2, 8)
    assert need >= max(1 * 2, 1 * 32) * 4 and need % 256 == 0
    assert _call(L.dir_pair_tail_fwd, A.fwd, workspace_bytes=need - 1) == EWORKSPACE
    assert _call(L.dir_pair_tail_bwd, A.bwd, workspace_bytes=need - 1) == EWORKSPACE
    # a NULL required pointer
    for k in ("s1", "s2", "mask1", "mask2", "weight", "bias", "emb", "uv", "arg1", "arg2", "logits"):
        assert _call(L.dir_pair_tail_fwd, A.fwd, **{k: None}) == EINVAL, k
    for k in ("dlogits", "weight", "uv", "arg1", "arg2", "emb"):
        assert _call(L.dir_pair_tail_bwd, A.bwd, **{k: None}) == EINVAL, k
    # sizes
    for k in ("B", "T1", "T2", "D"):
        for bad in (0, -3):
            assert _call(L.dir_pair_tail_fwd, A.fwd, **{k: bad}) == EINVAL, (k, bad)
            assert _call(L.dir_pair_tail_bwd, A.bwd, **{k: bad}) == EINVAL, (k, bad)
    # p outside [0, 1]
    for bad in (-0.1, 1.0000001, float("nan"), float("inf")):
        assert _call(L.dir_pair_tail_fwd, A.fwd, p=bad) == EINVAL and _call(L.dir_pair_tail_bwd, A.bwd, p=bad) == EINVAL, bad
    for ok in (0.0, 1.0):
        assert _call(L.dir_pair_tail_fwd, A.fwd, p=ok) == EWORKSPACE and _call(L.dir_pair_tail_bwd, A.bwd, p=ok) == EWORKSPACE
    # the calibration pointers only partly given
    four = ("bins", "m1", "scale", "m2")
    for mask in range(1, 15):
        over = {k: (A.P if mask >> i & 1 else None) for i, k in enumerate(four)}
        assert _call(L.dir_pair_tail_fwd, A.fwd, **over) == EINVAL, over
    assert _call(L.dir_pair_tail_fwd, A.fwd, nb=0) == EINVAL
    assert _call(L.dir_pair_tail_fwd, A.fwd, bins=None, m1=None, scale=None, m2=None, nb=0) == EWORKSPACE      # none of the four: fine
    assert _call(L.dir_pair_tail_bwd, A.bwd, bins=None) == EINVAL and _call(L.dir_pair_tail_bwd, A.bwd, scale=None) == EINVAL
    assert _call(L.dir_pair_tail_bwd, A.bwd, bins=None, scale=None, nb=0) == EWORKSPACE
    # optional pieces of the backward: demb, either ds, dweight (then no workspace is asked for ... and nothing is left to do but launch,
    # so only the combinations that still end in a check are called here)
    assert _call(L.dir_pair_tail_bwd, A.bwd, demb=None) == EWORKSPACE and _call(L.dir_pair_tail_bwd, A.bwd, ds1=None, ds2=None, uv=None,
                                                                                arg1=None, arg2=None) == EWORKSPACE
    # element counts at or beyond 2^31
    for over in (dict(B=1024, T1=1024, D=2048), dict(B=1024, T2=1024, D=2048), dict(B=32768, D=16384), dict(B=65536, D=4)):
        assert _call(L.dir_pair_tail_fwd, A.fwd, **over) == EUNSUPPORTED and _call(L.dir_pair_tail_bwd, A.bwd, **over) == EUNSUPPORTED, over
    assert L.dir_pair_tail_workspace(0, 8) == L.dir_pair_tail_workspace(8, 0) == L.dir_pair_tail_workspace(32768, 16384) == 0
    assert L.dir_pair_tail_workspace(128, 3000) == 16 * 4 * 3000 * 4           # the product shape: 16 batch slices of [4D] float32 partials


def test_drop_in_module_and_no_cpu_fallback():
    from dirhip import _lib
    from dirhip.pair_tail import PairHead, pair_tail_forward
    spec = importlib.util.spec_from_file_location("stsb_models_dropin", os.path.join(PKG, "sts-b-dir", "models.py"))
    mod = importlib.util.module_from_spec(spec)
    import sys
    sys.path.insert(0, os.path.join(PKG, "sts-b-dir"))
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(PKG, "sts-b-dir"))
    assert mod.PairHead is PairHead and mod.pair_tail_forward is pair_tail_forward
    head = PairHead(6)
    assert head.pred_layer.in_features == 24 and head.pred_layer.out_features == 1
    assert (head.start_smooth, head.loss, head.huber_beta, head.dropout, head.FDS) == (1, "mse", 0.5, 0.2, None)
    with pytest.raises(ValueError):
        PairHead(6, loss="nope")
    s1, s2 = torch.randn(2, 3, 6), torch.randn(2, 4, 6)
    m1, m2 = torch.ones(2, 3, dtype=torch.bool), torch.ones(2, 4, dtype=torch.bool)
    for h in (head, head.eval()):
        with pytest.raises(_lib.DirHipError):
            h(s1, s2, m1, m2, torch.ones(2, 1))
    with pytest.raises(_lib.DirHipError):
        pair_tail_forward(s1, s2, m1, m2, head.pred_layer)
