"""CPU checks of oracle/optim_oracle.py and of the counted bounds in tests/optim_reference.py, on the very inputs that
tests/test_hip_optim_exact.py gives the kernels:

  * tolerance: torch.optim.Adam / SGD (foreach=False, fused=False) on CPU float32 tensors meet the per-element bound against the oracle.
    If torch's own float32 arithmetic broke a bound, the bound would be wrong, not the kernel;
  * sharpness: eight plausible wrong formulas each break the bound on >= 1 % of the elements of at least one case, i.e. the inputs can tell
    the formulas apart at this bound;
  * layouts: prep_w16 against torch's bfloat16 conversion bit for bit, prep_w16_rot against the torch flip / permute and parity-class
    formulations of tests/test_hip_conv.py, on values that encode their own (co, r, s, ci).

Largest observed error of torch on the CPU as a fraction of its bound (this file, all rows and settings): Adam 0.9993 (parameter), 0.93
(exp_avg), 0.80 (exp_avg_sq); SGD 0.9996 (parameter), 0.998 (momentum_buffer). The parameter's last rounding alone reaches u |P|, its own term.
"""
import os
import re

import numpy as np
import pytest
import torch

import optim_reference as R
from oracle import optim_oracle as O

def _adam_inputs(setting):
    """Concatenated (p, g, m, v) of all rows for the FIRST step of a setting (one step is what the host checks run)."""
    zero = setting[4] == 1
    cols = [[], [], [], []]
    for i, r in enumerate(R.ROWS):
        m, v = R.make_adam_state(i, r.numel, zero)
        for c, a in zip(cols, (R.make_param(i, r.numel), R.make_grad(i, r.numel, 0 if zero else 1), m, v)):
            c.append(a)
    return [np.concatenate(c) for c in cols]


def _sgd_inputs(first, momentum):
    cols = [[], [], []]
    for i, r in enumerate(R.ROWS):
        for c, a in zip(cols, (R.make_param(i, r.numel), R.make_grad(i, r.numel, 0 if first else 1), R.make_sgd_buffer(i, r.numel))):
            c.append(a)
    p, g, b = [np.concatenate(c) for c in cols]
    return p, g, (None if first or momentum == 0 else b)


def _adam_args(setting):
    lr, (b1, b2), eps, wd, step = setting
    return lr, b1, b2, eps, wd, step


def _sgd_args(setting):
    mom, wd, nesterov, damp = setting
    return R.SGD_LR, mom, damp, wd, nesterov


def test_build_has_no_fast_math_flag():
    """The counted bound takes sqrtf and the division as correctly rounded and every operation as rounded once: no fast-math, no contraction."""
    mk = open(os.path.join(os.path.dirname(__file__), "..", "imbalanced-regression_amd", "csrc", "Makefile")).read()
    flags = " ".join(line for line in mk.splitlines() if re.match(r"\s*(HIPFLAGS|CXXFLAGS)\s*[:+]?=", line))
    assert "-ffp-contract=off" in flags
    for bad in ("-ffast-math", "-Ofast", "-funsafe-math-optimizations", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-freciprocal-math",
                "-fapprox-func", "-fgpu-flush-denormals-to-zero", "-ffp-contract=fast"):
        assert bad not in mk, bad


def test_inputs_are_what_the_bounds_assume():
    """Fixed seeds, gradients over 1e-12 .. 1e4, zeros of both signs, second moments >= 0, and every product of one step normal in float32."""
    tiny = float(np.finfo(np.float32).tiny)
    for i, r in enumerate(R.ROWS):
        p = R.make_param(i, r.numel)
        assert np.array_equal(p, R.make_param(i, r.numel)) and p.dtype == np.float32
        m, v = R.make_adam_state(i, r.numel, False)
        assert (v >= 0).all()
        for k in range(R.NSTEPS):
            g = R.make_grad(i, r.numel, k)
            nz = np.abs(g[g != 0]).astype(np.float64)
            assert nz.min() >= 0.99e-12 and nz.max() <= 1.01e4
            if r.numel >= 16:
                assert (g == 0).any() and np.signbit(g[g == 0]).any() and not np.signbit(g[g == 0]).all()
            # the smallest non-zero factors that meet: (1 - beta2) g^2, lr g, weight_decay p, (1 - beta1) g
            assert 1e-3 * nz.min() ** 2 > tiny and 1e-3 * nz.min() > tiny and 1e-4 * np.abs(p).min() > tiny
    allg = np.concatenate([R.make_grad(i, r.numel, 0) for i, r in enumerate(R.ROWS)])
    mags = np.log10(np.abs(allg[allg != 0]))
    assert mags.min() < -11.9 and mags.max() > 3.9


@pytest.mark.parametrize("setting", R.ADAM_SETTINGS, ids=[f"adam{i}" for i in range(len(R.ADAM_SETTINGS))])
def test_torch_cpu_adam_meets_the_counted_bound(setting):
    p, g, m, v = _adam_inputs(setting)
    lr, b1, b2, eps, wd, step = _adam_args(setting)
    want = O.adam_step(p, g, m, v, lr, b1, b2, eps, wd, step)
    bound = R.adam_bound(p, g, m, v, lr, b1, b2, eps, wd, step)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    tp.grad = torch.from_numpy(g.copy())
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False, fused=False)
    opt.state[tp] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
    opt.step()
    st = opt.state[tp]
    assert float(st["step"]) == step
    got = (tp.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy())
    fracs = [R.worst_fraction(a, w, b) for a, w, b in zip(got, want, bound)]
    print("torch CPU Adam, worst error / bound (p, exp_avg, exp_avg_sq):", fracs)
    assert max(fracs) <= 1.0, fracs
    if setting[4] == 1:                                            # zero gradient on zero state: nothing moves
        z = (g == 0)
        assert z.any() and np.array_equal(got[0][z], p[z]) and not got[1][z].any() and not got[2][z].any()


@pytest.mark.parametrize("setting,first", R.SGD_CASES, ids=[f"sgd{R.SGD_SETTINGS.index(s)}-first{f}" for s, f in R.SGD_CASES])
def test_torch_cpu_sgd_meets_the_counted_bound(setting, first):
    p, g, buf = _sgd_inputs(first, setting[0])
    args = _sgd_args(setting)
    want_p, want_b = O.sgd_step(p, g, buf, *args)
    bound_p, bound_b = R.sgd_bound(p, g, buf, *args)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    tp.grad = torch.from_numpy(g.copy())
    lr, mom, damp, wd, nesterov = args
    opt = torch.optim.SGD([tp], lr=lr, momentum=mom, dampening=damp, weight_decay=wd, nesterov=nesterov, foreach=False, fused=False)
    if buf is not None:
        opt.state[tp] = {"momentum_buffer": torch.from_numpy(buf.copy())}
    opt.step()
    fracs = [R.worst_fraction(tp.detach().numpy(), want_p, bound_p)]
    if mom != 0:
        fracs.append(R.worst_fraction(opt.state[tp]["momentum_buffer"].numpy(), want_b, bound_b))
    else:
        assert want_b is None and bound_b is None
    print("torch CPU SGD, worst error / bound (p, momentum_buffer):", fracs)
    assert max(fracs) <= 1.0, fracs


def test_variant_scaffold_without_a_mutation_is_the_oracle():
    p, g, m, v = _adam_inputs(R.ADAM_SETTINGS[2])
    a = _adam_args(R.ADAM_SETTINGS[2])
    for x, y in zip(R._adam_variant(p, g, m, v, *a, wrong=None), O.adam_step(p, g, m, v, *a)):
        assert np.array_equal(x, y)
    for setting, first in R.SGD_CASES:
        p, g, buf = _sgd_inputs(first, setting[0])
        for x, y in zip(R._sgd_variant(p, g, buf, *_sgd_args(setting), wrong=None), O.sgd_step(p, g, buf, *_sgd_args(setting))):
            assert (x is None and y is None) or np.array_equal(x, y)


def _broken_share(got, want, bound):
    """Largest share of elements outside the bound among the outputs (parameter and state)."""
    return max(float((np.abs(a - w) > b).mean()) for a, w, b in zip(got, want, bound) if w is not None)


@pytest.mark.parametrize("wrong", R.ADAM_WRONG)
def test_wrong_adam_formula_breaks_the_bound(wrong):
    shares = []
    for setting in R.ADAM_SETTINGS:
        p, g, m, v = _adam_inputs(setting)
        a = _adam_args(setting)
        shares.append(_broken_share(R.adam_wrong(wrong, p, g, m, v, *a), O.adam_step(p, g, m, v, *a), R.adam_bound(p, g, m, v, *a)))
    print(wrong, "share of elements outside the bound, per setting:", shares)
    assert max(shares) >= 0.01, shares


@pytest.mark.parametrize("wrong", R.SGD_WRONG)
def test_wrong_sgd_formula_breaks_the_bound(wrong):
    shares = []
    for setting, first in R.SGD_CASES:
        p, g, buf = _sgd_inputs(first, setting[0])
        a = _sgd_args(setting)
        shares.append(_broken_share(R.sgd_wrong(wrong, p, g, buf, *a), O.sgd_step(p, g, buf, *a), R.sgd_bound(p, g, buf, *a)))
    print(wrong, "share of elements outside the bound, per case:", shares)
    assert max(shares) >= 0.01, shares


# ----------------------------------------------------------------------------------------------------------------- layouts
def test_prep_w16_is_torch_bfloat16_bit_for_bit():
    rng = np.random.default_rng(21)
    bits = np.concatenate([rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32),       # every exponent, both signs
                           (rng.integers(0, 2 ** 16, 50000, dtype=np.uint64).astype(np.uint32) << 16) | 0x8000,   # exact ties
                           R.SPECIAL_BITS])
    w = bits.view(np.float32)
    got = O.prep_w16(w)
    ref = torch.from_numpy(w.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(w)
    assert nan.sum() > 100 and (~nan).sum() > 200000
    assert np.array_equal(got[~nan], ref[~nan])
    # torch turns every NaN into ONE pattern of its choice (and not the same one on every code path); the kernels keep sign and payload.
    # Against torch a NaN must stay a NaN; the pattern itself is checked against the rule, written out for a few by hand.
    assert (((ref[nan] & 0x7F80) == 0x7F80) & ((ref[nan] & 0x7F) != 0)).all()
    assert (((got[nan] & 0x7F80) == 0x7F80) & ((got[nan] & 0x40) != 0)).all()
    assert np.array_equal(got[nan], ((bits[nan] >> 16) | 0x40).astype(np.uint16))
    by_hand = {0x7FC00000: 0x7FC0, 0xFFC00000: 0xFFC0, 0x7F800001: 0x7FC0, 0xFF80FFFF: 0xFFC0, 0x7FFFFFFF: 0x7FFF, 0x7FA55555: 0x7FE5,
               0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0xBF808000: 0xBF80, 0xBF818000: 0xBF82, 0x3F807FFF: 0x3F80, 0x3F808001: 0x3F81,
               0x00000000: 0x0000, 0x80000000: 0x8000, 0x7F800000: 0x7F80, 0xFF800000: 0xFF80, 0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80,
               0x7F7F7FFF: 0x7F7F, 0x7F7F8000: 0x7F80}
    assert set(by_hand) == set(R.SPECIAL_BITS.tolist())
    for b, h in by_hand.items():
        assert int(O.prep_w16(np.array([b], np.uint32).view(np.float32))[0]) == h, hex(b)
    assert np.array_equal(O.prep_w16(w[:250000].reshape(50, 100, 50)), got[:250000].reshape(50, 100, 50))      # shape kept


def _coded_weight(cout, r, s, cin):
    """Three [Cout][R][S][Cin] float32 arrays whose bf16 rounding is exact and which together name their own (co, r, s, ci): sign and
    exponent carry (r, s) in each; the 7 fraction bits carry co % 128 in the first, ci % 128 in the second and the high parts of both in the
    third. A layout that is right for all three maps every (co, r, s, ci) to its own place."""
    co, rr, ss, ci = np.meshgrid(np.arange(cout), np.arange(r), np.arange(s), np.arange(cin), indexing="ij")
    scale = np.where((rr + ss) % 2 == 0, 1.0, -1.0) * 2.0 ** (rr * s + ss - 20)
    out = [(scale * (128 + f)).astype(np.float32) for f in (co % 128, ci % 128, (co // 128) * 2 + ci // 128)]
    assert cout <= 256 and cin <= 256 and len(np.unique(np.stack(out).reshape(3, -1), axis=1)[0]) == co.size      # all codes distinct
    return out


@pytest.mark.parametrize("cout,cin,r", [(6, 10, 3), (80, 48, 3), (64, 128, 1), (24, 40, 7)])
def test_prep_w16_rot_mode0_is_the_flipped_transposed_weight(cout, cin, r):
    for w in _coded_weight(cout, r, r, cin):
        assert np.array_equal(O.prep_w16(w).astype(np.uint32) << 16, w.view(np.uint32))          # exact in bf16: nothing hidden by rounding
        t = torch.from_numpy(w).permute(0, 3, 1, 2)                                               # the nn.Conv2d weight [Cout, Cin, R, S]
        ref = t.to(torch.bfloat16).flip(2, 3).permute(1, 0, 2, 3).contiguous(memory_format=torch.channels_last)
        ref = ref.permute(0, 2, 3, 1).contiguous().view(torch.int16).numpy().view(np.uint16).reshape(-1)     # memory order [Cin][R][S][Cout]
        got = O.prep_w16_rot(w, 0)
        assert got.dtype == np.uint16 and got.shape == (w.size,)
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("cout,cin", [(6, 10), (80, 48), (128, 64)])
def test_prep_w16_rot_mode1_is_the_four_parity_classes(cout, cin):
    for w in _coded_weight(cout, 3, 3, cin):
        w16 = torch.from_numpy(w).permute(0, 3, 1, 2).to(torch.bfloat16)                          # [Cout, Cin, 3, 3]
        pieces = []
        for a in (0, 1):
            for b in (0, 1):
                rs = [1] if a == 0 else [2, 0]
                ss = [1] if b == 0 else [2, 0]
                sub = w16[:, :, rs][:, :, :, ss]                                                    # [Cout, Cin, R', S']
                pieces.append(sub.permute(1, 2, 3, 0).contiguous().reshape(-1))                     # [Cin][R'][S'][Cout]
        ref = torch.cat(pieces).view(torch.int16).numpy().view(np.uint16)
        got = O.prep_w16_rot(w, 1)
        assert got.shape == (9 * cout * cin,)
        assert np.array_equal(got, ref)
        assert sorted(got.tolist()) == sorted(O.prep_w16(w).reshape(-1).tolist())                   # a permutation: every tap exactly once
