"""-m gpu: dir_adam_step / dir_sgd_step / dir_conv_prep_weights* (csrc/dir_optim.hip) held PER ELEMENT to the float64 oracle
(oracle/optim_oracle.py), through the C ABI on hand-made tables — no network, no other kernel — and through dirhip.optim on five small tensors.

The table (tests/optim_reference.py: ROWS) interleaves ten plain rows (1 .. 100003 elements: below, at and above a wave, a block, one sweep of
the 128 x 256 grid) with ten convolution rows: one tile, stride-2 classes with Cin != Cout, 144 tiles (more than the 128 workgroups), a null
w16_rot, and four layers on the generic branch (Cin or Cout not a multiple of 64), with rot modes 0, 1 and none. Every step of every run is
teacher-forced: the oracle starts from the kernel's own float32 parameter and state of the step before, so the bound is a one-step bound.

The bound is COUNTED (tests/optim_reference.py, module docstring, with every term): half an ulp of its result for each float32 operation on
the path and one relative 2**-24 for each hyperparameter that arrives as a float32, propagated to the output; a fused multiply-add is
charged as two operations; no array-scale term. csrc/Makefile passes no fast-math flag (tests/test_optim_oracle_host.py checks it), so sqrtf and the division are
correctly rounded. Per element, with u = 2**-24 (Adam: 7 rounded scalars and 13 operations reach the parameter; SGD: 4 and 8):
    exp_avg        (1-b1) (E_G + u |G - m|) + 2 u |(1-b1) (G - m)| + u |M|                  E_G = u (2 |wd p| + |G|), G = g + wd p
    exp_avg_sq     2 u b2 v + (1-b2) (2 |G| E_G + u G^2) + 2 u (1-b2) G^2 + u V
    parameter      ss (E_M / N + |M / N| E_N / N + u |M / N|) + 2 u |ss M / N| + u |P|      N = sqrt(V) / c2 + eps,
                   E_N = (E_V / (2 sqrt V) + u sqrt V) / c2 + 3 u sqrt(V) / c2 + u eps + u N
    momentum_buffer  2 u |mom b| + (1-damp) E_G + 2 u |(1-damp) G| + u |B|                   (first step: E_G)
    parameter (SGD)  lr E_H + 2 u |lr H| + u |P|          E_H = E_G + mom E_B + 2 u |mom B| + u |H| (Nesterov), E_B (momentum), E_G (none)
The bf16 operands are not bounded but compared bit for bit with prep_w16 / prep_w16_rot of the master weight the kernel has just written.

Each test prints the largest error it saw as a fraction of the bound before it asserts (run with -s). The kernels' operation order,
evaluated in numpy float32 on these inputs, reaches 0.9993 (Adam parameter), 0.99 (exp_avg), 0.92 (exp_avg_sq), 0.9996 (SGD parameter) and
0.998 (momentum_buffer) of the bounds: the last rounding alone fills its own term.
"""
import numpy as np
import pytest
import torch

import optim_reference as R
from oracle import optim_oracle as O

pytestmark = pytest.mark.gpu

PAD = 64                                   # sentinel elements behind every buffer
F_SENTINEL = 12345.0
H_SENTINEL = 0x5A5A
EINVAL = -1


def _lib():
    from dirhip import _lib as L
    return L


def _fbuf(values):
    """Device float32 buffer = values followed by PAD sentinels."""
    t = torch.full((len(values) + PAD,), F_SENTINEL, dtype=torch.float32, device="cuda")
    t[:len(values)].copy_(torch.from_numpy(np.array(values, dtype=np.float32)))
    return t


def _hbuf(n):
    return torch.full((n + PAD,), H_SENTINEL, dtype=torch.int16, device="cuda")


def _bits16(t):
    return t.cpu().numpy().view(np.uint16)


def _tail_intact(t, n):
    tail = t[n:].cpu().numpy()
    return (tail.view(np.uint16) == H_SENTINEL).all() if t.dtype == torch.int16 else (tail == F_SENTINEL).all()


class _Table:
    """Device buffers of every row of R.ROWS and the [ntensors][12] int64 table over them. ``state_cols``: how many state tensors a row
    has (Adam 2, SGD 1 or 0: null pointers)."""

    def __init__(self, state_cols, states):
        self.p = [_fbuf(R.make_param(i, r.numel)) for i, r in enumerate(R.ROWS)]
        self.g = [_fbuf(np.zeros(r.numel, np.float32)) for r in R.ROWS]
        self.s = [[_fbuf(states[c][i]) for i in range(len(R.ROWS))] for c in range(state_cols)]
        self.w16 = [_hbuf(r.numel) if r.cout else None for r in R.ROWS]
        self.rot = [_hbuf(r.numel) if r.cout else None for r in R.ROWS]          # allocated for has_rot = no too: must stay untouched
        rows = []
        for i, r in enumerate(R.ROWS):
            st = [self.s[c][i].data_ptr() for c in range(state_cols)] + [0] * (2 - state_cols)
            conv = [self.w16[i].data_ptr(), self.rot[i].data_ptr() if r.has_rot else 0, r.cout, r.r * r.r, r.cin, r.rot_mode, 0] if r.cout else [0] * 7
            rows.append([self.p[i].data_ptr(), self.g[i].data_ptr()] + st + [r.numel] + conv)
        self.table = torch.tensor(rows, dtype=torch.int64).cuda()
        assert self.table.shape == (len(R.ROWS), 12)

    def set_grads(self, k):
        for i, r in enumerate(R.ROWS):
            self.g[i][:r.numel].copy_(torch.from_numpy(R.make_grad(i, r.numel, k).copy()))

    def host(self, bufs):
        return [b[:r.numel].cpu().numpy() for b, r in zip(bufs, R.ROWS)]

    def check_operands_and_tails(self, p_new, what):
        """bf16 operands == oracle of the master weight just written, bit for bit; nothing written behind any buffer or into an unlisted w16_rot."""
        for i, r in enumerate(R.ROWS):
            tag = f"{what} row {i} {tuple(r)}"
            for t in [self.p[i], self.g[i]] + [s[i] for s in self.s]:
                assert _tail_intact(t, r.numel), tag
            if not r.cout:
                continue
            w = p_new[i].reshape(r.cout, r.r, r.r, r.cin)
            assert np.array_equal(_bits16(self.w16[i][:r.numel]), O.prep_w16(w).reshape(-1)), tag + " w16"
            assert _tail_intact(self.w16[i], r.numel), tag
            if r.has_rot:
                assert np.array_equal(_bits16(self.rot[i][:r.numel]), O.prep_w16_rot(w, r.rot_mode)), tag + " w16_rot"
                assert _tail_intact(self.rot[i], r.numel), tag
            else:
                assert _tail_intact(self.rot[i], 0), tag + ": a w16_rot buffer the table does not list was written"


@pytest.mark.parametrize("setting", R.ADAM_SETTINGS, ids=[f"adam{i}" for i in range(len(R.ADAM_SETTINGS))])
def test_adam_step_table_against_float64_oracle_per_element(setting):
    """Three teacher-forced steps with a fresh gradient each over the whole table (OptAdam on the tile and the generic branch, rot modes 0, 1
    and none, plain rows of every size class). Parameter, exp_avg and exp_avg_sq within the counted bound of the oracle for EVERY element
    (module docstring); bf16 operands bit for bit; sentinels behind every buffer intact."""
    L = _lib()
    lr, (b1, b2), eps, wd, step0 = setting
    zero = step0 == 1
    states = list(zip(*[R.make_adam_state(i, r.numel, zero) for i, r in enumerate(R.ROWS)]))
    T = _Table(2, states)
    p, m, v = T.host(T.p), T.host(T.s[0]), T.host(T.s[1])
    worst = [0.0, 0.0, 0.0]
    for k in range(R.NSTEPS):
        k_grad = k if zero else k + 1 if k + 1 < R.NSTEPS else 0              # (a run on non-zero state starts with the gradient that has both zero runs)
        T.set_grads(k_grad)
        L.check(L.lib().dir_adam_step(L.ptr(T.table), len(R.ROWS), lr, b1, b2, eps, wd, step0 + k, L.stream_ptr(T.table.device)), "dir_adam_step")
        torch.cuda.synchronize()
        p1, m1, v1 = T.host(T.p), T.host(T.s[0]), T.host(T.s[1])
        for i, r in enumerate(R.ROWS):
            g = R.make_grad(i, r.numel, k_grad)
            args = (p[i], g, m[i], v[i], lr, b1, b2, eps, wd, step0 + k)
            want, bound = O.adam_step(*args), R.adam_bound(*args)
            for j, (got, name) in enumerate(zip((p1[i], m1[i], v1[i]), ("param", "exp_avg", "exp_avg_sq"))):
                f = R.worst_fraction(got, want[j], bound[j])
                worst[j] = max(worst[j], f)
                assert f <= 1.0, f"step {step0 + k} row {i} {tuple(r)} {name}: {f} of the bound at element {int(np.argmax(np.abs(got - want[j]) / np.maximum(bound[j], 1e-300)))}"
            z = (g == 0) & (m[i] == 0) & (v[i] == 0)                          # zero gradient on zero state (weight decay or not: G = wd p moves it)
            if wd == 0 and z.any():
                assert np.array_equal(p1[i][z], p[i][z]) and not m1[i][z].any() and not v1[i][z].any()
        T.check_operands_and_tails(p1, f"adam step {step0 + k}")
        p, m, v = p1, m1, v1
    print(f"dir_adam_step {setting}: worst error / bound (param, exp_avg, exp_avg_sq) = {worst}")


@pytest.mark.parametrize("setting,first", R.SGD_CASES, ids=[f"sgd{R.SGD_SETTINGS.index(s)}-first{f}" for s, f in R.SGD_CASES])
def test_sgd_step_table_against_float64_oracle_per_element(setting, first):
    """As the Adam test, for OptSgd: each setting from a fresh buffer (first = 1, the kernel fills sentinel-filled buffers) and from a
    non-trivial one; momentum = 0 with NULL buffer pointers in the table."""
    L = _lib()
    mom, wd, nesterov, damp = setting
    ncols = 1 if mom else 0
    if first:
        states = [[np.full(r.numel, F_SENTINEL, np.float32) for r in R.ROWS]]       # never read: the kernel must overwrite all of it
    else:
        states = [[R.make_sgd_buffer(i, r.numel) for i, r in enumerate(R.ROWS)]]
    T = _Table(ncols, states)
    p = T.host(T.p)
    b = T.host(T.s[0]) if (mom and not first) else [None] * len(R.ROWS)
    worst = [0.0, 0.0]
    for k in range(R.NSTEPS):
        k_grad = k if (first or not mom) else k + 1 if k + 1 < R.NSTEPS else 0
        T.set_grads(k_grad)
        L.check(L.lib().dir_sgd_step(L.ptr(T.table), len(R.ROWS), R.SGD_LR, mom, damp, wd, int(nesterov), int(bool(first and k == 0)),
                                     L.stream_ptr(T.table.device)), "dir_sgd_step")
        torch.cuda.synchronize()
        p1 = T.host(T.p)
        b1 = T.host(T.s[0]) if mom else [None] * len(R.ROWS)
        for i, r in enumerate(R.ROWS):
            args = (p[i], R.make_grad(i, r.numel, k_grad), b[i], R.SGD_LR, mom, damp, wd, nesterov)
            (want_p, want_b), (bound_p, bound_b) = O.sgd_step(*args), R.sgd_bound(*args)
            f = R.worst_fraction(p1[i], want_p, bound_p)
            worst[0] = max(worst[0], f)
            assert f <= 1.0, f"step {k} row {i} {tuple(r)} param: {f} of the bound"
            if mom:
                f = R.worst_fraction(b1[i], want_b, bound_b)
                worst[1] = max(worst[1], f)
                assert f <= 1.0, f"step {k} row {i} {tuple(r)} momentum_buffer: {f} of the bound"
        T.check_operands_and_tails(p1, f"sgd step {k}")
        p, b = p1, b1
    print(f"dir_sgd_step {setting} first={first}: worst error / bound (param, momentum_buffer) = {worst}")


def test_unfused_weight_preparation_against_oracle_bit_for_bit():
    """OptNone on every convolution row, through dir_conv_prep_weights_ex (one launch per layer, grid sized by the layer) and through
    dir_conv_prep_weights_batched (one launch, 128 workgroups per layer): weights with exact ties, +-0, +-inf, the largest finite floats and
    NaNs planted all over each tensor. Both operands equal the oracle bit for bit and the master weight is unchanged, bit for bit."""
    L = _lib()
    rows = [(i, r) for i, r in enumerate(R.ROWS) if r.cout]
    w_host = {i: R.make_prep_weight(i, r.numel) for i, r in rows}
    assert all(np.isnan(w).any() and np.isinf(w).any() for w in w_host.values())
    for path in ("ex", "batched"):
        w = {i: _fbuf(w_host[i]) for i, r in rows}
        w16 = {i: _hbuf(r.numel) for i, r in rows}
        rot = {i: _hbuf(r.numel) for i, r in rows}
        if path == "ex":
            for i, r in rows:
                L.check(L.lib().dir_conv_prep_weights_ex(L.ptr(w[i]), r.cout, r.r, r.r, r.cin, L.ptr(w16[i]), L.ptr(rot[i]) if r.has_rot else None,
                                                         r.rot_mode, L.stream_ptr(w[i].device)), "dir_conv_prep_weights_ex")
        else:
            table = torch.tensor([[w[i].data_ptr(), w16[i].data_ptr(), rot[i].data_ptr() if r.has_rot else 0, r.cout, r.r * r.r, r.cin, r.rot_mode]
                                  for i, r in rows], dtype=torch.int64).cuda()
            L.check(L.lib().dir_conv_prep_weights_batched(L.ptr(table), len(rows), L.stream_ptr(table.device)), "dir_conv_prep_weights_batched")
        torch.cuda.synchronize()
        for i, r in rows:
            tag = f"{path} row {i} {tuple(r)}"
            wh = w_host[i].reshape(r.cout, r.r, r.r, r.cin)
            assert np.array_equal(w[i].cpu().numpy().view(np.uint32)[:r.numel], w_host[i].view(np.uint32)), tag + ": master weight changed"
            assert _tail_intact(w[i], r.numel) and _tail_intact(w16[i], r.numel), tag
            assert np.array_equal(_bits16(w16[i][:r.numel]), O.prep_w16(wh).reshape(-1)), tag + " w16"
            if r.has_rot:
                assert np.array_equal(_bits16(rot[i][:r.numel]), O.prep_w16_rot(wh, r.rot_mode)), tag + " w16_rot"
                assert _tail_intact(rot[i], r.numel), tag
            else:
                assert _tail_intact(rot[i], 0), tag + ": w16_rot written though not passed"


def test_refused_arguments_return_einval_and_launch_nothing():
    L = _lib()
    lib = L.lib()
    n = 256
    p0, g0 = np.linspace(1, 2, n, dtype=np.float32), np.full(n, 0.5, np.float32)
    p, g, m, v = _fbuf(p0), _fbuf(g0), _fbuf(np.zeros(n, np.float32)), _fbuf(np.zeros(n, np.float32))
    table = torch.tensor([[p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.int64).cuda()
    s = L.stream_ptr(table.device)
    adam = lambda tb, nt, step: lib.dir_adam_step(tb, nt, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, s)               # noqa: E731
    sgd = lambda tb, nt, mom, damp, nest: lib.dir_sgd_step(tb, nt, 1e-2, mom, damp, 0.0, nest, 0, s)         # noqa: E731
    assert adam(L.ptr(table), 0, 1) == EINVAL
    assert adam(L.ptr(table), 65536, 1) == EINVAL
    assert adam(L.ptr(table), -1, 1) == EINVAL
    assert adam(L.ptr(table), 1, 0) == EINVAL
    assert adam(None, 1, 1) == EINVAL
    assert sgd(L.ptr(table), 0, 0.9, 0.0, 0) == EINVAL
    assert sgd(L.ptr(table), 65536, 0.9, 0.0, 0) == EINVAL
    assert sgd(None, 1, 0.9, 0.0, 0) == EINVAL
    assert sgd(L.ptr(table), 1, 0.9, 0.1, 1) == EINVAL            # Nesterov with dampening
    assert sgd(L.ptr(table), 1, 0.0, 0.0, 1) == EINVAL            # Nesterov without momentum
    assert lib.dir_conv_prep_weights_batched(L.ptr(table), 0, s) == EINVAL
    assert lib.dir_conv_prep_weights_batched(L.ptr(table), 65536, s) == EINVAL
    w, w16, rot = _fbuf(np.ones(64 * 64 * 9, np.float32)), _hbuf(64 * 64 * 9), _hbuf(64 * 64 * 9)
    prep = lambda r, mode: lib.dir_conv_prep_weights_ex(L.ptr(w), 64, r, r, 64, L.ptr(w16), L.ptr(rot), mode, s)   # noqa: E731
    assert prep(3, 2) == EINVAL
    assert prep(3, -1) == EINVAL
    assert prep(1, 1) == EINVAL                                    # the stride-2 classes exist for 3x3 only
    assert lib.dir_conv_prep_weights_ex(None, 64, 3, 3, 64, L.ptr(w16), L.ptr(rot), 0, s) == EINVAL
    assert lib.dir_conv_prep_weights_ex(L.ptr(w), 64, 3, 3, 64, None, L.ptr(rot), 0, s) == EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(p[:n].cpu().numpy(), p0) and not m.cpu().numpy()[:n].any() and not v.cpu().numpy()[:n].any()
    assert _tail_intact(w16, 0) and _tail_intact(rot, 0)
    assert lib.dir_error_string(EINVAL)
    # and the same table is accepted when the arguments are right (the refusals above were about the arguments)
    assert adam(L.ptr(table), 1, 1) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(p[:n].cpu().numpy(), p0)


# ------------------------------------------------------------------------------------------------------------ through dirhip.optim
class _Net:
    """Three registered convolution layers (64 .. 128 channels, an 8 x 8 map: 1x1, 3x3 and a stride-2 3x3, i.e. rot modes 0, 0, 1), a
    bias-like vector and a linear weight; ``dirhip.optim`` on them and ``torch.optim`` (foreach=False, fused=False) on clones. ``step``
    teacher-forces the clones and the oracle from our own values, runs both, and holds ours to the oracle at the counted bound, to torch at
    twice that (each is within one bound of the exact result), and the bf16 operands to the oracle bit for bit."""

    def __init__(self, kind, groups=None, **kw):
        import torch.nn as nn
        from dirhip import conv as C
        from dirhip import optim as DO
        self.C, self.kind = C, kind
        torch.manual_seed(2)
        convs = [nn.Conv2d(64, 128, 1, bias=False), nn.Conv2d(128, 128, 3, padding=1, bias=False), nn.Conv2d(128, 64, 3, stride=2, padding=1, bias=False)]
        self.convs = [c.cuda().to(memory_format=torch.channels_last) for c in convs]
        self.x = torch.randn(2, 64, 8, 8, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        self.forward()                                             # registers the layers: from here on the optimizer owns their bf16 operands
        self.params = [c.weight for c in self.convs] + [nn.Parameter(torch.randn(64, device="cuda")), nn.Parameter(torch.randn(10, 64, device="cuda") * 0.1)]
        self.ref_params = [p.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for p in self.params]
        ours_cls, ref_cls = (DO.Adam, torch.optim.Adam) if kind == "adam" else (DO.SGD, torch.optim.SGD)
        def arg(ps):
            return ps if groups is None else [dict(params=[ps[i] for i in idx], **g) for idx, g in groups]
        self.ours = ours_cls(arg(self.params), **kw)
        self.ref = ref_cls(arg(self.ref_params), foreach=False, fused=False, **kw)
        self.old_grads = []                                        # kept alive: a new gradient tensor is at a NEW address
        self.nstep = 0
        self.worst = 0.0

    def forward(self):
        with torch.no_grad():
            y = self.x
            for c in self.convs:
                y, _ = self.C.conv_bn_input(y, c, False)
        return y

    def make_grads(self, present=None):
        """Fresh gradient tensors (new addresses, the parameter's strides), 1e-12 .. 1e4 with a run of zeros; None where not ``present``."""
        out = []
        for i, p in enumerate(self.params):
            if present is not None and i not in present:
                out.append(None)
                continue
            vals = R.make_grad(100 + i, p.numel(), self.nstep % R.NSTEPS) * np.float32(1 + self.nstep // R.NSTEPS)
            g = torch.empty_like(p, memory_format=torch.preserve_format).copy_(torch.from_numpy(vals.copy()).reshape(p.shape))
            assert g.stride() == p.stride()
            out.append(g)
        return out

    def _hyper(self, p):
        return next(g for g in self.ours.param_groups if any(q is p for q in g["params"]))

    def step(self, present=None, closure=False, expect_kernel=True, refresh=False):
        grads = self.make_grads(present)
        self.old_grads.append([(g, None if g is None else g.cpu().numpy().copy()) for g in grads])
        def assign():
            for p, rp, g in zip(self.params, self.ref_params, grads):
                p.grad = g
                rp.grad = None if g is None else g.clone(memory_format=torch.preserve_format)
        assign()
        state_keys = ("exp_avg", "exp_avg_sq") if self.kind == "adam" else ("momentum_buffer",)
        before = []
        for p, rp in zip(self.params, self.ref_params):                       # teacher forcing: torch and the oracle start from OUR values
            rp.data.copy_(p.data)
            so, sr = self.ours.state.get(p, {}), self.ref.state.get(rp, {})
            for k in state_keys:
                if isinstance(so.get(k), torch.Tensor):
                    sr[k].copy_(so[k])
            before.append((p.detach().cpu().numpy().copy(), {k: so[k].cpu().numpy().copy() for k in state_keys if isinstance(so.get(k), torch.Tensor)}))
        keys_before = {gi: t[0] for gi, t in self.ours._tables.items()}
        if closure:
            for p, rp in zip(self.params, self.ref_params):
                p.grad = rp.grad = None
            def cl():
                assert torch.is_grad_enabled()
                assign()
                return torch.tensor(3.5)
            assert float(self.ref.step(cl)) == 3.5
            assert float(self.ours.step(cl)) == 3.5
        else:
            self.ref.step()                                        # (every optimizer.step() opens a new weight-cache generation: ours last)
            assert self.ours.step() is None
        torch.cuda.synchronize()
        self.nstep += 1
        if expect_kernel:                                          # our launch, not torch's step: a table for THIS step's gradient addresses
            assert all(self.ours._tables[gi][0] != k for gi, k in keys_before.items())
            assert len(self.ours._tables) == len([g for g in self.ours.param_groups if any(p.grad is not None for p in g["params"])])
        for i, (p, rp, g, (p0, s0)) in enumerate(zip(self.params, self.ref_params, grads, before)):
            so, sr = self.ours.state.get(p, {}), self.ref.state.get(rp, {})
            assert set(so.keys()) == set(sr.keys()), (i, so.keys(), sr.keys())
            if "step" in sr:
                assert float(so["step"]) == float(sr["step"]), (i, so["step"], sr["step"])
            got_p = p.detach().cpu().numpy()
            if g is None:
                assert np.array_equal(got_p, p0)
                for k, a in s0.items():
                    assert np.array_equal(so[k].cpu().numpy(), a)
                continue
            h = self._hyper(p)
            g_host = self.old_grads[-1][i][1]
            if self.kind == "adam":
                args = (p0, g_host, s0.get("exp_avg", np.zeros_like(p0)), s0.get("exp_avg_sq", np.zeros_like(p0)), h["lr"], h["betas"][0], h["betas"][1],
                        h["eps"], h["weight_decay"], int(sr["step"]))
                want, bound = O.adam_step(*args), R.adam_bound(*args)
                got = (got_p, so["exp_avg"].cpu().numpy(), so["exp_avg_sq"].cpu().numpy())
                theirs = (rp.detach().cpu().numpy(), sr["exp_avg"].cpu().numpy(), sr["exp_avg_sq"].cpu().numpy())
                assert so["exp_avg"].stride() == p.stride() and so["exp_avg_sq"].stride() == p.stride()
            else:
                args = (p0, g_host, s0.get("momentum_buffer"), h["lr"], h["momentum"], h["dampening"], h["weight_decay"], h["nesterov"])
                want, bound = O.sgd_step(*args), R.sgd_bound(*args)
                got, theirs = (got_p,), (rp.detach().cpu().numpy(),)
                if h["momentum"]:
                    got += (so["momentum_buffer"].cpu().numpy(),)
                    theirs += (sr["momentum_buffer"].cpu().numpy(),)
            for a, t, w, b in zip(got, theirs, want, bound):
                f = R.worst_fraction(a, w, b)
                self.worst = max(self.worst, f)
                assert f <= 1.0, f"step {self.nstep} tensor {i}: {f} of the bound against the oracle"
                assert R.worst_fraction(a, t.astype(np.float64), 2 * b) <= 1.0, f"step {self.nstep} tensor {i}: against torch.optim"
        if refresh:
            self.forward()                                         # torch's own step rewrote the weights: the next forward re-prepares
        for c in self.convs:
            st = c._dir_w16
            assert st.key == self.C._weight_key(c.weight)          # what the step wrote is what the next forward uses
            w = c.weight.detach().permute(0, 2, 3, 1).contiguous().cpu().numpy()          # [Cout][R][S][Cin]
            assert np.array_equal(_bits16(st.w16.permute(0, 2, 3, 1).contiguous().view(torch.int16)).reshape(-1), O.prep_w16(w).reshape(-1))
            rot = st.w16_rot if st.w16_rot.dim() == 1 else st.w16_rot.permute(0, 2, 3, 1).contiguous()
            assert np.array_equal(_bits16(rot.view(torch.int16)).reshape(-1), O.prep_w16_rot(w, st.rot_mode))
        return keys_before

    def old_grads_intact(self):
        for grads in self.old_grads:
            for g, saved in grads:
                if g is not None:
                    assert np.array_equal(g.cpu().numpy().view(np.uint32), saved.view(np.uint32))


ADAM_KW = dict(lr=1e-3, weight_decay=1e-4)
SGD_KW = dict(lr=1e-2, momentum=0.9, weight_decay=1e-4)
KINDS = [("adam", ADAM_KW), ("sgd", SGD_KW)]


@pytest.mark.parametrize("kind,kw", KINDS, ids=["adam", "sgd"])
def test_optimizer_follows_gradients_to_new_addresses(kind, kw):
    """zero_grad(set_to_none=True): every step's gradients are new tensors at new addresses. The cached table's key changes with them and no
    stale address is read as a gradient or written: results match the oracle for THIS step's gradients, earlier gradient tensors are intact."""
    net = _Net(kind, **kw)
    assert [c._dir_w16.rot_mode for c in net.convs] == [0, 0, 1]
    keys = []
    for _ in range(3):
        net.step()
        keys.append(net.ours._tables[0][0])
        net.ours.zero_grad(set_to_none=True)
        assert all(p.grad is None for p in net.params)
    assert len(set(keys)) == 3
    ptrs = [g.data_ptr() for grads in net.old_grads for g, _ in grads]
    assert len(set(ptrs)) == len(ptrs)
    net.old_grads_intact()
    print(f"dirhip.optim {kind}: worst error / bound = {net.worst}")


@pytest.mark.parametrize("kind,kw", [("adam", dict(lr=1e-3)), ("sgd", dict(lr=1e-2, momentum=0.8, dampening=0.1))], ids=["adam", "sgd"])
def test_two_parameter_groups_with_their_own_lr_and_weight_decay(kind, kw):
    groups = [([0, 1, 4], dict(lr=5e-2, weight_decay=1e-2)), ([2, 3], dict(weight_decay=0.0))]
    net = _Net(kind, groups=groups, **kw)
    for _ in range(3):
        net.step()
    assert len(net.ours._tables) == 2 and net.ours._tables[0][1].shape == (3, 12) and net.ours._tables[1][1].shape == (2, 12)
    assert net.ours.param_groups[0]["lr"] == 5e-2 and net.ours.param_groups[1]["lr"] == kw["lr"]
    print(f"dirhip.optim {kind}, two groups: worst error / bound = {net.worst}")


def test_adam_restored_step_count_and_reference_layout_moments():
    """load_state_dict with step = 1000 and NCHW-contiguous moments, then two steps: the bias corrections are those of steps 1001 and 1002
    (the oracle is given torch's own step count), the moments are re-laid out to the parameters' strides with the same values."""
    import copy
    net = _Net("adam", **ADAM_KW)
    net.step()
    sd = net.ref.state_dict()
    for st in sd["state"].values():
        st["step"] = torch.tensor(1000.0)
        for k in ("exp_avg", "exp_avg_sq"):
            st[k] = st[k].contiguous().clone()
    net.ours.load_state_dict(copy.deepcopy(sd))
    net.ref.load_state_dict(copy.deepcopy(sd))
    assert net.ours._tables == {}
    assert net.ours.state[net.params[1]]["exp_avg"].stride() != net.params[1].stride()
    for want in (1001.0, 1002.0):
        net.step()
        assert all(float(net.ours.state[p]["step"]) == want for p in net.params)
    print(f"dirhip.optim adam, restored step count: worst error / bound = {net.worst}")


@pytest.mark.parametrize("kind,kw", KINDS, ids=["adam", "sgd"])
def test_step_with_a_closure(kind, kw):
    net = _Net(kind, **kw)
    for _ in range(2):
        net.step(closure=True)
    print(f"dirhip.optim {kind}, closure: worst error / bound = {net.worst}")


def test_adam_parameter_that_gets_its_first_gradient_late():
    """A parameter without a gradient for two steps, then with one: its step count (1) differs from the others' (3). torch.optim.Adam takes
    that without complaint, and so must the drop-in: no exception, no half-advanced state, torch's result and torch's step counts —
    through torch's own step, since one launch has one step count."""
    net = _Net("adam", **ADAM_KW)
    for _ in range(2):
        net.step(present=[0, 1, 2, 4])
    assert len(net.ours.state.get(net.params[3], {})) == 0
    steps_before = [float(net.ours.state[p]["step"]) for i, p in enumerate(net.params) if i != 3]
    assert steps_before == [2.0] * 4
    for n in (3, 4):
        net.step(expect_kernel=False, refresh=True)
        assert [float(net.ours.state[p]["step"]) for p in net.params] == [n, n, n, n - 2.0, n]
        assert [float(net.ref.state[p]["step"]) for p in net.ref_params] == [n, n, n, n - 2.0, n]
    print(f"dirhip.optim adam, late first gradient: worst error / bound = {net.worst}")


def test_sgd_momentum_parameter_that_gets_its_first_gradient_late():
    """The same for SGD with momentum: one parameter's buffer starts two steps after the others'."""
    net = _Net("sgd", **SGD_KW)
    for _ in range(2):
        net.step(present=[0, 1, 2, 4])
    assert "momentum_buffer" not in net.ours.state.get(net.params[3], {})
    for _ in range(2):
        net.step(expect_kernel=False, refresh=True)
    assert all(isinstance(net.ours.state[p]["momentum_buffer"], torch.Tensor) for p in net.params)
    print(f"dirhip.optim sgd, late first gradient: worst error / bound = {net.worst}")

