"""CPU: the float64 references of tests/bf16_reference.py against torch float64 autograd on inputs where no decision is ambiguous
(continuous random values: no ties, no pre-activation at 0), and each bar against the defect it is meant to catch."""
import pytest
import torch
import torch.nn.functional as F

import bf16_reference as R


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bn_case(shape, seed, relu, has_res):
    g = _gen(seed)
    n, c, h, w = shape
    x = torch.randn(shape, generator=g, dtype=torch.float64) * 1.7 + 0.3
    res = torch.randn(shape, generator=g, dtype=torch.float64) if has_res else None
    gamma = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(c, generator=g, dtype=torch.float64) * 0.2
    dy = torch.randn(shape, generator=g, dtype=torch.float64) + (torch.randn(c, generator=g, dtype=torch.float64) * 0.7).view(1, -1, 1, 1)
    return x, res, gamma, beta, dy


@pytest.mark.parametrize("relu,has_res", [(False, False), (True, False), (True, True)])
def test_bn_reference_matches_autograd(relu, has_res):
    shape = (3, 16, 5, 7)
    x, res, gamma, beta, dy = _bn_case(shape, 1, relu, has_res)
    eps, mom = 1e-5, 0.1
    rm0, rv0 = torch.randn(16, generator=_gen(2), dtype=torch.float64) * 0.1, torch.rand(16, generator=_gen(3), dtype=torch.float64) + 0.5
    xa, ga, ba = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ra = res.clone().requires_grad_(True) if has_res else None
    rm, rv = rm0.clone(), rv0.clone()
    ya = F.batch_norm(xa, rm, rv, ga, ba, True, mom, eps)
    if has_res:
        ya = ya + ra
    if relu:
        ya = torch.relu(ya)
    ya.backward(dy)

    mean, var = R.bn_stats(x)
    pre = R.bn_fwd(x, gamma, beta, eps, mean, var, res)
    y = torch.relu(pre) if relu else pre
    torch.testing.assert_close(y, ya.detach(), rtol=1e-12, atol=1e-12)
    mask = pre > 0
    frac, ok = R.relu_ambiguous(pre, mask)
    assert frac == 0.0 and ok
    gm = torch.where(mask, dy, torch.zeros_like(dy)) if relu else dy
    b = R.bn_bwd(gm, x, gamma, eps, mean, var)
    torch.testing.assert_close(b["dx"], xa.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(b["dgamma"], ga.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(b["dbeta"], ba.grad, rtol=1e-10, atol=1e-12)
    if has_res:
        torch.testing.assert_close(gm, ra.grad, rtol=0, atol=0)
    m = shape[0] * shape[2] * shape[3]
    erm, erv = R.running_stats(rm0, rv0, mean, var, m, mom)
    torch.testing.assert_close(erm, rm, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(erv, rv, rtol=1e-12, atol=1e-14)


def test_bn_bars_have_teeth():
    """dx without its -a sum(g)/M term, dgamma / dbeta with one kernel row block dropped, y rounded toward zero: each is rejected."""
    shape = (8, 64, 56, 56)                                   # the issue's example: the term is < 0.2 % of max|dx| there
    x, _, gamma, beta, dy = _bn_case(shape, 4, False, False)
    x = x.to(torch.bfloat16).double()
    dy = dy.to(torch.bfloat16).double()
    mean, var = R.bn_stats(x)
    b = R.bn_bwd(dy, x, gamma, 1e-5, mean, var)
    m = shape[0] * shape[2] * shape[3]
    no_term = b["dx"] + R._c(b["a"] * b["dbeta"] / m)
    R.has_teeth(no_term, b["dx"], R.bf16_bar(b["dx"], b["dx_extra"]), "dx without -a sum(g)/M")
    rows = R.bn_block_rows(m, 64, 8, block=0)
    g2 = dy.permute(0, 2, 3, 1).reshape(m, 64).clone()
    g2[rows] = 0
    g2 = g2.view(shape[0], shape[2], shape[3], 64).permute(0, 3, 1, 2)
    bd = R.bn_bwd(g2, x, gamma, 1e-5, mean, var)
    R.has_teeth(bd["dgamma"], b["dgamma"], R.sum_bar(b["S_dgamma"]), "dgamma without row block 0")
    R.has_teeth(bd["dbeta"], b["dbeta"], R.sum_bar(b["S_dbeta"]), "dbeta without row block 0")
    y = R.bn_fwd(x, gamma, beta, 1e-5, mean, var)
    R.has_teeth(R.bf16_round_toward_zero(y), y, R.bf16_bar(y), "y rounded toward zero")
    # and the bar accepts what it is meant to accept: y rounded to nearest bf16
    assert R.ratio(y.to(torch.bfloat16).double(), y, R.bf16_bar(y)) <= 1.0


def test_bn_block_rows_partition_the_rows():
    """The row blocks of bn_block_rows partition the rows (whatever geometry it restates, every row lies in exactly one block)."""
    for m, c, vec in ((25088, 64, 8), (25088, 256, 8), (90, 128, 8), (12, 8, 8), (6272, 2048, 8), (1000, 64, 4)):
        ct = min(c, 32 * vec)
        rpi = 256 // (ct // vec)
        want = max(1, -(-m // (rpi * 4)))
        rblocks = min(want, max(1, 768 // (c // ct)))
        seen = torch.cat([R.bn_block_rows(m, c, vec, b) for b in range(rblocks)])
        assert torch.equal(seen.sort().values, torch.arange(m))


@pytest.mark.parametrize("shape", [(2, 8, 9, 7), (2, 8, 10, 12), (1, 8, 1, 1)])
def test_maxpool_reference_matches_autograd(shape):
    x = torch.randn(shape, generator=_gen(5), dtype=torch.float64)
    dy = torch.randn((shape[0], shape[1], (shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1), generator=_gen(6), dtype=torch.float64)
    xa = x.clone().requires_grad_(True)
    ya = F.max_pool2d(xa, 3, 2, 1)
    ya.backward(dy)
    best, route, second = R.maxpool_ref(x)
    assert torch.equal(best, ya.detach())
    dx = R.pool_scatter(dy, route, torch.ones_like(route, dtype=torch.bool), shape[2], shape[3])
    torch.testing.assert_close(dx, xa.grad, rtol=0, atol=0)


def test_maxpool_reference_tie_rule_is_first_maximum():
    """Plateaus (ReLU zeros): torch routes to the first maximum in scan order, and so does the reference."""
    x = torch.relu(torch.randn((2, 8, 9, 8), generator=_gen(7))).to(torch.bfloat16).double()
    x[:, :, :4] = 0.0
    dy = torch.randn((2, 8, 5, 4), generator=_gen(8), dtype=torch.float64)
    xa = x.clone().requires_grad_(True)
    F.max_pool2d(xa, 3, 2, 1).backward(dy)
    best, route, second = R.maxpool_ref(x)
    dx = R.pool_scatter(dy, route, torch.ones_like(route, dtype=torch.bool), 9, 8)
    assert torch.equal(dx, xa.grad)
    # the defect 'one window routed to its second-best position' is rejected
    route2 = route.clone()
    route2[0, 0, 2, 1] = second[0, 0, 2, 1]
    dy2 = dy.clone()
    dy2[0, 0, 2, 1] = 1.0                                     # a gradient that is not ~0 on that window
    ref = R.pool_scatter(dy2, route, torch.ones_like(route, dtype=torch.bool), 9, 8)
    bad = R.pool_scatter(dy2, route2, torch.ones_like(route, dtype=torch.bool), 9, 8)
    R.has_teeth(bad, ref, R.bf16_bar(ref), "pool dx routed to the second-best position")


def test_stem_tail_reference_matches_autograd():
    shape = (2, 16, 9, 10)
    g = _gen(9)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    gamma = torch.rand(16, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(16, generator=g, dtype=torch.float64) * 0.3
    dy = torch.randn((2, 16, 5, 5), generator=g, dtype=torch.float64) + 0.5
    xa, ga, ba = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ya = F.max_pool2d(torch.relu(F.batch_norm(xa, None, None, ga, ba, True, 0.1, 1e-5)), 3, 2, 1)
    ya.backward(dy)
    mean, var = R.bn_stats(x)
    t = R.stem_tail_ref(x, gamma, beta, 1e-5, mean, var)
    assert not t["ambiguous"].any()
    torch.testing.assert_close(t["y"], ya.detach(), rtol=1e-12, atol=1e-12)
    gs = R.pool_scatter(dy, t["route"], t["valid"], 9, 10)
    b = R.bn_bwd(gs, x, gamma, 1e-5, mean, var)
    torch.testing.assert_close(b["dx"], xa.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(b["dgamma"], ga.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(b["dbeta"], ba.grad, rtol=1e-10, atol=1e-12)


def test_stem_tail_reference_takes_the_kernel_route_only_on_near_ties():
    x = torch.zeros((1, 8, 3, 3), dtype=torch.float64)
    x[0, :, 1, 1] = 1.0
    x[0, :, 1, 2] = 1.0 + 2.0 ** -30                         # within float32 rounding of the maximum: ambiguous
    x[0, 1, 1, 2] = 1.5                                       # clearly the maximum in channel 1
    gamma, beta = torch.ones(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)
    mean, var = torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64) - 1e-5
    kidx = torch.full((1, 8, 2, 2), 6, dtype=torch.uint8)   # window (0, 1) holds (1, 1) at k = 6 and (1, 2) at k = 7
    t = R.stem_tail_ref(x, gamma, beta, 1e-5, mean, var, kernel_idx=kidx)
    assert bool(t["ambiguous"][0, 0, 0, 1]) and int(t["route"][0, 0, 0, 1]) == 6
    assert not bool(t["ambiguous"][0, 1, 0, 1]) and int(t["route"][0, 1, 0, 1]) == 7


@pytest.mark.parametrize("shape", [(2, 3, 13, 16), (1, 3, 5, 8)])
def test_stem_wgrad_reference_matches_autograd(shape):
    g = _gen(10)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    w = torch.randn((64, 3, 7, 7), generator=g, dtype=torch.float64).requires_grad_(True)
    y = F.conv2d(x, w, None, 2, 3)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64) + 0.3
    y.backward(dy)
    dw, S = R.stem_wgrad_ref(dy, x)
    torch.testing.assert_close(dw, w.grad, rtol=1e-12, atol=1e-12)
    assert (S >= dw.abs() - 1e-12).all()


def test_stem_wgrad_bar_has_teeth():
    """dW with one output row of one image missing, or with the rows of the reduce's last workgroup partial missing, is rejected."""
    g = _gen(11)
    n, h, w = 3, 13, 224
    x = torch.randn((n, 3, h, w), generator=g).to(torch.bfloat16).double()
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dy = (torch.randn((n, 64, ho, wo), generator=g) + 0.5).to(torch.bfloat16).double()
    dw, S = R.stem_wgrad_ref(dy, x)
    bar = R.sum_bar(S)
    d1 = dy.clone()
    d1[1, :, ho - 1] = 0
    R.has_teeth(R.stem_wgrad_ref(d1, x)[0], dw, bar, "one output row missing")
    rows = n * ho                                             # workgroups: min(rows, 1024); the last one owns rows grid-1, 2 grid-1, ...
    grid = min(rows, 1024)
    d2 = dy.clone().permute(0, 2, 1, 3).reshape(rows, 64, wo)
    d2[grid - 1::grid] = 0
    d2 = d2.view(n, ho, 64, wo).permute(0, 2, 1, 3)
    R.has_teeth(R.stem_wgrad_ref(d2, x)[0], dw, bar, "last workgroup partial missing")


def test_bf16_round_toward_zero():
    t = torch.tensor([1.0 + 2.0 ** -7 * 0.75, -(1.0 + 2.0 ** -7 * 0.75), 3.0], dtype=torch.float64)
    assert R.bf16_round_toward_zero(t).tolist() == [1.0, -1.0, 3.0]


def test_relu_ambiguity_scales_with_the_terms():
    """A mask flip is explained only where the pre-activation is within float32 rounding of the |terms| it was summed from."""
    pre = torch.tensor([[[[1e-9]], [[0.5]]]], dtype=torch.float64)
    terms = torch.tensor([[[[40.0]], [[40.0]]]], dtype=torch.float64)
    frac, ok = R.relu_ambiguous(pre, torch.tensor([[[[False]], [[True]]]]), terms)
    assert ok and frac == 0.5
    assert not R.relu_ambiguous(pre, torch.tensor([[[[False]], [[True]]]]))[1]      # without the terms: 1e-9 is not near 0
    assert not R.relu_ambiguous(pre, torch.tensor([[[[True]], [[False]]]]), terms)[1]


# ---- convolutions ------------------------------------------------------------------------------------------------------------------
CONV_CASES = [  # (N, Cin, H, W, Cout, k, stride, pad)
    (2, 3, 5, 3, 4, 3, 1, 1), (2, 3, 5, 3, 4, 3, 2, 1), (1, 2, 6, 6, 3, 3, 2, 1), (2, 2, 7, 5, 3, 3, 2, 0),
    (2, 4, 5, 3, 3, 1, 1, 0), (2, 4, 6, 4, 3, 1, 2, 0), (2, 4, 5, 5, 3, 1, 2, 0), (3, 2, 1, 1, 2, 1, 1, 0),
    (3, 2, 1, 1, 2, 3, 1, 1), (2, 2, 2, 2, 3, 3, 1, 1), (2, 2, 2, 2, 3, 3, 2, 1), (1, 3, 2, 2, 2, 1, 2, 0),
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_references_match_torch(case):
    """conv_fwd_ref / conv_dgrad_ref / conv_wgrad_ref equal F.conv2d / conv2d_input / conv2d_weight in float64, and S bounds |result|."""
    from torch.nn.grad import conv2d_input, conv2d_weight
    n, cin, h, w, cout, k, stride, pad = case
    g = _gen(sum(case))
    x = torch.randn((n, cin, h, w), generator=g, dtype=torch.float64)
    wt = torch.randn((cout, cin, k, k), generator=g, dtype=torch.float64)
    y, S = R.conv_fwd_ref(x, wt, stride, pad)
    ya = F.conv2d(x, wt, None, stride, pad)
    torch.testing.assert_close(y, ya, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(S, F.conv2d(x.abs(), wt.abs(), None, stride, pad), rtol=1e-12, atol=1e-12)
    dy = torch.randn(ya.shape, generator=g, dtype=torch.float64)
    dx, Sx = R.conv_dgrad_ref(dy, wt, x.shape, stride, pad)
    torch.testing.assert_close(dx, conv2d_input(x.shape, wt, dy, stride, pad), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(Sx, conv2d_input(x.shape, wt.abs(), dy.abs(), stride, pad), rtol=1e-12, atol=1e-12)
    dw, Sw = R.conv_wgrad_ref(dy, x, k, stride, pad)
    torch.testing.assert_close(dw, conv2d_weight(x, wt.shape, dy, stride, pad), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(Sw, conv2d_weight(x.abs(), wt.shape, dy.abs(), stride, pad), rtol=1e-12, atol=1e-12)
    for r, s in ((y, S), (dx, Sx), (dw, Sw)):
        assert (s >= r.abs() - 1e-12).all()


def test_join_reference_and_bit_masks():
    """join_ref = mask * (conv + addend + up2(compact)); the bit layout round-trips and its reversed order differs."""
    g = _gen(21)
    shape = (2, 16, 6, 4)
    c = torch.randn(shape, generator=g, dtype=torch.float64)
    a = torch.randn(shape, generator=g, dtype=torch.float64)
    a2 = torch.randn((2, 16, 3, 2), generator=g, dtype=torch.float64)
    m = torch.rand(shape, generator=g) > 0.4
    ref, bar = R.join_ref(c, c.abs(), a, a2, m)
    up = torch.zeros(shape, dtype=torch.float64)
    up[:, :, 0::2, 0::2] = a2
    torch.testing.assert_close(ref, torch.where(m, c + a + up, torch.zeros_like(c)), rtol=0, atol=0)
    assert (bar > 0).all()
    assert torch.equal(R.bits_to_mask(R.mask_to_bits(m), shape), m)
    assert not torch.equal(R.bits_to_mask(R.mask_to_bits(m, reverse=True), shape), m)


# An honest float32 kernel, emulated: exact bf16 x bf16 products summed 16 at a time (one MFMA step), each group added to a float32
# accumulator with one rounding; split-K ranges accumulated from zero and their partials summed in split order in float32.
def _emulate(a, b, splits=1, round_kstep=False, chunk=16):
    """a, b: [E, K] float64 holding bf16 values. Returns float32 results [E] as float64. round_kstep: the defect 'running sum rounded
    to bf16 once per 64-wide K-step'."""
    e, k = a.shape
    groups = (a * b).view(e, k // chunk, chunk).sum(-1)
    nch = groups.shape[1]
    per = -(-nch // splits)
    groups = torch.nn.functional.pad(groups, (0, per * splits - nch)).view(e, splits, per)
    acc = torch.zeros((e, splits), dtype=torch.float32)
    for i in range(per):
        acc = (acc.double() + groups[:, :, i]).float()
        if round_kstep and (i + 1) % (64 // chunk) == 0:
            acc = acc.bfloat16().float()
    out = acc[:, 0]
    for s in range(1, splits):
        out = (out.double() + acc[:, s].double()).float()
    return out.double()


def _operands(e, k, seed, one_signed):
    g = _gen(seed)
    a = torch.randn((e, k), generator=g)
    if one_signed:
        a = torch.relu(a) + 0.01                               # post-ReLU activations: one-signed x
    b = torch.randn((e, k), generator=g) * (2.0 / k) ** 0.5
    return a.bfloat16().double(), b.bfloat16().double()


@pytest.mark.parametrize("k", [576, 4608])
@pytest.mark.parametrize("one_signed", [False, True])
def test_conv_forward_bar_is_sound_and_has_teeth(k, one_signed):
    """bf16 output of one float32 sum: bf16_bar(ref, SUM_REL S) passes the emulated honest kernel (RNE output) at the longest K of the
    network and rejects truncation, per-K-step bf16 rounding of the running sum and a missing 64-channel K block."""
    a, b = _operands(8192, k, k + int(one_signed), one_signed)
    ref = (a * b).sum(1)
    S = (a * b).abs().sum(1)
    bar = R.bf16_bar(ref, R.SUM_REL * S)
    acc = _emulate(a, b)
    honest = R.ratio(acc.bfloat16().double(), ref, bar)
    assert honest <= 1.0, f"honest kernel: ratio {honest:.3g}"
    trunc = R.has_teeth(R.bf16_round_toward_zero(acc), ref, bar, "rounded toward zero")
    kstep = R.has_teeth(_emulate(a, b, round_kstep=True).bfloat16().double(), ref, bar, "running sum rounded per K-step")
    a2 = a.clone()
    a2[:, 64:128] = 0
    block = R.has_teeth(_emulate(a2, b).bfloat16().double(), ref, bar, "missing 64-channel K block")
    print(f"K={k} one_signed={one_signed}: honest {honest:.3g}, truncation {trunc:.3g}, per-K-step bf16 {kstep:.3g}, "
          f"missing block {block:.3g}")


def test_conv_border_tap_bar_has_teeth():
    """A data path that reads the last input row / column as padding (a missing border tap) is rejected by the forward bar."""
    g = _gen(23)
    x = torch.randn((2, 64, 7, 7), generator=g).bfloat16().double()
    w = (torch.randn((64, 64, 3, 3), generator=g) * (2.0 / 576) ** 0.5).bfloat16().double()
    ref, S = R.conv_fwd_ref(x, w, 1, 1)
    bar = R.bf16_bar(ref, R.SUM_REL * S)
    assert R.ratio(ref.float().bfloat16().double(), ref, bar) <= 1.0
    x2 = x.clone()
    x2[:, :, -1, :] = 0
    x2[:, :, :, -1] = 0
    r = R.has_teeth(R.conv_fwd_ref(x2, w, 1, 1)[0].float().bfloat16().double(), ref, bar, "missing border tap")
    print(f"border tap: {r:.3g}")


def test_join_bar_is_sound_and_has_teeth():
    """bf16(bf16(bf16(conv) + addend) + compact) under a mask passes join_ref's bar; the compact addend added at odd pixels, a bit
    mask read in reversed bit order, and truncated roundings are rejected."""
    g = _gen(24)
    shape = (4, 64, 8, 6)
    dy = torch.randn(shape, generator=g).bfloat16().double()
    w = (torch.randn((64, 64, 3, 3), generator=g) * (2.0 / 576) ** 0.5).bfloat16().double()
    conv, S = R.conv_dgrad_ref(dy, w, shape, 1, 1)
    add = torch.randn(shape, generator=g).bfloat16().double()
    a2 = torch.randn((4, 64, 4, 3), generator=g).bfloat16().double()
    mask = torch.rand(shape, generator=g) > 0.5
    up = R.up2(a2, 8, 6)

    def kernel(c32, rnd):
        v = rnd(c32)
        v = rnd(v + add)
        v = torch.where(up != 0, rnd(v + up), v)
        return torch.where(mask, v, torch.zeros_like(v))
    rne = lambda t: t.float().bfloat16().double()               # noqa: E731
    ref, bar = R.join_ref(conv, S, add, a2, mask)
    honest = R.ratio(kernel(conv.float().double(), rne), ref, bar)
    assert honest <= 1.0, honest
    assert torch.equal(kernel(conv.float().double(), rne)[~mask], torch.zeros(int((~mask).sum()), dtype=torch.float64))
    odd = torch.zeros_like(up)
    odd[:, :, 1::2, 1::2] = a2
    bad = rne(rne(conv) + add) + odd
    R.has_teeth(torch.where(mask, rne(bad), torch.zeros_like(bad)), ref, bar, "compact addend at odd pixels")
    rev = R.bits_to_mask(R.mask_to_bits(mask, reverse=True), shape)
    v = kernel(conv.float().double(), rne)
    R.has_teeth(torch.where(rev, rne(rne(rne(conv) + add) + up), torch.zeros_like(v)), ref, bar, "bit order reversed in a mask byte")
    R.has_teeth(kernel(conv.float().double(), R.bf16_round_toward_zero), ref, bar, "join rounded toward zero")
    print(f"join: honest {honest:.3g}")


@pytest.mark.parametrize("one_signed", [False, True])
def test_wgrad_bars_are_sound_and_have_teeth(one_signed):
    """float32 dW at M = 256 * 56^2: the emulated honest split-K kernel passes both bars; a dW missing one 64-pixel K-step or one
    split, or with co and ci transposed, is rejected — the first only thanks to the WGRAD_REL max|ref| bar."""
    m, co, ci, splits = 256 * 56 * 56, 4, 4, 16
    g = _gen(25 + int(one_signed))
    dy = torch.randn((m, co), generator=g).bfloat16().double()
    x = torch.randn((m, ci), generator=g)
    if one_signed:
        x = torch.relu(x)
    x = x.bfloat16().double()
    a = dy.t().repeat_interleave(ci, 0)                        # element (o, i): dy[:, o] . x[:, i]
    b = x.t().repeat(co, 1)
    ref = (a * b).sum(1)
    S = (a * b).abs().sum(1)
    bar = R.wgrad_bar(ref, S)
    got = _emulate(a, b, splits=splits)
    r_sum = R.ratio(got, ref, R.sum_bar(S))
    r_max = R.ratio(got, ref, torch.full_like(ref, R.WGRAD_REL * float(ref.abs().max())))
    assert r_sum <= 1.0 and r_max <= 1.0, f"honest split-K: {r_sum:.3g} of SUM_REL S, {r_max:.3g} of WGRAD_REL max|ref|"
    step = (a[:, 64:128] * b[:, 64:128]).sum(1)
    r_step = R.has_teeth(ref - step, ref, bar, "dW missing one 64-pixel K-step")
    per = -(-m // splits)
    r_split = R.has_teeth(ref - (a[:, :per] * b[:, :per]).sum(1), ref, bar, "dW missing one split")
    r_tr = R.has_teeth(ref.view(co, ci).t().reshape(-1), ref, bar, "dW with co and ci transposed")
    print(f"wgrad one_signed={one_signed}: honest {r_sum:.3g} (S bar) {r_max:.3g} (max bar); K-step {r_step:.3g}, split {r_split:.3g}, "
          f"transposed {r_tr:.3g}, S-bar-only on the K-step {R.ratio(ref - step, ref, R.sum_bar(S)):.3g}")
