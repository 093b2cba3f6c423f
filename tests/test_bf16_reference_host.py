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
