"""-m gpu: the BatchNorm, max-pool, stem-tail and stem weight-gradient kernels against the rounding-aware float64 references of
tests/bf16_reference.py, elementwise, at half a bf16 ulp (bf16 outputs) and 2e-5 of the sum of |terms| (float32 reductions). The
references take the kernels' discrete decisions (ReLU mask, near-tie pool routes) as given, and every test also checks that its
bar rejects the reference with a plausible defect applied. Worst measured ratios |got - ref| / bar go to $DIR_TEST_RECORDS."""
import json
import os

import pytest
import torch
import torch.nn as nn

import bf16_reference as R
from conftest import records_dir
from dirhip import _lib as L

pytestmark = pytest.mark.gpu
CL = torch.channels_last
EPS, MOM = 1e-5, 0.1


def _record(test, **ratios):
    with open(os.path.join(records_dir(), "bn_exact_ratios.jsonl"), "a") as f:
        f.write(json.dumps(dict(test=test, **{k: round(float(v), 4) for k, v in ratios.items()})) + "\n")


def _out_bar(dtype, ref, extra=0.0):
    """bf16: half an ulp + float32 slack; float32: 1e-5 relative + 1e-6 of the scale."""
    if dtype == torch.bfloat16:
        return R.bf16_bar(ref, extra)
    ref = ref.double()
    return R.STAT_REL * ref.abs() + R.ABS_SLACK * float(ref.abs().max()) + extra


def _rows(t):
    """[N, C, H, W] -> [M, C] rows in NHWC order (float64)."""
    n, c = t.shape[:2]
    return t.double().permute(0, 2, 3, 1).reshape(-1, c)


def _from_rows(rows, shape):
    n, c, h, w = shape
    return rows.view(n, h, w, c).permute(0, 3, 1, 2)


def _params(c, g):
    gamma = torch.rand(c, device="cuda", generator=g) + 0.5
    beta = torch.randn(c, device="cuda", generator=g) * 0.2
    return gamma, beta


def _dy(shape, dtype, g):
    """Gradient with a per-channel offset as well as noise: makes the sum(g) and sum(g x) terms of dx large enough to test."""
    off = torch.randn(shape[1], device="cuda", generator=g) * 0.7
    return (torch.randn(shape, device="cuda", generator=g) + off.view(1, -1, 1, 1)).to(dtype).contiguous(memory_format=CL)


def _bn_teeth(name, g, x, gamma, beta, mean, var, b, dtype, y_ref=None):
    """The bars of a BatchNorm test reject: dx without -a sum(g)/M; dgamma / dbeta without the rows of row block 0; y rounded toward zero."""
    shape = x.shape
    m = shape[0] * shape[2] * shape[3]
    no_term = b["dx"] + R._c(b["a"] * b["dbeta"] / m)
    R.has_teeth(no_term, b["dx"], _out_bar(dtype, b["dx"], b["dx_extra"]), f"{name}: dx without -a sum(g)/M")
    rows = R.bn_block_rows(m, shape[1], 8 if dtype == torch.bfloat16 else 4, 0).to(x.device)
    g2 = _rows(g).clone()
    g2[rows] = 0
    bd = R.bn_bwd(_from_rows(g2, shape), x, gamma, EPS, mean, var)
    R.has_teeth(bd["dgamma"], b["dgamma"], R.sum_bar(b["S_dgamma"]), f"{name}: dgamma without row block 0")
    R.has_teeth(bd["dbeta"], b["dbeta"], R.sum_bar(b["S_dbeta"]), f"{name}: dbeta without row block 0")
    if y_ref is not None and dtype == torch.bfloat16:
        R.has_teeth(R.bf16_round_toward_zero(y_ref), y_ref, R.bf16_bar(y_ref), f"{name}: y rounded toward zero")


def _conv(cin, cout, k, g, stride=1, padding=None):
    """nn.Conv2d with weights drawn from the test's own generator (the global RNG state is left alone)."""
    with torch.random.fork_rng(devices=[torch.cuda.current_device()]):
        conv = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2 if padding is None else padding, bias=False)
    conv = conv.cuda().to(memory_format=CL)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, device="cuda", generator=g) * (2.0 / (cin * k * k)) ** 0.5)
    return conv


def _recomputed_mask(x, gamma, beta, mean, rstd):
    """The backward's ReLU mask recomputed from x (dir_bn.hip bn_mask_coef): float32 x a + b > 0, a and b rounded from float64."""
    gm, rs = gamma.double(), rstd.double()
    a = (gm * rs).float().view(1, -1, 1, 1)
    b = (beta.double() - mean.double() * gm * rs).float().view(1, -1, 1, 1)
    return x.float() * a + b > 0


def _ws(code, m, c):
    n = L.lib().dir_bn_workspace(code, m, c)
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device="cuda")


# ---- BatchNorm (+ residual) (+ ReLU), training mode ----------------------------------------------------------------------------
SHAPES = [((8, 64, 56, 56), True, False), ((8, 256, 56, 56), True, True), ((4, 512, 28, 28), False, False),
          ((6, 1024, 14, 14), True, True), ((5, 2048, 7, 7), True, True), ((3, 64, 112, 112), True, False),
          ((2, 128, 9, 5), False, True), ((2, 8, 3, 2), True, False)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,relu,has_res", SHAPES)
def test_bn_act_train_exact(dtype, shape, relu, has_res):
    from dirhip.bn import bn_act
    g = torch.Generator(device="cuda").manual_seed(sum(shape) + 101)
    n, c, h, w = shape
    m = n * h * w
    x = (torch.randn(shape, device="cuda", generator=g) * 1.7 + 0.3).to(dtype).contiguous(memory_format=CL)
    r = torch.randn(shape, device="cuda", generator=g).to(dtype).contiguous(memory_format=CL) if has_res else None
    dy = _dy(shape, dtype, g)
    gamma, beta = _params(c, g)
    bn = nn.BatchNorm2d(c).cuda()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(torch.randn(c, device="cuda", generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(c, device="cuda", generator=g) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    xg = x.clone().requires_grad_(True)
    rg = r.clone().requires_grad_(True) if has_res else None
    y = bn_act(xg, bn, relu=relu, residual=rg)
    y.backward(dy)
    # the statistics entry point called directly, for save_mean / save_rstd (same kernels, same y bit for bit)
    code = L.DIR_BF16 if dtype == torch.bfloat16 else L.DIR_F32
    y2 = torch.empty_like(x)
    smean, srstd = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    ws = _ws(code, m, c)
    L.check(L.lib().dir_bn_fwd_train(L.ptr(x), L.ptr(r), L.ptr(y2), code, m, c, L.ptr(gamma), L.ptr(beta), None, None, MOM, EPS,
                                     int(relu), L.ptr(smean), L.ptr(srstd), L.ptr(ws), ws.numel(), L.stream_ptr()), "dir_bn_fwd_train")
    assert torch.equal(y2, y.detach())

    mean, var = R.bn_stats(x)
    pre = R.bn_fwd(x, gamma, beta, EPS, mean, var, r)
    y_ref = torch.relu(pre) if relu else pre
    rat = {}
    rat["y"] = R.check(y.detach(), y_ref, _out_bar(dtype, y_ref), "y")
    rat["save_mean"] = R.check(smean, mean, R.stat_bar(mean), "save_mean")
    rstd = 1.0 / torch.sqrt(var + EPS)
    rat["save_rstd"] = R.check(srstd, rstd, R.stat_bar(rstd), "save_rstd")
    erm, erv = R.running_stats(rm0, rv0, mean, var, m, MOM)
    rat["running_mean"] = R.check(bn.running_mean, erm, R.stat_bar(erm), "running_mean")
    rat["running_var"] = R.check(bn.running_var, erv, R.stat_bar(erv), "running_var")
    if relu:
        mask = y.detach() > 0                                # the kernel's own decision
        frac, ok = R.relu_ambiguous(pre, mask, R.bn_terms(x, gamma, beta, EPS, mean, var, r))
        assert ok and frac < R.AMBIGUOUS_MAX, (frac, ok)
        gm = torch.where(mask, dy.double(), torch.zeros((), dtype=torch.float64, device="cuda"))
    else:
        gm = dy.double()
    b = R.bn_bwd(gm, x, gamma, EPS, mean, var)
    rat["dx"] = R.check(xg.grad, b["dx"], _out_bar(dtype, b["dx"], b["dx_extra"]), "dx")
    if has_res:
        assert torch.equal(rg.grad.double(), gm), "dres"    # the masked gradient, stored as is
    rat["dgamma"] = R.check(bn.weight.grad, b["dgamma"], R.sum_bar(b["S_dgamma"]), "dgamma")
    rat["dbeta"] = R.check(bn.bias.grad, b["dbeta"], R.sum_bar(b["S_dbeta"]), "dbeta")
    _bn_teeth("bn_act", gm, x, gamma, beta, mean, var, b, dtype, y_ref)
    _record(f"bn_act_train[{dtype}-{shape}-relu{int(relu)}-res{int(has_res)}]", **rat)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bn_act_eval_exact(dtype):
    from dirhip.bn import bn_act
    g = torch.Generator(device="cuda").manual_seed(1)
    shape = (4, 256, 14, 14)
    x = torch.randn(shape, device="cuda", generator=g).to(dtype).contiguous(memory_format=CL)
    r = torch.randn(shape, device="cuda", generator=g).to(dtype).contiguous(memory_format=CL)
    bn = nn.BatchNorm2d(256).cuda().eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(256, device="cuda", generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(256, device="cuda", generator=g) + 0.5)
        bn.weight.copy_(torch.rand(256, device="cuda", generator=g) + 0.5)
        bn.bias.copy_(torch.randn(256, device="cuda", generator=g) * 0.2)
        y = bn_act(x, bn, relu=True, residual=r)
    y_ref = torch.relu(R.bn_fwd(x, bn.weight, bn.bias, EPS, bn.running_mean.double(), bn.running_var.double(), r))
    rat = R.check(y, y_ref, _out_bar(dtype, y_ref), "y")
    if dtype == torch.bfloat16:
        R.has_teeth(R.bf16_round_toward_zero(y_ref), y_ref, R.bf16_bar(y_ref), "y rounded toward zero")
    _record(f"bn_act_eval[{dtype}]", y=rat)


@pytest.mark.parametrize("deferred", [False, True])
def test_bn_join_exact(deferred):
    """relu(bn(x) + bn_r(r)) in one apply pass, and its backward (one-pass pair when deferred), against float64."""
    from dirhip.bn import bn_join
    g = torch.Generator(device="cuda").manual_seed(5)
    shape = (8, 256, 14, 14)
    m = 8 * 14 * 14
    x0 = torch.randn(shape, device="cuda", generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
    r0 = (torch.randn(shape, device="cuda", generator=g) * 2 + 0.5).to(torch.bfloat16).contiguous(memory_format=CL)
    dy = _dy(shape, torch.bfloat16, g)
    bn, bn_r = nn.BatchNorm2d(256).cuda(), nn.BatchNorm2d(256).cuda()
    with torch.no_grad():
        for m_ in (bn, bn_r):
            m_.weight.copy_(torch.rand(256, device="cuda", generator=g) + 0.5)
            m_.bias.copy_(torch.randn(256, device="cuda", generator=g) * 0.1)
    x, r = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
    y = bn_join(x, bn, None, r, bn_r, None, relu=True, defer_relu_grad=deferred)
    mask = y.detach() > 0
    if deferred:
        y._dir_relu_flag[0] = True
        y.backward(torch.where(mask, dy, torch.zeros_like(dy)))
    else:
        y.backward(dy)
    mx, vx = R.bn_stats(x0)
    mr, vr = R.bn_stats(r0)
    pre = R.bn_fwd(x0, bn.weight, bn.bias, EPS, mx, vx) + R.bn_fwd(r0, bn_r.weight, bn_r.bias, EPS, mr, vr)
    y_ref = torch.relu(pre)
    rat = {"y": R.check(y.detach(), y_ref, R.bf16_bar(y_ref), "y")}
    terms = R.bn_terms(x0, bn.weight, bn.bias, EPS, mx, vx) + R.bn_terms(r0, bn_r.weight, bn_r.bias, EPS, mr, vr)
    frac, ok = R.relu_ambiguous(pre, mask, terms)
    assert ok and frac < R.AMBIGUOUS_MAX, (frac, ok)
    gm = torch.where(mask, dy.double(), torch.zeros((), dtype=torch.float64, device="cuda"))
    bx = R.bn_bwd(gm, x0, bn.weight, EPS, mx, vx)
    br = R.bn_bwd(gm, r0, bn_r.weight, EPS, mr, vr)
    rat["dx"] = R.check(x.grad, bx["dx"], R.bf16_bar(bx["dx"], bx["dx_extra"]), "dx")
    rat["dr"] = R.check(r.grad, br["dx"], R.bf16_bar(br["dx"], br["dx_extra"]), "dr")
    for name, got, ref, S in (("dgamma", bn.weight.grad, bx["dgamma"], bx["S_dgamma"]), ("dbeta", bn.bias.grad, bx["dbeta"], bx["S_dbeta"]),
                              ("dgamma_r", bn_r.weight.grad, br["dgamma"], br["S_dgamma"]), ("dbeta_r", bn_r.bias.grad, br["dbeta"], br["S_dbeta"])):
        rat[name] = R.check(got, ref, R.sum_bar(S), name)
    for name, got, mean, var in (("x", bn, mx, vx), ("r", bn_r, mr, vr)):
        erm, erv = R.running_stats(torch.zeros(256, device="cuda"), torch.ones(256, device="cuda"), mean, var, m, MOM)
        rat[f"running_mean_{name}"] = R.check(got.running_mean, erm, R.stat_bar(erm), "running_mean")
        rat[f"running_var_{name}"] = R.check(got.running_var, erv, R.stat_bar(erv), "running_var")
    _bn_teeth("bn_join", gm, x0, bn.weight, bn.bias, mx, vx, bx, torch.bfloat16, y_ref)
    _record(f"bn_join[deferred{int(deferred)}]", **rat)


# ---- partial lists of every length: dir_bn_fwd_train_partials / dir_bn_prepare_train / dir_bn_bwd_partials ----------------------
def _split_sums(a, b, n_rows):
    """[M, C] float64 terms a, b -> float32 [R][2][C] partial list of R consecutive (ragged) row groups."""
    gid = _group_ids(a.shape[0], n_rows, a.device)
    out = torch.zeros((n_rows, 2, a.shape[1]), dtype=torch.float64, device=a.device)
    out[:, 0].index_add_(0, gid, a)
    out[:, 1].index_add_(0, gid, b)
    return out.float().contiguous()


def _group_ids(m, n_rows, device):
    return torch.arange(m, device=device) * n_rows // m


@pytest.mark.parametrize("shape", [(8, 64, 40, 40), (2, 512, 40, 40), (2, 64, 32, 32)])
@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 63, 64, 1023, 1024, 1025, 2049, 6272])
def test_bn_partial_lists_exact(shape, n_rows):
    """Synthetic float32 partial lists (from x in float64, R row groups) on both sides of every branch of prepare_impl / bwd_impl:
    R < 1024 (one finalize launch over the list), R >= 1024 with >= 32 row blocks (fold to <= 32 float64 rows, ragged last split),
    and (2, 64, 32, 32): R >= 1024 but 16 row blocks, too few to fold."""
    g = torch.Generator(device="cuda").manual_seed(n_rows + shape[1])
    n, c, h, w = shape
    m = n * h * w
    x = (torch.randn(shape, device="cuda", generator=g) * 1.3 + 0.4).to(torch.bfloat16).contiguous(memory_format=CL)
    dy = _dy(shape, torch.bfloat16, g)
    gamma, beta = _params(c, g)
    xr = _rows(x)
    part = _split_sums(xr, xr * xr, n_rows)
    stream = L.stream_ptr()
    rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    y = torch.empty_like(x)
    smean, srstd = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    ws = _ws(L.DIR_BF16, m, c)
    L.check(L.lib().dir_bn_fwd_train_partials(L.ptr(x), None, L.ptr(y), L.DIR_BF16, m, c, L.ptr(part), n_rows, L.ptr(gamma), L.ptr(beta),
                                              L.ptr(rm), L.ptr(rv), MOM, EPS, 1, L.ptr(smean), L.ptr(srstd), L.ptr(ws), ws.numel(), stream),
            "dir_bn_fwd_train_partials")
    mean, var = R.bn_stats(x)
    rstd = 1.0 / torch.sqrt(var + EPS)
    pre = R.bn_fwd(x, gamma, beta, EPS, mean, var)
    y_ref = torch.relu(pre)
    rat = {"y": R.check(y, y_ref, R.bf16_bar(y_ref), "y")}
    rat["save_mean"] = R.check(smean, mean, R.stat_bar(mean), "save_mean")
    rat["save_rstd"] = R.check(srstd, rstd, R.stat_bar(rstd), "save_rstd")
    erm, erv = R.running_stats(torch.zeros(c, device="cuda"), torch.ones(c, device="cuda"), mean, var, m, MOM)
    rat["running_mean"] = R.check(rm, erm, R.stat_bar(erm), "running_mean")
    rat["running_var"] = R.check(rv, erv, R.stat_bar(erv), "running_var")
    # the same list through dir_bn_prepare_train (the join's and the stem tail's statistics step): coefficients a, b
    coef = torch.empty(2, c, device="cuda")
    m2, r2 = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    L.check(L.lib().dir_bn_prepare_train(L.ptr(x), L.DIR_BF16, m, c, L.ptr(part), n_rows, L.ptr(gamma), L.ptr(beta), None, None, MOM, EPS,
                                         L.ptr(m2), L.ptr(r2), L.ptr(coef), L.ptr(ws), ws.numel(), stream), "dir_bn_prepare_train")
    assert torch.equal(m2, smean) and torch.equal(r2, srstd)
    a, b_, _ = R.bn_coef(gamma, beta, mean, var, EPS)
    rat["coef_a"] = R.check(coef[0], a, R.stat_bar(a), "coef a")
    rat["coef_b"] = R.check(coef[1], b_, R.stat_bar(b_), "coef b")
    # backward from a partial list of (sum g, sum g x) with the ReLU mask recomputed from x
    mask = y > 0
    frac, ok = R.relu_ambiguous(pre, mask, R.bn_terms(x, gamma, beta, EPS, mean, var))
    assert ok and frac < R.AMBIGUOUS_MAX, (frac, ok)
    # dir_bn_bwd_partials is given no saved output: it recomputes the mask from x with the forward's float32 coefficients
    # (bn_mask_coef). The reference masks with the forward's y > 0; the two must be the same decision, checked here on its own
    assert torch.equal(_recomputed_mask(x, gamma, beta, smean, srstd), mask), "recomputed ReLU mask differs from the forward's"
    gm = torch.where(mask, dy.double(), torch.zeros((), dtype=torch.float64, device="cuda"))
    gr = _rows(gm)
    bpart = _split_sums(gr, gr * xr, n_rows)
    dx = torch.empty_like(x)
    dgamma, dbeta = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    L.check(L.lib().dir_bn_bwd_partials(L.ptr(dy), L.ptr(x), L.ptr(dx), L.DIR_BF16, m, c, L.ptr(gamma), L.ptr(beta), L.ptr(smean),
                                        L.ptr(srstd), L.ptr(dgamma), L.ptr(dbeta), 1, L.ptr(bpart), n_rows, L.ptr(ws), ws.numel(), stream),
            "dir_bn_bwd_partials")
    bb = R.bn_bwd(gm, x, gamma, EPS, mean, var)
    rat["dx"] = R.check(dx, bb["dx"], R.bf16_bar(bb["dx"], bb["dx_extra"]), "dx")
    rat["dgamma"] = R.check(dgamma, bb["dgamma"], R.sum_bar(bb["S_dgamma"]), "dgamma")
    rat["dbeta"] = R.check(dbeta, bb["dbeta"], R.sum_bar(bb["S_dbeta"]), "dbeta")
    # a dropped list row (the ragged last one) is caught
    keep = torch.ones(n_rows, dtype=torch.bool, device="cuda")
    keep[int(_group_ids(m, n_rows, "cuda")[-1])] = False
    drop = bpart[keep].double().sum(0)
    R.has_teeth(drop[1] * rstd - mean * rstd * drop[0], bb["dgamma"], R.sum_bar(bb["S_dgamma"]), "dgamma without the list row of the last data row")
    R.has_teeth(drop[0], bb["dbeta"], R.sum_bar(bb["S_dbeta"]), "dbeta without the list row of the last data row")
    _bn_teeth("partials", gm, x, gamma, beta, mean, var, bb, torch.bfloat16, y_ref)
    _record(f"bn_partials[{shape}-R{n_rows}]", **rat)


# ---- max pool 3x3 / s2 / p1, bf16 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,plateau", [((4, 64, 112, 112), False), ((3, 64, 9, 7), False), ((2, 8, 5, 6), False),
                                           ((2, 16, 10, 12), True), ((3, 64, 9, 7), True)])
def test_maxpool_exact(shape, plateau):
    g = torch.Generator(device="cuda").manual_seed(3 + sum(shape))
    n, c, h, w = shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x = torch.relu(torch.randn(shape, device="cuda", generator=g))
    if plateau:
        x[:, :, : h // 2] = 0.0                              # whole windows of ReLU zeros: the tie rule decides every route there
    x = x.to(torch.bfloat16).contiguous(memory_format=CL)
    y = torch.empty((n, c, ho, wo), dtype=torch.bfloat16, device="cuda", memory_format=CL)
    idx = torch.empty((n, c, ho, wo), dtype=torch.uint8, device="cuda", memory_format=CL)
    stream = L.stream_ptr()
    L.check(L.lib().dir_maxpool3x3s2_fwd(L.ptr(x), L.ptr(y), L.ptr(idx), n, h, w, c, stream), "dir_maxpool3x3s2_fwd")
    dy = _dy((n, c, ho, wo), torch.bfloat16, g)
    dx = torch.empty_like(x)
    L.check(L.lib().dir_maxpool3x3s2_bwd(L.ptr(dy), L.ptr(idx), L.ptr(dx), n, h, w, c, stream), "dir_maxpool3x3s2_bwd")
    best, route, second = R.maxpool_ref(x)
    assert torch.equal(y.double(), best)
    assert torch.equal(idx.long(), route)
    valid = torch.ones_like(route, dtype=torch.bool)
    dx_ref = R.pool_scatter(dy, route, valid, h, w)
    S = R.pool_scatter(dy.double().abs(), route, valid, h, w)
    bar = R.bf16_bar(dx_ref, R.SUM_REL * S)
    rat = R.check(dx, dx_ref, bar, "dx")
    # teeth: the window with the largest |dy| routed to its second-best position
    k = int(dy.double().abs().contiguous().argmax())
    route2 = route.clone().contiguous().view(-1)
    route2[k] = second.reshape(-1)[k]
    R.has_teeth(R.pool_scatter(dy, route2.view_as(route), valid, h, w), dx_ref, bar, "dx routed to the second-best position")
    _record(f"maxpool[{shape}-plateau{int(plateau)}]", dx=rat)


# ---- stem tail: maxpool(relu(bn(x))), both backward forms ------------------------------------------------------------------------
@pytest.mark.parametrize("shape,source", [((4, 64, 32, 32), "own"), ((3, 64, 9, 7), "own"), ((2, 64, 10, 15), "own"),
                                          ((2, 32, 8, 8), "own"), ((8, 64, 56, 56), "own"), ((4, 3, 64, 64), "stem_conv"),
                                          ((3, 3, 18, 16), "stem_conv")])
def test_stem_tail_exact(shape, source):
    g = torch.Generator(device="cuda").manual_seed(6 + sum(shape))
    stream = L.stream_ptr()
    part = None
    if source == "stem_conv":                                # the product's form: statistics from the convolution's epilogue
        from dirhip.conv import stem_conv
        conv = _conv(3, 64, 7, g, stride=2, padding=3)
        img = torch.randn(shape, device="cuda", generator=g)
        with torch.no_grad():
            x, part = stem_conv(img, conv, want_stats=True)
        x = x.contiguous(memory_format=CL)
    else:
        x = torch.randn(shape, device="cuda", generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
    n, c, h, w = x.shape
    m = n * h * w
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    gamma = torch.linspace(0.5, 1.5, c, device="cuda")
    beta = torch.randn(c, device="cuda", generator=g) * 0.3
    mean_k, rstd_k, coef = torch.empty(c, device="cuda"), torch.empty(c, device="cuda"), torch.empty(2, c, device="cuda")
    ws = _ws(L.DIR_BF16, m, c)
    L.check(L.lib().dir_bn_prepare_train(L.ptr(x), L.DIR_BF16, m, c, L.ptr(part), 0 if part is None else part.shape[0], L.ptr(gamma),
                                         L.ptr(beta), None, None, MOM, EPS, L.ptr(mean_k), L.ptr(rstd_k), L.ptr(coef), L.ptr(ws),
                                         ws.numel(), stream), "dir_bn_prepare_train")
    y = torch.empty((n, c, ho, wo), dtype=torch.bfloat16, device="cuda", memory_format=CL)
    idx = torch.empty((n, c, ho, wo), dtype=torch.uint8, device="cuda", memory_format=CL)
    xmax = torch.empty_like(y)
    L.check(L.lib().dir_bn_relu_maxpool_fwd_xmax(L.ptr(x), L.ptr(coef), L.ptr(y), L.ptr(idx), L.ptr(xmax), n, h, w, c, stream),
            "dir_bn_relu_maxpool_fwd_xmax")
    dy = _dy((n, c, ho, wo), torch.bfloat16, g)
    pws = torch.empty(L.lib().dir_bn_relu_maxpool_bwd_workspace(c), dtype=torch.uint8, device="cuda")
    got = {}
    for form in ("xmax", "gather"):
        dx, dgamma, dbeta = torch.empty_like(x), torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
        if form == "xmax":
            L.check(L.lib().dir_bn_relu_maxpool_bwd_xmax(L.ptr(dy), L.ptr(idx), L.ptr(x), L.ptr(xmax), L.ptr(dx), n, h, w, c, L.ptr(gamma),
                                                         L.ptr(mean_k), L.ptr(rstd_k), L.ptr(dgamma), L.ptr(dbeta), L.ptr(pws), pws.numel(),
                                                         stream), "dir_bn_relu_maxpool_bwd_xmax")
        else:
            L.check(L.lib().dir_bn_relu_maxpool_bwd(L.ptr(dy), L.ptr(idx), L.ptr(x), L.ptr(dx), n, h, w, c, L.ptr(gamma), L.ptr(mean_k),
                                                    L.ptr(rstd_k), L.ptr(dgamma), L.ptr(dbeta), L.ptr(pws), pws.numel(), stream),
                    "dir_bn_relu_maxpool_bwd")
        got[form] = (dx, dgamma, dbeta)

    mean, var = R.bn_stats(x)
    rstd = 1.0 / torch.sqrt(var + EPS)
    rat = {"save_mean": R.check(mean_k, mean, R.stat_bar(mean), "save_mean"),
           "save_rstd": R.check(rstd_k, rstd, R.stat_bar(rstd), "save_rstd")}
    t = R.stem_tail_ref(x, gamma, beta, EPS, mean, var, kernel_idx=idx)
    amb = float(t["ambiguous"].double().mean())
    assert amb < R.AMBIGUOUS_MAX, amb
    want_idx = torch.where(t["valid"], t["route"], torch.full_like(t["route"], 9))
    assert torch.equal(idx.long(), want_idx), int((idx.long() != want_idx).sum())
    rat["y"] = R.check(y, t["y"], R.bf16_bar(t["y"]), "y")
    gs = R.pool_scatter(dy, t["route"], t["valid"], h, w)
    S_pool = R.pool_scatter(dy.double().abs(), t["route"], t["valid"], h, w)
    b = R.bn_bwd(gs, x, gamma, EPS, mean, var)
    extra = b["dx_extra"] + R._c(b["a"].abs()) * R.SUM_REL * S_pool      # the <= 4 routed dy of a pixel are summed in float32 first
    for form, (dx, dgamma, dbeta) in got.items():
        rat[f"dx_{form}"] = R.check(dx, b["dx"], R.bf16_bar(b["dx"], extra), f"dx ({form})")
        rat[f"dgamma_{form}"] = R.check(dgamma, b["dgamma"], R.sum_bar(b["S_dgamma"]), f"dgamma ({form})")
        rat[f"dbeta_{form}"] = R.check(dbeta, b["dbeta"], R.sum_bar(b["S_dbeta"]), f"dbeta ({form})")
    # teeth: y rounded toward zero; dx without -a sum(g)/M; one window routed to its second-best position
    R.has_teeth(R.bf16_round_toward_zero(t["y"]), t["y"], R.bf16_bar(t["y"]), "y rounded toward zero")
    R.has_teeth(b["dx"] + R._c(b["a"] * b["dbeta"] / m), b["dx"], R.bf16_bar(b["dx"], extra), "dx without -a sum(g)/M")
    k = int((dy.double().abs() * t["valid"]).contiguous().argmax())
    route2 = t["route"].clone().contiguous().view(-1)
    route2[k] = t["second"].reshape(-1)[k]
    b2 = R.bn_bwd(R.pool_scatter(dy, route2.view_as(t["route"]), t["valid"], h, w), x, gamma, EPS, mean, var)
    R.has_teeth(b2["dx"], b["dx"], R.bf16_bar(b["dx"], extra), "dx routed to the second-best position")
    _record(f"stem_tail[{shape}-{source}]", ambiguous=amb, **rat)


# ---- stem weight gradient, called directly ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(1, 5, 8),                 # 3 workgroups: nblocks < 4
                                   (3, 13, 224),              # 21 workgroups: the reduce's ragged tail (21 % 16 != 0), odd H
                                   (8, 257, 16),              # 1032 output rows > the 1024-workgroup cap: persistent workgroups loop
                                   (2, 31, 256),              # W = 256 (Wo = 128, the widest), 32 workgroups
                                   (2, 9, 8), (4, 224, 224)])
def test_stem_wgrad_exact(n, h, w):
    g = torch.Generator(device="cuda").manual_seed(n * 1000 + h + w)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x = torch.randn((n, 3, h, w), device="cuda", generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
    dy = _dy((n, 64, ho, wo), torch.bfloat16, g)
    nbytes = L.lib().dir_stem_conv_wgrad_workspace(n, h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        dw = torch.empty((64, 3, 7, 7), device="cuda", memory_format=CL)
        L.check(L.lib().dir_stem_conv_wgrad(L.ptr(dy), L.ptr(x), L.ptr(dw), n, h, w, L.ptr(ws), ws.numel(), L.stream_ptr()),
                "dir_stem_conv_wgrad")
        outs.append(dw)
    assert torch.equal(outs[0], outs[1]), "not bit-reproducible"
    dyc, xc = dy.double().cpu(), x.double().cpu()
    dw_ref, S = R.stem_wgrad_ref(dyc, xc)
    bar = R.sum_bar(S)
    rat = R.check(outs[0].double().cpu(), dw_ref, bar, "dW")
    # teeth: one output row of one image missing; the rows of the reduce's last workgroup partial missing
    d1 = dyc.clone()
    d1[n - 1, :, ho - 1] = 0
    R.has_teeth(R.stem_wgrad_ref(d1, xc)[0], dw_ref, bar, "one output row missing")
    rows = n * ho
    grid = min(rows, 1024)
    d2 = dyc.clone().permute(0, 2, 1, 3).reshape(rows, 64, wo)
    d2[grid - 1::grid] = 0
    R.has_teeth(R.stem_wgrad_ref(d2.view(n, ho, 64, wo).permute(0, 2, 1, 3), xc)[0], dw_ref, bar, "last workgroup partial missing")
    _record(f"stem_wgrad[{n}x{h}x{w}]", dW=rat)


@pytest.mark.parametrize("w", [12, 20, 264, 512])
def test_stem_wgrad_refuses_unsupported_widths(w):
    n, h = 1, 16
    x = torch.zeros((n, 3, h, w), device="cuda", dtype=torch.bfloat16).contiguous(memory_format=CL)
    dy = torch.zeros((n, 64, (h - 1) // 2 + 1, (w - 1) // 2 + 1), device="cuda", dtype=torch.bfloat16).contiguous(memory_format=CL)
    dw = torch.empty((64, 3, 7, 7), device="cuda", memory_format=CL)
    ws = torch.empty(L.lib().dir_stem_conv_wgrad_workspace(n, h), dtype=torch.uint8, device="cuda")
    rc = L.lib().dir_stem_conv_wgrad(L.ptr(dy), L.ptr(x), L.ptr(dw), n, h, w, L.ptr(ws), ws.numel(), L.stream_ptr())
    assert rc == L.DIR_EUNSUPPORTED, rc


# ---- the conv -> BatchNorm chain, teacher-forced stage by stage ------------------------------------------------------------------
def _bn_stage(name, y, out, gy, gout, bn, rm0, rv0):
    """BatchNorm(+ReLU) node of a chain on the kernel's own inputs: out from y, and gy (the gradient it handed to the convolution)
    from gout (the gradient it was handed). Returns the ratios."""
    n, c, h, w = y.shape
    m = n * h * w
    gamma, beta = bn.weight.detach(), bn.bias.detach()
    mean, var = R.bn_stats(y)
    pre = R.bn_fwd(y, gamma, beta, EPS, mean, var)
    out_ref = torch.relu(pre)
    rat = {"out": R.check(out, out_ref, R.bf16_bar(out_ref), f"{name}: bn out")}
    erm, erv = R.running_stats(rm0, rv0, mean, var, m, MOM)
    rat["running_mean"] = R.check(bn.running_mean, erm, R.stat_bar(erm), f"{name}: running_mean")
    rat["running_var"] = R.check(bn.running_var, erv, R.stat_bar(erv), f"{name}: running_var")
    mask = out > 0
    frac, ok = R.relu_ambiguous(pre, mask, R.bn_terms(y, gamma, beta, EPS, mean, var))
    assert ok and frac < R.AMBIGUOUS_MAX, (frac, ok)
    gm = torch.where(mask, gout.double(), torch.zeros((), dtype=torch.float64, device="cuda"))
    b = R.bn_bwd(gm, y, gamma, EPS, mean, var)
    rat["bn_dx"] = R.check(gy, b["dx"], R.bf16_bar(b["dx"], b["dx_extra"]), f"{name}: gradient handed to the convolution")
    rat["dgamma"] = R.check(bn.weight.grad, b["dgamma"], R.sum_bar(b["S_dgamma"]), f"{name}: dgamma")
    rat["dbeta"] = R.check(bn.bias.grad, b["dbeta"], R.sum_bar(b["S_dbeta"]), f"{name}: dbeta")
    _bn_teeth(name, gm, y, gamma, beta, mean, var, b, torch.bfloat16, out_ref)
    return rat


def _bn_module(c, g):
    bn = nn.BatchNorm2d(c).cuda()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, device="cuda", generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, device="cuda", generator=g) * 0.2)
    return bn, bn.running_mean.clone(), bn.running_var.clone()


@pytest.mark.parametrize("n,cin,cout,hw,k", [(6, 128, 256, 14, 3),     # the shapes of test_hip_conv.py's chain test
                                             (4, 256, 64, 28, 1)])
def test_conv_bn_chain_teacher_forced(n, cin, cout, hw, k):
    """conv_bn_input -> bn_act(relu) with the statistics from the conv epilogue. A hook captures the bf16 gradient the BatchNorm hands
    to the convolution; then each stage is held to float64 on the kernel's own inputs: the BatchNorm (forward from the conv's bf16
    output, backward from dy), the conv data gradient and the conv weight gradient (both from the captured gradient)."""
    from torch.nn.grad import conv2d_input, conv2d_weight
    from dirhip.bn import bn_act
    from dirhip.conv import conv_bn_input
    g = torch.Generator(device="cuda").manual_seed(n * 100 + cin + cout + k)
    conv = _conv(cin, cout, k, g)
    bn, rm0, rv0 = _bn_module(cout, g)
    x0 = torch.randn(n, cin, hw, hw, device="cuda", generator=g).to(torch.bfloat16).contiguous(memory_format=CL)
    x = x0.clone().requires_grad_(True)
    y, partial = conv_bn_input(x, conv, want_stats=True)
    assert partial is not None
    held = {}
    y.register_hook(lambda t: held.__setitem__("gy", t.detach().clone()))
    out = bn_act(y, bn, relu=True, partial=partial)
    dy = _dy(out.shape, torch.bfloat16, g)
    out.backward(dy)
    gy = held["gy"]
    assert gy.dtype == torch.bfloat16
    rat = _bn_stage("chain", y.detach(), out.detach(), gy, dy, bn, rm0, rv0)
    # conv stages on the captured gradient, float64 on the CPU, the bf16 weights the kernels use
    w16 = conv.weight.detach().to(torch.bfloat16).double().cpu()
    gyc, xc = gy.double().cpu(), x0.double().cpu()
    pad = k // 2
    dx_ref = conv2d_input(xc.shape, w16, gyc, 1, pad)
    S_dx = conv2d_input(xc.shape, w16.abs(), gyc.abs(), 1, pad)
    dx_bar = R.bf16_bar(dx_ref, R.SUM_REL * S_dx)
    rat["conv_dx"] = R.check(x.grad.double().cpu(), dx_ref, dx_bar, "conv data gradient")
    dw_ref = conv2d_weight(xc, w16.shape, gyc, 1, pad)
    dw_bar = R.sum_bar(conv2d_weight(xc.abs(), w16.shape, gyc.abs(), 1, pad))
    rat["conv_dw"] = R.check(conv.weight.grad.double().cpu(), dw_ref, dw_bar, "conv weight gradient")
    # teeth: a data gradient that misses the first input channel's taps; a weight gradient without one image's contribution
    w_bad = w16.clone()
    w_bad[:, 0] = 0
    R.has_teeth(conv2d_input(xc.shape, w_bad, gyc, 1, pad), dx_ref, dx_bar, "conv dx without input channel 0's taps")
    g_bad = gyc.clone()
    g_bad[n - 1] = 0
    R.has_teeth(conv2d_weight(xc, w16.shape, g_bad, 1, pad), dw_ref, dw_bar, "conv dW without the last image")
    _record(f"conv_bn_chain[{n}x{cin}x{hw}->{cout}k{k}]", **rat)


def test_conv_bn_real_chain_long_partial_lists(monkeypatch):
    """The product's path through the long-list folds at 64 x 64 x 56 x 56: conv_bn_input (1x1) emits 1568 epilogue rows of
    statistics, bn_act folds them (forward); the consuming 3x3 convolution's data gradient emits its rows of (sum g, sum g x) through
    the BatchNorm's BwdLink, and the BatchNorm backward folds those. The BatchNorm stage is checked on its own inputs."""
    from dirhip import bn as B
    from dirhip.conv import conv_bn_input
    g = torch.Generator(device="cuda").manual_seed(64)
    conv1, conv2 = _conv(64, 64, 1, g), _conv(64, 64, 3, g)
    bn, rm0, rv0 = _bn_module(64, g)
    x = torch.randn(64, 64, 56, 56, device="cuda", generator=g).to(torch.bfloat16).contiguous(memory_format=CL).requires_grad_(True)
    y, partial = conv_bn_input(x, conv1, want_stats=True)
    assert partial.shape == (1568, 2, 64), partial.shape
    held, seen = {}, {}
    orig = B.BwdLink.is_dout

    def is_dout(self, t):                                    # record whether the BatchNorm backward takes the conv's partial list
        seen["rows"] = None if self.partial is None else self.partial.shape[0]
        seen["same"] = orig(self, t)
        return seen["same"]
    monkeypatch.setattr(B.BwdLink, "is_dout", is_dout)
    y.register_hook(lambda t: held.__setitem__("gy", t.detach().clone()))
    out = B.bn_act(y, bn, relu=True, partial=partial, fuse_bwd_stats=True)
    link = out._dir_bn_link
    out.register_hook(lambda t: held.__setitem__("gout", t.detach().clone()))
    z, _ = conv_bn_input(out, conv2, want_stats=False)
    z.backward(_dy(z.shape, torch.bfloat16, g))
    # the backward ran dir_bn_bwd_partials on the data gradient's list, long enough for the fold (>= 1024 rows)
    assert seen.get("same") and seen["rows"] >= 1024, seen
    # that path recomputes the ReLU mask from x; the reference masks with the forward's out > 0: the same decision
    assert torch.equal(_recomputed_mask(y.detach(), bn.weight.detach(), bn.bias.detach(), link.mean, link.rstd), out.detach() > 0)
    rat = _bn_stage("real chain", y.detach(), out.detach(), held["gy"], held["gout"], bn, rm0, rv0)
    _record(f"conv_bn_real_chain[64x64x56x56-bwd_rows{seen['rows']}]", **rat)
