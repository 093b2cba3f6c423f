"""-m gpu: the bf16 convolution kernels (dir_conv.hip forward / data gradient, dir_conv_wgrad*.hip weight gradients, the stem forward)
against the float64 per-tap references of tests/bf16_reference.py, per element over whole outputs: every template instantiation of
the four launchers, the AUTO thresholds on both sides, ragged / tiny / non-square maps, every ResNet-50 geometry at batch 256, the fused
data-gradient epilogue (addend, compact stride-2 addend, ReLU mask and bit mask, BatchNorm-backward sums) and the autograd nodes.

Bars (module docstring of bf16_reference.py): bf16 outputs of one float32 sum at half an ulp + 2e-5 S; fused joins with half an ulp per
intermediate rounding, exact zeros where masked; float32 weight gradients at BOTH 2e-5 S and 1e-5 max|ref|; forward statistics at 1e-5.
Every test checks that its bars reject a plausible defect of the reference it just built, and appends its worst ratios to
$DIR_TEST_RECORDS/conv_exact_ratios.jsonl. The last test asserts that the kernels seen under the profiler are exactly EXPECTED_KERNELS."""
import ctypes
import json
import os
import re

import pytest
import torch
import torch.nn as nn

import bf16_reference as R
from conftest import records_dir
from dirhip import _lib as L

pytestmark = pytest.mark.gpu
CL = torch.channels_last

# every instantiation the four launchers can reach (conv_launch_ex, wgrad_impl, wgrad3_impl, dir_stem_conv_fwd), template arguments in
# full (bool as 0 / 1). test_hip_conv_exact_host.py counts the launch sites this list was written for.
EXPECTED_KERNELS = {
    "conv3x3_patch_kernel<56,128,1>", "conv3x3_patch_kernel<56,64,1>", "conv3x3_patch_kernel<28,128,1>",
    "conv3x3_patch_kernel<28,64,1>", "conv3x3_patch_kernel<14,128,1>", "conv3x3_patch_kernel<14,64,1>",
    "conv_igemm_big_kernel<256,256,2,1>", "conv_igemm_big_kernel<256,256,2,0>",
    "conv_igemm_dma_kernel<128,2,0>", "conv_igemm_dma_kernel<64,2,0>", "conv_igemm_dma_kernel<128,1,1>", "conv_igemm_dma_kernel<128,1,0>",
    "conv_igemm_kernel<64,1,1,1>", "conv_igemm_kernel<128,2,2,0>", "conv_igemm_kernel<128,1,2,0>", "conv_igemm_kernel<128,1,1,0>",
    "conv_igemm_kernel<64,2,2,0>", "conv_igemm_kernel<64,1,2,0>", "conv_igemm_kernel<64,1,1,0>",
    "conv_wgrad_kernel<128,128,1,2>", "conv_wgrad_kernel<128,128,0,2>", "conv_wgrad_kernel<128,64,1,1>", "conv_wgrad_kernel<128,64,0,1>",
    "conv_wgrad_kernel<64,128,1,1>", "conv_wgrad_kernel<64,128,0,1>", "conv_wgrad_kernel<64,64,1,1>", "conv_wgrad_kernel<64,64,0,1>",
    "conv_wgrad1_dma_kernel<1>", "conv_wgrad1_dma_kernel<2>", "conv_wgrad_reduce_kernel", "conv_wgrad_reduce_batched_kernel",
    "conv_wgrad3_kernel<56>", "conv_wgrad3_kernel<28>", "conv_wgrad3_kernel<14>", "conv_wgrad3_kernel<7>",
    "stem_conv_kernel",
}
_FAMILY = re.compile(r"(conv3x3_patch_kernel|conv_igemm_big_kernel|conv_igemm_dma_kernel|conv_igemm_kernel|conv_wgrad1_dma_kernel|"
                     r"conv_wgrad3_kernel|conv_wgrad_reduce_batched_kernel|conv_wgrad_reduce_kernel|conv_wgrad_kernel|stem_conv_kernel)")
SEEN = set()


def _canon(name):
    """Profiler kernel name (demangled or mangled) -> 'base<a,b,...>' with bools as 0 / 1, or None outside the four launchers."""
    m = _FAMILY.search(name)
    if m is None:
        return None
    base, rest = m.group(1), name[m.end():]
    t = re.match(r"\s*<([^<>]*)>", rest)
    if t:
        args = []
        for a in t.group(1).split(","):
            a = re.sub(r"\(\w+\)", "", a.strip())
            args.append({"true": "1", "false": "0"}.get(a, a.rstrip("uUlL") if a[:1].isdigit() else a))
        return f"{base}<{','.join(args)}>"
    t = re.match(r"I((?:L[ib]\d+E)+)E", rest)
    if t:
        return base + "<" + ",".join(re.findall(r"L[ib](\d+)E", t.group(1))) + ">"
    return base


class _Profiled:
    """Run the kernels of a test under the profiler; the names of the four launchers' kernels go to SEEN."""

    def __enter__(self):
        from torch.profiler import ProfilerActivity, profile
        self.prof = profile(activities=[ProfilerActivity.CUDA])
        self.prof.__enter__()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.prof.__exit__(*exc)
        if exc[0] is None:
            for e in self.prof.key_averages():
                c = _canon(e.key)
                if c is not None:
                    SEEN.add(c)
        return False


def _record(test, **ratios):
    with open(os.path.join(records_dir(), "conv_exact_ratios.jsonl"), "a") as f:
        f.write(json.dumps(dict(test=test, **{k: round(float(v), 4) for k, v in ratios.items()})) + "\n")


def _bf16(shape, g, one_signed=False, scale=1.0):
    t = torch.randn(shape, device="cuda", generator=g) * scale
    if one_signed:
        t = torch.relu(t)
    return t.to(torch.bfloat16).contiguous(memory_format=CL)


def _weight(cout, cin, k, g):
    return _bf16((cout, cin, k, k), g, scale=(2.0 / (cin * k * k)) ** 0.5)


def _rot(w):
    """Forward weight [Cx, Cy, k, k] -> the data-gradient convolution's operand [Cy, Cx, k, k] (taps rotated by 180 degrees)."""
    return w.flip(2, 3).transpose(0, 1).contiguous(memory_format=CL)


def _fwd_bar(ref, S):
    return R.bf16_bar(ref, R.SUM_REL * S)


def _check_stats(stats, y, name):
    """Epilogue statistics (per-tile column sums) against float64 sums of the kernel's own stored y."""
    tot = stats.double().sum(0)
    yd = y.double()
    s1, s2 = yd.sum(dim=(0, 2, 3)), (yd * yd).sum(dim=(0, 2, 3))
    return max(R.check(tot[0], s1, R.stats_bar(s1), f"{name}: sum"), R.check(tot[1], s2, R.stats_bar(s2), f"{name}: sumsq"))


def _fwd_teeth(x, w, stride, pad, ref, bar, name):
    """Rounded toward zero; input channels 0..63 (one K block) missing."""
    R.has_teeth(R.bf16_round_toward_zero(ref), ref, bar, f"{name}: rounded toward zero")
    blk = R.conv_fwd_ref(x[:, :64], w[:, :64], stride, pad)[0]
    R.has_teeth(ref - blk, ref, bar, f"{name}: one 64-channel K block missing")


def _wgrad_check(dw, dy, x, k, stride, pad, name):
    """Both bars; teeth: the first 64 output pixels (one K-step) missing, co / ci transposed where square."""
    ref, S = R.conv_wgrad_ref(dy, x, k, stride, pad)
    got = dw.double()
    r_s = R.check(got, ref, R.sum_bar(S), f"{name}: dW vs 2e-5 S")
    r_m = R.check(got, ref, torch.full_like(ref, R.WGRAD_REL * float(ref.abs().max())), f"{name}: dW vs 1e-5 max|ref|")
    bar = R.wgrad_bar(ref, S)
    d0 = torch.zeros_like(dy[:1])
    first = d0.permute(0, 2, 3, 1).reshape(-1, dy.shape[1])
    first[:64] = dy[:1].permute(0, 2, 3, 1).reshape(-1, dy.shape[1])[:64]
    d0 = first.view(1, dy.shape[2], dy.shape[3], dy.shape[1]).permute(0, 3, 1, 2)
    R.has_teeth(ref - R.conv_wgrad_ref(d0, x[:1], k, stride, pad)[0], ref, bar, f"{name}: one 64-pixel K-step missing")
    if ref.shape[0] == ref.shape[1]:
        R.has_teeth(ref.transpose(0, 1), ref, bar, f"{name}: co and ci transposed")
    return r_s, r_m


# ---- forward: every instantiation of conv_launch_ex, the AUTO thresholds on both sides ------------------------------------------------
V = L
FWD_CASES = [  # (N, Cin, H, W, Cout, k, stride, pad, variant, kernel the plan must take)
    ((2, 64, 56, 56, 128, 3, 1, 1), V.CONV_PATCH3, "patch<56,128>"), ((2, 64, 56, 56, 64, 3, 1, 1), V.CONV_PATCH3, "patch<56,64>"),
    ((3, 128, 28, 28, 128, 3, 1, 1), V.CONV_PATCH3, "patch<28,128>"), ((3, 128, 28, 28, 64, 3, 1, 1), V.CONV_PATCH3, "patch<28,64>"),
    ((5, 256, 14, 14, 128, 3, 1, 1), V.CONV_PATCH3, "patch<14,128>"), ((5, 256, 14, 14, 64, 3, 1, 1), V.CONV_PATCH3, "patch<14,64>"),
    ((3, 64, 56, 56, 64, 3, 1, 1), V.CONV_AUTO, "patch (AUTO, KT 9 < CVB_MIN_KT)"),
    ((4, 256, 16, 16, 256, 3, 1, 1), V.CONV_BIG, "big lean"),
    ((600, 1024, 8, 8, 256, 1, 1, 0), V.CONV_AUTO, "big (AUTO: KT 16, 150 tiles)"),
    ((596, 1024, 8, 8, 256, 1, 1, 0), V.CONV_AUTO, "single DMA lean (AUTO: 149 tiles < CVB_MIN_TILES)"),
    ((600, 960, 8, 8, 256, 1, 1, 0), V.CONV_AUTO, "single DMA lean (AUTO: KT 15 < CVB_MIN_KT)"),
    ((2, 256, 14, 14, 128, 3, 1, 1), V.CONV_TILE_DMA, "dma<128>"), ((3, 256, 14, 14, 64, 3, 1, 1), V.CONV_TILE_DMA, "dma<64>"),
    ((4, 2048, 7, 7, 128, 1, 1, 0), V.CONV_AUTO, "dma<128> (AUTO: KT 32 = CV_DMA_MIN_KT)"),
    ((3, 2048, 7, 7, 64, 1, 1, 0), V.CONV_AUTO, "dma<64> (AUTO: KT 32)"),
    ((4, 1984, 7, 7, 128, 1, 1, 0), V.CONV_AUTO, "reg<128,1,2> (AUTO: KT 31)"),
    ((3, 128, 28, 28, 128, 3, 2, 1), V.CONV_AUTO, "single DMA lean (AUTO: KT 18, stride 2)"),
    ((3, 128, 28, 28, 128, 3, 2, 1), V.CONV_TILE_REG, "reg<128,1,1>"),
    ((3, 1216, 9, 7, 128, 1, 1, 0), V.CONV_AUTO, "reg<128,1,2> (AUTO: KT 19, ragged M)"),
    ((2, 2240, 5, 3, 128, 1, 1, 0), V.CONV_AUTO, "dma<128> (AUTO: KT 35)"),
    ((2, 256, 9, 13, 128, 3, 1, 1), V.CONV_AUTO, "dma<128> (AUTO: KT 36, non-square)"),
    ((2, 256, 9, 13, 128, 3, 1, 1), V.CONV_TILE_REG, "reg<128,2,2> (KT 36 = the two-tile prefetch)"),
    ((2, 256, 9, 13, 64, 3, 1, 1), V.CONV_TILE_REG, "reg<64,2,2>"), ((2, 2240, 5, 3, 64, 1, 1, 0), V.CONV_TILE_REG, "reg<64,1,2> (KT 35)"),
    ((2, 1216, 5, 3, 64, 1, 1, 0), V.CONV_AUTO, "reg<64,1,2>"),
    ((7, 128, 5, 3, 64, 3, 2, 1), V.CONV_AUTO, "reg<64,1,1> lean (odd N, 5x3)"),
    ((1, 64, 1, 1, 64, 1, 1, 0), V.CONV_AUTO, "1x1 map"), ((3, 64, 2, 2, 128, 3, 1, 1), V.CONV_AUTO, "2x2 map"),
    ((7, 64, 5, 3, 192, 3, 2, 1), V.CONV_AUTO, "Cout 192 (three 64-wide tiles)"),
    ((2, 256, 56, 56, 512, 1, 2, 0), V.CONV_AUTO, "1x1 stride 2"), ((1, 1024, 14, 14, 2048, 1, 2, 0), V.CONV_TILE_REG, "1x1 stride 2 reg"),
    ((2, 512, 7, 7, 512, 3, 1, 1), V.CONV_TILE_REG, "reg<128,2,2> 7x7"), ((2, 512, 7, 7, 512, 3, 1, 1), V.CONV_TILE_DMA, "dma 7x7"),
    # the smallest shapes that still reach a branch of the shared prologue / epilogue: one ragged tile (M = 49) through the LEAN and the
    # pipelined store loops, one 256 x 256 CU tile (M = 256), one or two images through every patch-staged instantiation
    ((1, 64, 7, 7, 64, 3, 1, 1), V.CONV_AUTO, "reg<64,1,1> lean, M = 49"), ((1, 64, 7, 7, 64, 3, 1, 1), V.CONV_TILE_DMA, "dma<64>, M = 49"),
    ((1, 64, 7, 7, 128, 1, 1, 0), V.CONV_AUTO, "single DMA lean, M = 49"), ((1, 64, 16, 16, 256, 3, 1, 1), V.CONV_BIG, "big lean, one tile"),
    ((2, 64, 14, 14, 64, 3, 1, 1), V.CONV_PATCH3, "patch<14,64> N=2"), ((2, 64, 14, 14, 128, 3, 1, 1), V.CONV_PATCH3, "patch<14,128> N=2"),
    ((1, 64, 28, 28, 64, 3, 1, 1), V.CONV_PATCH3, "patch<28,64> N=1"), ((1, 64, 28, 28, 128, 3, 1, 1), V.CONV_PATCH3, "patch<28,128> N=1"),
    ((1, 64, 56, 56, 64, 3, 1, 1), V.CONV_PATCH3, "patch<56,64> N=1"), ((1, 64, 56, 56, 128, 3, 1, 1), V.CONV_PATCH3, "patch<56,128> N=1"),
]


@pytest.mark.parametrize("case,variant,what", FWD_CASES, ids=[f"{c}-v{v}" for c, v, _ in FWD_CASES])
def test_conv_forward_exact(case, variant, what):
    from dirhip.conv import conv2d_igemm
    n, cin, h, w, cout, k, stride, pad = case
    g = torch.Generator(device="cuda").manual_seed(sum(case) + variant)
    x = _bf16((n, cin, h, w), g, one_signed=(n % 2 == 1))
    wt = _weight(cout, cin, k, g)
    with _Profiled():
        y, stats = conv2d_igemm(x, wt, stride, pad, want_stats=True, variant=variant)
    ref, S = R.conv_fwd_ref(x, wt, stride, pad)
    bar = _fwd_bar(ref, S)
    rat = {"y": R.check(y, ref, bar, f"{what}: y"), "stats": _check_stats(stats, y, what)}
    _fwd_teeth(x, wt, stride, pad, ref, bar, what)
    _record(f"fwd[{case}-v{variant}]", **rat)


# ---- every ResNet-50 convolution at batch 256: forward (AUTO, statistics) and weight gradient ------------------------------------------
def _resnet50_geometries(n=256):
    """(N, Cin, H, W, Cout, k, stride, pad) of every convolution of a real bf16 resnet50 forward, collected by patching the conv nodes
    dirhip.resnet binds."""
    from dirhip import resnet as RN
    from dirhip.parallel import DataParallelEngine
    seen = []

    def geo(x, c):
        seen.append((x.shape[0], c.in_channels, x.shape[2], x.shape[3], c.out_channels, c.kernel_size[0], c.stride[0], c.padding[0]))
    orig = (RN.conv_bn_input, RN.projection_pair, RN.stem_conv)

    def cbi(x, conv, *a, **k):
        geo(x, conv)
        return orig[0](x, conv, *a, **k)

    def pp(x, c1, cd, *a, **k):
        geo(x, c1)
        geo(x, cd)
        return orig[1](x, c1, cd, *a, **k)

    def sc(x, conv, *a, **k):
        geo(x, conv)
        return orig[2](x, conv, *a, **k)
    RN.conv_bn_input, RN.projection_pair, RN.stem_conv = cbi, pp, sc
    try:
        torch.manual_seed(0)
        model = RN.resnet50(fds=False, bucket_num=100, bucket_start=0, start_update=0, start_smooth=1, kernel="gaussian", ks=5, sigma=2,
                            momentum=0.9).cuda()
        eng = DataParallelEngine(model, amp_dtype=torch.bfloat16, channels_last=True)
        eng.train()
        x = torch.randn(n, 3, 224, 224, device="cuda")
        t = torch.rand(n, 1, device="cuda") * 80
        with torch.no_grad():
            eng(x, t, 0)
    finally:
        RN.conv_bn_input, RN.projection_pair, RN.stem_conv = orig
    out = []
    for s in seen:
        if s not in out:
            out.append(s)
    return out


def test_resnet50_layers_at_batch_256_exact():
    from dirhip.conv import conv2d_igemm, conv2d_wgrad
    geos = _resnet50_geometries()
    convs = [s for s in geos if s[1] != 3]
    assert len(geos) == len(convs) + 1 and len(convs) == 22, geos          # the stem, and the bottleneck layers' 22 distinct geometries
    g = torch.Generator(device="cuda").manual_seed(256)
    for case in convs:
        n, cin, h, w, cout, k, stride, pad = case
        x = _bf16((n, cin, h, w), g, one_signed=True)                      # post-ReLU activations
        wt = _weight(cout, cin, k, g)
        with _Profiled():
            y, stats = conv2d_igemm(x, wt, stride, pad, want_stats=True)
        ref, S = R.conv_fwd_ref(x, wt, stride, pad)
        bar = _fwd_bar(ref, S)
        rat = {"y": R.check(y, ref, bar, f"{case}: y"), "stats": _check_stats(stats, y, str(case))}
        R.has_teeth(R.bf16_round_toward_zero(ref), ref, bar, f"{case}: rounded toward zero")
        del y, ref, S, bar
        dy = _bf16((n, cout, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1), g)
        with _Profiled():
            dw = conv2d_wgrad(dy, x, k, stride, pad)
        rat["dW_S"], rat["dW_max"] = _wgrad_check(dw, dy, x, k, stride, pad, f"{case}")
        _record(f"resnet50_b256[{case}]", **rat)
        del x, dy, dw
    torch.cuda.empty_cache()


# ---- fused data gradient: dir_conv_dgrad_ex under each variant that takes the geometry ------------------------------------------------
DGRAD_CASES = [  # (N, Cy, H, W, Cx, k, variant, operands)   Cy = channels of dy (the kernel's Cin), Cx = of dx (its Cout)
    ((4, 256, 14, 14, 128, 1), V.CONV_AUTO, "addend+mask"), ((4, 256, 14, 14, 128, 1), V.CONV_TILE_REG, "addend+mask"),
    ((4, 256, 14, 14, 128, 1), V.CONV_TILE_DMA, "addend+bits"), ((4, 256, 14, 14, 64, 1), V.CONV_AUTO, "addend+bits"),
    ((4, 256, 14, 14, 64, 1), V.CONV_TILE_DMA, "mask"), ((3, 64, 9, 13, 128, 3), V.CONV_AUTO, "bnx"),
    ((4, 256, 16, 16, 256, 3), V.CONV_BIG, "addend+bits"), ((4, 256, 16, 16, 256, 3), V.CONV_BIG, "bnx+recompute"),
    ((2, 64, 28, 28, 64, 3), V.CONV_PATCH3, "mask+bnx+recompute"), ((2, 64, 56, 56, 128, 3), V.CONV_AUTO, "bits+bnx+recompute"),
    ((3, 128, 12, 12, 128, 1), V.CONV_AUTO, "s2"), ((3, 128, 12, 12, 128, 1), V.CONV_TILE_REG, "s2+mask"),
    ((3, 128, 12, 10, 64, 1), V.CONV_AUTO, "s2+bits+bnx"), ((3, 128, 12, 12, 128, 1), V.CONV_AUTO, "addend+s2+mask"),
    ((5, 512, 7, 7, 512, 3), V.CONV_AUTO, "addend+mask"), ((2, 2048, 7, 7, 128, 1), V.CONV_AUTO, "addend+bits+bnx"),
    # (kernel form x epilogue option) pairs the cases above do not reach, at the smallest shapes that do. The both-addends loop
    # (addend+s2) with the bit mask, the BatchNorm sums with and without gamma, on 64-wide tiles and under the register-staged
    # (one- and two-tile prefetch), two-stage LDS-DMA and patch-staged K loops:
    ((2, 64, 8, 8, 64, 1), V.CONV_AUTO, "addend+s2+bits+bnx+recompute"), ((2, 64, 8, 8, 64, 3), V.CONV_TILE_REG, "addend+s2+mask+bnx"),
    ((2, 256, 8, 8, 64, 3), V.CONV_TILE_REG, "addend+s2+bits"), ((2, 256, 8, 8, 128, 3), V.CONV_TILE_DMA, "addend+s2+mask+bnx+recompute"),
    ((1, 64, 56, 56, 128, 3), V.CONV_PATCH3, "addend+s2+mask"),
    # the pipelined loop: a ragged single tile (M = 49), the 256 x 256 CU tile with the mask tensor / the compact addend, the patch-staged
    # kernel with the addends and the bit mask, the two-stage LDS-DMA and two-tile-prefetch loops with the compact addend
    ((1, 64, 7, 7, 64, 1), V.CONV_AUTO, "addend+mask+bnx"), ((1, 64, 7, 7, 128, 3), V.CONV_TILE_DMA, "bits+bnx+recompute"),
    ((1, 64, 16, 16, 256, 3), V.CONV_BIG, "mask+bnx"), ((1, 64, 16, 16, 256, 3), V.CONV_BIG, "s2+bits"),
    ((2, 64, 14, 14, 128, 3), V.CONV_PATCH3, "addend+bits"), ((1, 64, 28, 28, 64, 3), V.CONV_PATCH3, "s2+bnx"),
    ((2, 256, 8, 8, 128, 3), V.CONV_TILE_DMA, "s2+bnx+recompute"), ((2, 256, 8, 8, 128, 3), V.CONV_TILE_REG, "s2+mask"),
    ((2, 64, 8, 8, 128, 1), V.CONV_AUTO, "bits+bnx"),
]


@pytest.mark.parametrize("case,variant,ops", DGRAD_CASES, ids=[f"{c}-v{v}-{o}" for c, v, o in DGRAD_CASES])
def test_conv_dgrad_fused_exact(case, variant, ops):
    n, cy, h, w, cx, k, = case
    pad = k // 2
    g = torch.Generator(device="cuda").manual_seed(sum(case) + variant + len(ops))
    dy = _bf16((n, cy, h, w), g)
    wf = _weight(cy, cx, k, g)                                  # the layer's forward weight: x [Cx] -> y [Cy]
    shape = (n, cx, h, w)
    add = _bf16(shape, g) if "addend" in ops else None
    a2 = _bf16((n, cx, h // 2, w // 2), g) if "s2" in ops else None
    mask_t = _bf16(shape, g) if "mask" in ops else None          # the ReLU output the gradient belongs to: > 0 keeps
    mask = (mask_t.float() > 0) if mask_t is not None else None
    bits = None
    if "bits" in ops:
        mask = torch.rand(shape, device="cuda", generator=g) > 0.45
        bits = R.mask_to_bits(mask)
    bnx = gamma = beta = mean = rstd = stats = None
    rows = 0
    if "bnx" in ops:
        bnx = _bf16(shape, g, scale=1.3)
        if "recompute" in ops:
            gamma = torch.rand(cx, device="cuda", generator=g) + 0.5
            beta = torch.randn(cx, device="cuda", generator=g) * 0.3
            mean = torch.randn(cx, device="cuda", generator=g) * 0.2
            rstd = torch.rand(cx, device="cuda", generator=g) + 0.5
        rows = L.lib().dir_conv_plan_rows(n, h, w, cy, cx, k, k, 1, pad, int(add is not None and a2 is not None), variant)
        assert rows > 0
        stats = torch.empty((rows, 2, cx), device="cuda")
    y = torch.empty(shape, dtype=torch.bfloat16, device="cuda", memory_format=CL)
    with _Profiled():
        L.check(L.lib().dir_conv_dgrad_ex(L.ptr(dy), L.ptr(_rot(wf)), L.ptr(add), L.ptr(a2), L.ptr(mask_t), L.ptr(bits), L.ptr(y), n, h, w, cy,
                                          cx, k, k, pad, L.ptr(bnx), L.ptr(gamma), L.ptr(beta), L.ptr(mean), L.ptr(rstd), L.ptr(stats), rows,
                                          variant, L.stream_ptr()), "dir_conv_dgrad_ex")
    conv, S = R.conv_dgrad_ref(dy, wf, shape, 1, pad)
    ref, bar = R.join_ref(conv, S, add, a2, mask)
    rat = {"dx": R.check(y, ref, bar, f"{ops}: dx")}
    if mask is not None:
        assert torch.equal(y[~mask].double(), torch.zeros(int((~mask).sum()), dtype=torch.float64, device="cuda")), "masked elements not 0"
    if bnx is not None:
        gk = y.double()
        if gamma is not None:
            from test_hip_bn_exact import _recomputed_mask
            gk = torch.where(_recomputed_mask(bnx, gamma, beta, mean, rstd), gk, torch.zeros((), dtype=torch.float64, device="cuda"))
        tot = stats.double().sum(0)
        xb = bnx.double()
        s1, s2 = gk.sum(dim=(0, 2, 3)), (gk * xb).sum(dim=(0, 2, 3))
        rat["sum_g"] = R.check(tot[0], s1, R.sum_bar(gk.abs().sum(dim=(0, 2, 3))), f"{ops}: sum g")
        rat["sum_gx"] = R.check(tot[1], s2, R.sum_bar((gk * xb).abs().sum(dim=(0, 2, 3))), f"{ops}: sum g x")
    # teeth on this reference: toward zero; the compact addend at odd pixels; the bit mask read in reversed bit order
    R.has_teeth(R.bf16_round_toward_zero(ref), ref, bar, f"{ops}: rounded toward zero")
    if a2 is not None:
        odd = torch.zeros_like(ref)
        odd[:, :, 1::2, 1::2] = a2.double()
        bad = ref - R.up2(a2, h, w) + odd
        if mask is not None:
            bad = torch.where(mask, bad, torch.zeros_like(bad))
        R.has_teeth(bad, ref, bar, f"{ops}: compact addend at odd pixels")
    if bits is not None:
        rev = R.bits_to_mask(R.mask_to_bits(mask, reverse=True), shape)
        R.has_teeth(R.join_ref(conv, S, add, a2, rev)[0], ref, bar, f"{ops}: bit order reversed")
    _record(f"dgrad_ex[{case}-v{variant}-{ops}]", **rat)


# ---- stride-2 3x3 data gradient by parity classes: dir_conv_dgrad_s2_ex ------------------------------------------------------------
@pytest.mark.parametrize("variant", [V.CONV_AUTO, V.CONV_TILE_REG, V.CONV_TILE_DMA])
@pytest.mark.parametrize("shape", [(2, 128, 28, 28, 128), (3, 64, 8, 12, 192), (1, 256, 2, 2, 64)])
def test_conv_dgrad_s2_exact(shape, variant):
    from dirhip import conv as C
    n, cx, h, w, cy = shape
    g = torch.Generator(device="cuda").manual_seed(sum(shape) + variant)
    conv = nn.Conv2d(cx, cy, 3, stride=2, padding=1, bias=False).cuda().to(memory_format=CL)
    with torch.no_grad():
        conv.weight.copy_(_weight(cy, cx, 3, g).float())
    wcls = C._prepared(conv)[1]
    assert wcls.dim() == 1
    w16 = conv.weight.detach().to(torch.bfloat16)
    dy = _bf16((n, cy, h // 2, w // 2), g)
    bnx = _bf16((n, cx, h, w), g)
    rows = 4 * L.lib().dir_conv_stats_rows(n, h // 2, w // 2)
    stats = torch.empty((rows, 2, cx), device="cuda")
    dx = torch.empty((n, cx, h, w), dtype=torch.bfloat16, device="cuda", memory_format=CL)
    with _Profiled():
        L.check(L.lib().dir_conv_dgrad_s2_ex(L.ptr(dy), L.ptr(wcls), L.ptr(dx), n, h // 2, w // 2, cy, cx, L.ptr(bnx), None, None, None, None,
                                             L.ptr(stats), rows, variant, L.stream_ptr()), "dir_conv_dgrad_s2_ex")
    ref, S = R.conv_dgrad_ref(dy, w16, (n, cx, h, w), 2, 1)
    bar = _fwd_bar(ref, S)
    rat = {"dx": R.check(dx, ref, bar, "dx")}
    gk, xb = dx.double(), bnx.double()
    tot = stats.double().sum(0)
    rat["sum_g"] = R.check(tot[0], gk.sum(dim=(0, 2, 3)), R.sum_bar(gk.abs().sum(dim=(0, 2, 3))), "sum g")
    rat["sum_gx"] = R.check(tot[1], (gk * xb).sum(dim=(0, 2, 3)), R.sum_bar((gk * xb).abs().sum(dim=(0, 2, 3))), "sum g x")
    R.has_teeth(R.bf16_round_toward_zero(ref), ref, bar, "rounded toward zero")
    w_bad = w16.clone()
    w_bad[:, :, 2, 2] = 0                                        # the bottom-right tap (parity class (0, 0), the border rows) missing
    R.has_teeth(R.conv_dgrad_ref(dy, w_bad, (n, cx, h, w), 2, 1)[0], ref, bar, "tap (2, 2) missing")
    _record(f"dgrad_s2[{shape}-v{variant}]", **rat)


# ---- autograd nodes: _ConvFn and _ProjectionPairFn ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(4, 256, 14, 14, 64, 1, 1, 0), (2, 64, 28, 28, 64, 3, 1, 1), (2, 128, 28, 28, 128, 3, 2, 1),
                                  (2, 64, 15, 15, 64, 3, 2, 1), (2, 256, 14, 14, 512, 1, 2, 0), (3, 128, 9, 7, 128, 3, 1, 1)])
def test_conv_node_gradients_exact(case):
    """conv_bn_input backward: stride-1 1x1 / 3x3 (rotated-weight implicit GEMM), the stride-2 3x3 parity path, and the float32
    fallback (odd map; a lone stride-2 1x1): dx against conv_dgrad_ref of the ORIGINAL bf16 weight, dW against conv_wgrad_ref."""
    from dirhip.conv import conv_bn_input
    n, cin, h, w, cout, k, stride, pad = case
    g = torch.Generator(device="cuda").manual_seed(sum(case) + 7)
    conv = nn.Conv2d(cin, cout, k, stride=stride, padding=pad, bias=False).cuda().to(memory_format=CL)
    with torch.no_grad():
        conv.weight.copy_(_weight(cout, cin, k, g).float())
    x0 = _bf16((n, cin, h, w), g, one_signed=True)
    x = x0.clone().requires_grad_(True)
    with _Profiled():
        y, _ = conv_bn_input(x, conv, want_stats=False)
        dy = _bf16(y.shape, g)
        y.backward(dy)
    w16 = conv.weight.detach().to(torch.bfloat16)
    ref, S = R.conv_fwd_ref(x0, w16, stride, pad)
    rat = {"y": R.check(y.detach(), ref, _fwd_bar(ref, S), "y")}
    dref, dS = R.conv_dgrad_ref(dy, w16, x0.shape, stride, pad)
    bar = _fwd_bar(dref, dS)
    rat["dx"] = R.check(x.grad, dref, bar, "dx")
    R.has_teeth(R.bf16_round_toward_zero(dref), dref, bar, "dx rounded toward zero")
    rat["dW_S"], rat["dW_max"] = _wgrad_check(conv.weight.grad, dy, x0, k, stride, pad, "dW")
    _record(f"conv_node[{case}]", **rat)


@pytest.mark.parametrize("stride", [1, 2])
def test_projection_pair_gradient_exact(stride):
    """_ProjectionPairFn: conv1's data gradient with the downsample conv's (compact, bf16) data gradient added in its store loop,
    against the float64 sum of both data gradients; both weight gradients."""
    from dirhip.conv import projection_pair
    g = torch.Generator(device="cuda").manual_seed(40 + stride)
    n, cin, h = 4, 256, 14
    c1 = nn.Conv2d(cin, 128, 1, bias=False).cuda().to(memory_format=CL)
    cd = nn.Conv2d(cin, 512, 1, stride=stride, bias=False).cuda().to(memory_format=CL)
    with torch.no_grad():
        c1.weight.copy_(_weight(128, cin, 1, g).float())
        cd.weight.copy_(_weight(512, cin, 1, g).float())
    x0 = _bf16((n, cin, h, h), g, one_signed=True)
    x = x0.clone().requires_grad_(True)
    with _Profiled():
        y1, _, yd, _ = projection_pair(x, c1, cd, want_stats=False)
        dy1, dyd = _bf16(y1.shape, g), _bf16(yd.shape, g)
        torch.autograd.backward([y1, yd], [dy1, dyd])
    w1, wd = c1.weight.detach().to(torch.bfloat16), cd.weight.detach().to(torch.bfloat16)
    a, Sa = R.conv_dgrad_ref(dy1, w1, x0.shape, 1, 0)
    if stride == 1:
        b, Sb = R.conv_dgrad_ref(dyd, wd, x0.shape, 1, 0)
        ref, bar = R.join_ref(a, Sa, addend=b)
    else:
        b, Sb = R.conv_fwd_ref(dyd, wd.transpose(0, 1).contiguous(), 1, 0)          # the compact gradient [N, Cin, H/2, W/2]
        ref, bar = R.join_ref(a, Sa, addend_s2=b)
        Sb, b = R.up2(Sb, h, h), R.up2(b, h, h)
    # the addend is itself a bf16 rounding of a float32 sum: its error, carried through the final rounding
    eb = R.SUM_REL * Sb
    bar = bar + (1 + R.BF16_REL) * (eb + R.BF16_REL * (b.abs() + eb))
    assert torch.allclose(ref, a + b, rtol=0, atol=0)
    rat = {"dx": R.check(x.grad, ref, bar, "dx")}
    # (rounding toward zero is not among the teeth here: three roundings of comparable terms allow ~1.5 ulp of the total)
    R.has_teeth(a, ref, bar, "dx without the downsample gradient")
    R.has_teeth(torch.roll(ref - a, 1, dims=3) + a, ref, bar, "downsample gradient one pixel off")
    rat["dW1_S"], rat["dW1_max"] = _wgrad_check(c1.weight.grad, dy1, x0, 1, 1, 0, "dW conv1")
    rat["dWd_S"], rat["dWd_max"] = _wgrad_check(cd.weight.grad, dyd, x0, 1, stride, 0, "dW downsample")
    _record(f"projection_pair[s{stride}]", **rat)


# ---- weight gradients: forms, all-taps 3x3, per-tap, stride 2, partials + batched reduction ------------------------------------------
WGRAD_CASES = [  # (N, Cin, H, W, Cout, k, stride, pad, form)
    ((4, 256, 14, 14, 512, 1, 1, 0), V.WGRAD_AUTO), ((4, 256, 14, 14, 512, 1, 1, 0), V.WGRAD_TRANSPOSE),
    ((4, 256, 14, 14, 512, 1, 1, 0), V.WGRAD_DMA1), ((4, 256, 14, 14, 512, 1, 1, 0), V.WGRAD_DMA2),
    ((33, 128, 7, 7, 128, 1, 1, 0), V.WGRAD_DMA1), ((7, 1024, 5, 3, 256, 1, 1, 0), V.WGRAD_DMA2),
    ((8, 64, 28, 28, 64, 1, 1, 0), V.WGRAD_AUTO), ((8, 64, 28, 28, 128, 1, 1, 0), V.WGRAD_AUTO), ((8, 128, 28, 28, 64, 1, 1, 0), V.WGRAD_AUTO),
    ((2, 64, 9, 13, 64, 3, 1, 1), V.WGRAD_AUTO), ((2, 128, 9, 13, 128, 3, 1, 1), V.WGRAD_AUTO),
    ((2, 64, 9, 13, 128, 3, 1, 1), V.WGRAD_AUTO), ((2, 128, 9, 13, 64, 3, 1, 1), V.WGRAD_AUTO),
    ((4, 256, 14, 14, 512, 1, 2, 0), V.WGRAD_AUTO), ((2, 128, 28, 28, 128, 3, 2, 1), V.WGRAD_AUTO), ((3, 64, 15, 15, 64, 3, 2, 1), V.WGRAD_AUTO),
    ((4, 64, 56, 56, 64, 3, 1, 1), V.WGRAD_AUTO), ((4, 128, 28, 28, 128, 3, 1, 1), V.WGRAD_AUTO),
    ((8, 256, 14, 14, 256, 3, 1, 1), V.WGRAD_AUTO), ((16, 512, 7, 7, 512, 3, 1, 1), V.WGRAD_AUTO),
    ((3, 64, 7, 7, 128, 3, 1, 1), V.WGRAD_AUTO),
]


# the all-taps geometries (3x3 / stride 1 on square 56, 28, 14, 7 maps) once more through the per-tap kernel
WGRAD_PARAMS = [(c, f, False) for c, f in WGRAD_CASES] + [(c, f, True) for c, f in WGRAD_CASES
                                                          if c[5] == 3 and c[6] == 1 and c[2] == c[3] and c[2] in (56, 28, 14, 7)]


@pytest.mark.parametrize("case,form,per_tap", WGRAD_PARAMS, ids=[f"{c}-f{f}-pertap{int(p)}" for c, f, p in WGRAD_PARAMS])
def test_conv_wgrad_exact(case, form, per_tap):
    import variant_switches as VS
    from dirhip import conv as C
    n, cin, h, w, cout, k, stride, pad = case
    g = torch.Generator(device="cuda").manual_seed(sum(case) + form + int(per_tap))
    x = _bf16((n, cin, h, w), g, one_signed=(n % 2 == 0))
    dy = _bf16((n, cout, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1), g)
    prev = VS.set_wgrad3_all_taps(not per_tap)
    try:
        with _Profiled():
            dw = C.conv2d_wgrad(dy, x, k, stride, pad, form=form)
        again = C.conv2d_wgrad(dy, x, k, stride, pad, form=form)
    finally:
        VS.set_wgrad3_all_taps(prev)
    r_s, r_m = _wgrad_check(dw, dy, x, k, stride, pad, f"{case} form {form}")
    assert torch.equal(dw, again), "not bit-reproducible"
    _record(f"wgrad[{case}-f{form}-pertap{int(per_tap)}]", dW_S=r_s, dW_max=r_m)


def test_conv_wgrad_partials_batched_reduction_exact():
    """dir_conv_wgrad_partials / dir_conv_wgrad3x3_partials + ONE dir_conv_wgrad_reduce_batched over both layers."""
    lib = L.lib()
    g = torch.Generator(device="cuda").manual_seed(77)
    cases = [(4, 256, 14, 14, 512, 1), (3, 128, 28, 28, 128, 3)]
    ops, rows, keep = [], [], []
    with _Profiled():
        for n, cin, h, w, cout, k in cases:
            x = _bf16((n, cin, h, w), g, one_signed=True)
            dy = _bf16((n, cout, h, w), g)
            dw = torch.empty((cout, cin, k, k), device="cuda", memory_format=CL)
            splits = ctypes.c_int(0)
            if k == 3:
                ws = torch.empty(lib.dir_conv_wgrad3x3_workspace(n, h, w, cin, cout), dtype=torch.uint8, device="cuda")
                L.check(lib.dir_conv_wgrad3x3_partials(L.ptr(dy), L.ptr(x), ctypes.addressof(splits), n, h, w, cin, cout, L.ptr(ws), ws.numel(),
                                                       L.stream_ptr()), "dir_conv_wgrad3x3_partials")
            else:
                ws = torch.empty(lib.dir_conv_wgrad_workspace(n, h, w, cin, cout, 1, 1, 1, 0, V.WGRAD_AUTO), dtype=torch.uint8, device="cuda")
                L.check(lib.dir_conv_wgrad_partials(L.ptr(dy), L.ptr(x), ctypes.addressof(splits), n, h, w, cin, cout, 1, 1, 1, 0, V.WGRAD_AUTO,
                                                    L.ptr(ws), ws.numel(), L.stream_ptr()), "dir_conv_wgrad_partials")
            assert splits.value >= 1
            rows.append((ws.data_ptr(), splits.value, cout * k * k * cin, dw.data_ptr()))
            ops.append((dy, x, dw, k))
            keep.append(ws)
        tab = torch.tensor(rows, dtype=torch.int64).cuda()
        L.check(lib.dir_conv_wgrad_reduce_batched(L.ptr(tab), len(rows), L.stream_ptr()), "dir_conv_wgrad_reduce_batched")
    rat = {}
    for i, (dy, x, dw, k) in enumerate(ops):
        rat[f"dW{i}_S"], rat[f"dW{i}_max"] = _wgrad_check(dw, dy, x, k, 1, k // 2, f"layer {i}")
    _record("wgrad_partials_batched", **rat)


# ---- stem forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 3, 224, 224), (3, 3, 18, 8), (2, 3, 31, 256), (1, 3, 9, 16), (2, 3, 17, 24), (5, 3, 64, 40)])
def test_stem_conv_forward_exact(shape):
    from dirhip.conv import stem_conv
    g = torch.Generator(device="cuda").manual_seed(sum(shape) + 3)
    conv = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda().to(memory_format=CL)
    with torch.no_grad():
        conv.weight.copy_(torch.randn((64, 3, 7, 7), device="cuda", generator=g) * (2.0 / 147) ** 0.5)
    img = torch.randn(shape, device="cuda", generator=g)
    with _Profiled(), torch.no_grad():
        y, stats = stem_conv(img, conv, want_stats=True)
    x16, w16 = img.to(torch.bfloat16), conv.weight.detach().to(torch.bfloat16)
    ref, S = R.conv_fwd_ref(x16, w16, 2, 3)
    bar = _fwd_bar(ref, S)
    rat = {"y": R.check(y, ref, bar, "y"), "stats": _check_stats(stats, y, "stem")}
    R.has_teeth(R.bf16_round_toward_zero(ref), ref, bar, "rounded toward zero")
    x2 = x16.clone()
    x2[:, :, -1] = 0
    x2[:, :, :, -1] = 0
    R.has_teeth(R.conv_fwd_ref(x2, w16, 2, 3)[0], ref, bar, "last input row / column read as padding")
    _record(f"stem_fwd[{shape}]", **rat)


# ---- whole network, teacher-forced: every weight gradient of one bf16 resnet50 training step at batch 256 ---------------------------
@pytest.mark.parametrize("batched", [False, True])
def test_resnet50_step_weight_gradients_teacher_forced(batched):
    """One product-path training step (batch 256, the batched end-of-pass split-K reduction off / on): every convolution's .grad against
    conv_wgrad_ref of the bf16 input it was given and the dY it received (captured with hooks on the conv nodes dirhip.resnet binds)."""
    import variant_switches as VS
    from dirhip import resnet as RN
    from dirhip.parallel import DataParallelEngine
    from dirhip.train_loop import resolve_loss
    caught = []
    orig = (RN.conv_bn_input, RN.projection_pair, RN.stem_conv)

    def catch(x, conv, y):
        ent = {"conv": conv, "x": x.detach().to(torch.bfloat16)}
        y.register_hook(lambda t: ent.__setitem__("dy", t.detach().to(torch.bfloat16)))
        caught.append(ent)

    def cbi(x, conv, *a, **k):
        out = orig[0](x, conv, *a, **k)
        catch(x, conv, out[0])
        return out

    def pp(x, c1, cd, *a, **k):
        out = orig[1](x, c1, cd, *a, **k)
        catch(x, c1, out[0])
        catch(x, cd, out[2])
        return out

    def sc(x, conv, *a, **k):
        out = orig[2](x, conv, *a, **k)
        catch(x, conv, out[0])
        return out
    prev = VS.set_wgrad_batched_reduce(batched)
    RN.conv_bn_input, RN.projection_pair, RN.stem_conv = cbi, pp, sc
    try:
        torch.manual_seed(0)
        model = RN.resnet50(fds=False, bucket_num=100, bucket_start=0, start_update=0, start_smooth=1, kernel="gaussian", ks=5, sigma=2,
                            momentum=0.9).cuda()
        eng = DataParallelEngine(model, amp_dtype=torch.bfloat16, channels_last=True)
        eng.train()
        g = torch.Generator(device="cuda").manual_seed(2)
        x = torch.randn(256, 3, 224, 224, device="cuda", generator=g)
        t = torch.rand(256, 1, device="cuda", generator=g) * 80
        eng.zero_grad(set_to_none=True)
        with _Profiled():
            loss = resolve_loss("l1")(eng(x, t, 2)[0], t, torch.ones(256, 1, device="cuda"))
            loss.backward()
    finally:
        RN.conv_bn_input, RN.projection_pair, RN.stem_conv = orig
        VS.set_wgrad_batched_reduce(prev)
    assert len(caught) == 53, len(caught)
    worst = {"dW_S": 0.0, "dW_max": 0.0}
    for ent in caught:
        conv = ent["conv"]
        k, stride, pad = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        name = f"{tuple(ent['x'].shape)} -> {conv.out_channels} k{k} s{stride}"
        r_s, r_m = _wgrad_check(conv.weight.grad, ent["dy"], ent["x"], k, stride, pad, name)
        worst["dW_S"], worst["dW_max"] = max(worst["dW_S"], r_s), max(worst["dW_max"], r_m)
    _record(f"resnet50_step_teacher_forced[batched{int(batched)}]", **worst)


# ---- coverage: runs last (file order) ----------------------------------------------------------------------------------------------
def test_every_launcher_instantiation_was_checked():
    """The kernels this module ran under the profiler are exactly the instantiations the four launchers can reach (run the whole
    module: the set is filled by the tests above)."""
    missing = sorted(EXPECTED_KERNELS - SEEN)
    extra = sorted(SEEN - EXPECTED_KERNELS)
    assert not missing and not extra, f"not observed: {missing}; observed but not listed: {extra}"
