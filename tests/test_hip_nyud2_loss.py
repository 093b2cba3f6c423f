"""GPU tests of the fused NYUD2-DIR training loss (``dir_depth_loss`` / ``dirhip.loss_nyud2.weighted_depth_mse_loss`` /
``PixelWeights.loss``) against the float32 numpy restatement of tests/test_nyud2_loss_host.py (held there to torch's CPU kernels and
autograd, bit for bit). Bars:

  dx_unit   bit-equal to the restatement.  The composition it replaces (``PixelWeights.weights`` feeding torch's expression and
            autograd on the GPU) is compared bit for bit as well; the restatement is the yardstick: should a vendor build of the pow
            backward ever differ in the last bit, the kernel still has to equal the restatement.
  loss      within 1 float32 ulp of float32(float64 sum of the restated terms / n): the kernel's float64 sum runs in another order
            than math.fsum, which moves the quotient by ~1e-16 relative, so the float32 rounding can flip at a tie only;
            and no farther from the float64 value than torch's own float32 composition is, plus that ulp.
"""
import functools

import numpy as np
import pytest
import torch

from test_nyud2_loss_host import SHAPES, make_case, restate, tables

pytestmark = pytest.mark.gpu
UNALIGNED = (3, 1, 7, 9)          # placed one element into a larger buffer: the base is 4 bytes past a 16-byte boundary
BATCH = (32, 1, 114, 152)         # the training batch: more quads than one pass of the capped grid covers


def dev(a, lead=0):
    """``a`` on the device, ``lead`` elements into a larger buffer (a contiguous view with a misaligned base for lead % 4 != 0)."""
    a = np.ascontiguousarray(a)
    if not lead:
        return torch.tensor(a).cuda()
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
    view = buf[lead:lead + a.size].view(a.shape)
    view.copy_(torch.tensor(a))
    assert view.data_ptr() % 16 == 4 * (lead % 4) and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def case(shape, tname):
    """(pred, depth, table, restatement) computed once per (shape, table) and shared, read-only, by the tests."""
    table = tables()[tname]
    pred, depth = make_case(shape, 11 + len(shape) + shape[2])
    r = restate(pred, depth, table)
    for a in (pred, depth, r["dx"], r["t"], r["w"]):
        a.setflags(write=False)
    return pred, depth, table, r


def check_loss(got, r, n, what):
    want = r["loss"]
    print(f"{what}: loss {got!r}, restated {float(want)!r}, float64 mean {r['sum64'] / n!r}")
    assert abs(np.float64(got) - np.float64(want)) <= np.spacing(want), what


# ---- value and gradient vs the restatement and vs the composition -----------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("tname", ["inverse_lds", "sqrt_inv", "none"])
def test_loss_and_gradient(shape, tname):
    from dirhip.lds_nyud2 import PixelWeights
    from dirhip.loss_nyud2 import weighted_depth_mse_loss
    pred, depth, table, r = case(shape, tname)
    n, lead = pred.size, (1 if shape == UNALIGNED else 0)
    o, d = dev(pred, lead).requires_grad_(True), dev(depth, lead)
    bw = None if table is None else [np.float32(x) for x in table]
    loss = weighted_depth_mse_loss(o, d, bw)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    loss.backward()
    assert o.grad.shape == o.shape
    assert np.array_equal(o.grad.cpu().numpy(), r["dx"]), "dx_unit differs from the restatement"
    check_loss(loss.item(), r, n, f"{shape} {tname}")
    # today's composition on the same GPU
    o2 = dev(pred, lead).requires_grad_(True)
    w = PixelWeights(bw).weights(d)
    assert np.array_equal(w.cpu().numpy(), r["w"])
    comp = torch.mean(((o2 - d) ** 2) * w)
    comp.backward()
    differ = int((o2.grad.cpu().numpy() != r["dx"]).sum())
    print(f"{shape} {tname}: composition loss {comp.item()!r}; gradient elements that differ from the restatement: {differ}")
    assert differ == 0, "torch's GPU autograd differs from the restatement (the kernel is held to the restatement above)"
    mean64 = r["sum64"] / n
    assert abs(loss.item() - mean64) <= abs(comp.item() - mean64) + np.spacing(r["loss"])


@pytest.mark.parametrize("leads", [(1, 1), (0, 1), (2, 3), (3, 3)])
@pytest.mark.parametrize("need_grad", [True, False])
def test_every_alignment_through_the_entry_point(leads, need_grad):
    """pred / depth at different offsets from a 16-byte boundary; the gradient buffer is aligned, so with a gradient every misaligned
    depth takes the element-wise path, without one (3, 3) and (1, 1) take 16-byte loads behind a lead-in."""
    from dirhip import ops
    for shape in (UNALIGNED, (5, 1, 57, 77), (1, 1, 1, 2)):
        pred, depth, table, r = case(shape, "inverse_lds")
        loss, dx = ops.depth_loss(dev(pred, leads[0]), dev(depth, leads[1]), dev(table), 10.0, need_grad)
        check_loss(loss.item(), r, pred.size, f"{shape} leads {leads}")
        if need_grad:
            assert np.array_equal(dx.cpu().numpy(), r["dx"])
        else:
            assert dx is None


def test_training_batch_and_other_bucket_rules():
    """32 maps of 114 x 152: every workgroup of the capped grid makes several passes. Then tables of 7 and 256 buckets with other
    multipliers (the clamp at both ends, the largest table the LDS layout takes)."""
    from dirhip import ops
    pred, depth, table, r = case(BATCH, "inverse_lds")
    o, d, t = dev(pred), dev(depth), dev(table)
    loss, dx = ops.depth_loss(o, d, t, 10.0, True)
    assert np.array_equal(dx.cpu().numpy(), r["dx"])
    check_loss(loss.item(), r, pred.size, "32 x 114 x 152")
    rng = np.random.default_rng(3)
    pred, depth, _, _ = case((5, 1, 57, 77), "none")
    for nb, mult in ((7, 0.5), (256, 20.0), (1, 10.0)):
        tab = rng.uniform(0.2, 3.0, nb).astype(np.float32)
        r = restate(pred, depth, tab, mult)
        loss, dx = ops.depth_loss(dev(pred), dev(depth), dev(tab), mult, True)
        assert np.array_equal(dx.cpu().numpy(), r["dx"]), (nb, mult)
        check_loss(loss.item(), r, pred.size, f"bucket_num {nb}")


# ---- reproducibility, autograd plumbing ------------------------------------------------------------------------------------------------
def test_two_calls_bit_equal():
    from dirhip import ops
    for shape in ((2, 1, 114, 152), BATCH):
        pred, depth, table, _ = case(shape, "inverse_lds")
        o, d, t = dev(pred), dev(depth), dev(table)
        l1, g1 = ops.depth_loss(o, d, t, 10.0, True)
        l2, g2 = ops.depth_loss(o, d, t, 10.0, True)
        l3, g3 = ops.depth_loss(o, d, t, 10.0, False)
        assert l1.cpu().numpy().tobytes() == l2.cpu().numpy().tobytes() == l3.cpu().numpy().tobytes()
        assert torch.equal(g1, g2) and g3 is None


def test_upstream_factor_and_no_grad():
    from dirhip.loss_nyud2 import weighted_depth_mse_loss
    pred, depth, table, r = case((5, 1, 57, 77), "sqrt_inv")
    o, d = dev(pred).requires_grad_(True), dev(depth)
    loss = weighted_depth_mse_loss(o, d, table)
    loss.backward(torch.tensor(3.0, device="cuda"))
    assert np.array_equal(o.grad.cpu().numpy(), r["dx"] * np.float32(3.0))
    # no gradient wanted: none is allocated, the value is the same
    before = torch.cuda.memory_allocated()
    plain = weighted_depth_mse_loss(o.detach(), d, table)
    assert not plain.requires_grad and plain.grad_fn is None
    assert torch.cuda.memory_allocated() - before < pred.size * 4                                   # the 0-dim loss only
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        again = weighted_depth_mse_loss(o, d, table)
    assert torch.cuda.memory_allocated() - before < pred.size * 4
    assert not again.requires_grad and plain.item() == again.item() == loss.item()
    # a non-contiguous prediction is made contiguous; the gradient comes back in the caller's layout
    wide = dev(np.repeat(pred, 2, axis=3)).requires_grad_(True)
    loss2 = weighted_depth_mse_loss(wide[..., ::2], d, table)
    loss2.backward()
    assert loss2.item() == loss.item() and np.array_equal(wide.grad[..., ::2].cpu().numpy(), r["dx"]) and not wide.grad[..., 1::2].any()
    with pytest.raises(NotImplementedError):
        weighted_depth_mse_loss(o, d.clone().requires_grad_(True), table)
    with pytest.raises(ValueError):
        weighted_depth_mse_loss(o, d[:1], table)


def test_nan_propagates_and_touches_nothing_else():
    from dirhip import ops
    pred, depth, table, r = case((5, 1, 57, 77), "inverse_lds")
    for which in ("depth", "pred"):
        p2, z2 = pred.copy(), depth.copy()
        (z2 if which == "depth" else p2).reshape(-1)[4321] = np.nan
        loss, dx = ops.depth_loss(dev(p2), dev(z2), dev(table), 10.0, True)
        dx = dx.cpu().numpy().reshape(-1)
        assert np.isnan(loss.item()) and np.isnan(dx[4321]), which
        keep = np.arange(dx.size) != 4321
        assert np.array_equal(dx[keep], r["dx"].reshape(-1)[keep]), which
        rn = restate(p2, z2, table)
        assert np.isnan(rn["loss"]) and rn["w"].reshape(-1)[4321] == (1.0 if which == "depth" else r["w"].reshape(-1)[4321])


def test_pixel_weights_loss_equals_the_free_function():
    from dirhip.lds_nyud2 import PixelWeights
    from dirhip.loss_nyud2 import weighted_depth_mse_loss
    for tname in ("inverse_lds", "none"):
        pred, depth, table, r = case((2, 1, 114, 152), tname)
        bw = None if table is None else [np.float32(x) for x in table]
        d = dev(depth)
        o1, o2 = dev(pred).requires_grad_(True), dev(pred).requires_grad_(True)
        pw = PixelWeights(bw)
        a, b = pw.loss(o1, d), weighted_depth_mse_loss(o2, d, bw)
        a.backward(); b.backward()
        assert a.item() == b.item() and torch.equal(o1.grad, o2.grad)
        assert np.array_equal(o1.grad.cpu().numpy(), r["dx"])
        assert pw.loss(o1, d).item() == a.item()                                                    # the cached device table


# ---- what runs ----------------------------------------------------------------------------------------------------------------------------
def test_only_the_loss_kernels_and_one_scale_kernel_run():
    from torch.profiler import ProfilerActivity, profile
    from dirhip.lds_nyud2 import PixelWeights
    pred, depth, table, _ = case((2, 1, 114, 152), "inverse_lds")
    pw = PixelWeights([np.float32(x) for x in table])
    o, d = dev(pred).requires_grad_(True), dev(depth)
    up = torch.tensor(3.0, device="cuda")
    torch.autograd.grad(pw.loss(o, d), o, up)                  # first call uploads the table and allocates the workspace
    torch.cuda.synchronize()

    def kernels(prof):
        assert not any("memcpy" in e.name.lower() or "memset" in e.name.lower() for e in prof.events())
        return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]

    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        loss = pw.loss(o, d)
        torch.cuda.synchronize()
    fwd = kernels(prof)
    print("forward:", fwd)
    assert len(fwd) == 2 and sum("depth_loss_kernel" in k for k in fwd) == 1 and sum("depth_loss_fold_kernel" in k for k in fwd) == 1, fwd
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        torch.autograd.grad(loss, o, up)
        torch.cuda.synchronize()
    bwd = kernels(prof)
    print("backward:", bwd)
    assert len(bwd) == 1 and "scale_by_scalar_kernel" in bwd[0], bwd
