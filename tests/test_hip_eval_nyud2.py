"""GPU tests of the fused NYUD2-DIR evaluator (``dir_depth_eval_accumulate`` / ``dirhip.eval_nyud2.Evaluator``) against the float64
restatement ``tests/nyud2_eval_reference.py``; its module docstring derives every bar used here:

  counts (delta1-3, NUM)   exactly equal
  d*d, d, d/depth columns  |table - restatement| <= 1e-12 * (the bucket's sum of |terms|)     float64 reordering of identical terms
  LG10 column              |table - restatement| <= lg10_bound (device logf within 1 ulp, restatement's log within 0.5 ulp, both
                           carried through the division by ln10 and the subtraction) — per bucket, from the restatement
"""
import os

import numpy as np
import pytest
import torch

import nyud2_eval_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
REL_GOLDEN = 5e-7          # tests/test_nyud2_eval_host.py::test_restatement_matches_reference_goldens: 4 x the measured 1.25e-7
F32_ACC_PIXELS = 300_000   # pixels of the float32-accumulation defect case: 2^-24 per addition over 3e5 additions vs the 1e-12 bar


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def run_table(pred, depth, mask=None, bucket_num=100, mult=10.0):
    from dirhip import ops
    t = torch.zeros(bucket_num, 8, dtype=torch.float64, device="cuda")
    ops.depth_eval_accumulate(pred, depth, mask, t, mult)
    return t.cpu().numpy()


def violations(got, want):
    """Names of the bars that ``got`` [nb, 8] misses against the restatement dict ``want``."""
    bad = []
    ref = want["table"]
    if not np.array_equal(got[:, 4:], ref[:, 4:]):
        bad.append("counts")
    for k, name in enumerate(("d2", "d", "rel")):
        if not np.all(np.abs(got[:, k] - ref[:, k]) <= 1e-12 * want["abs"][:, k]):
            bad.append(name)
    lg_ok = np.abs(got[:, 3] - ref[:, 3]) <= want["lg10_bound"]
    lg_ok |= (np.isnan(got[:, 3]) & np.isnan(ref[:, 3])) | (np.isinf(ref[:, 3]) & (got[:, 3] == ref[:, 3]))
    if not np.all(lg_ok):
        bad.append("lg10")
    return bad


def check(got, want, what):
    ref = want["table"]
    for k in range(4):
        err = np.abs(got[:, k] - ref[:, k])
        bar = want["lg10_bound"] if k == 3 else 1e-12 * want["abs"][:, k]
        with np.errstate(all="ignore"):
            worst = np.nanmax(np.where(bar > 0, err / bar, 0.0)) if np.isfinite(err).any() else 0.0
        print(f"{what}: column {R.COLUMNS[k]} max |err| {np.nanmax(err) if np.isfinite(err).any() else 0:.3e}, worst err/bar {worst:.3e}")
    assert violations(got, want) == [], what


def smooth_case(rng, n, h, w, H, W, lo=0.03, hi=10.9):
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    depth = np.stack([lo + (hi - lo) * (0.55 * xx + 0.45 * yy) ** (1.0 + 0.3 * i) + 0.03 * rng.standard_normal((H, W)) for i in range(n)])
    depth = np.clip(depth, 0.02, 11.5).astype(np.float32)
    ys, xs = np.linspace(0, H - 1, h).round().astype(int), np.linspace(0, W - 1, w).round().astype(int)
    pred = (depth[:, ys][:, :, xs] * rng.uniform(0.7, 1.45, (n, h, w))).astype(np.float32)
    return pred, depth


def restate_up(pred, depth, mask=None, **kw):
    return R.table(R.bilinear_align_corners(pred, *depth.shape[1:]), depth, mask, **kw)


# ---- table vs restatement ----------------------------------------------------------------------------------------------------
def test_golden_cases_table():
    g = np.load(os.path.join(GOLDEN, "nyud2_eval_ref.npz"))
    check(run_table(dev(g["up_pred"]), dev(g["up_depth"]), dev(g["up_mask"])), restate_up(g["up_pred"], g["up_depth"], g["up_mask"]), "up")
    check(run_table(dev(g["up2_pred"]), dev(g["up2_depth"])), restate_up(g["up2_pred"], g["up2_depth"]), "up2")
    check(run_table(dev(g["flat_pred"]).view(1, 1, -1), dev(g["flat_depth"]).view(1, 1, -1)), R.table(g["flat_pred"], g["flat_depth"]), "flat")
    check(run_table(dev(g["nan_pred"]).view(1, 1, -1), dev(g["nan_depth"]).view(1, 1, -1)), R.table(g["nan_pred"], g["nan_depth"]), "nan")


def test_full_size_masked_upsampling():
    rng = np.random.default_rng(1)
    pred, depth = smooth_case(rng, 4, 114, 152, 480, 640)
    mask = (depth > 0.5) & (rng.uniform(size=depth.shape) < 0.9)
    got = run_table(dev(pred), dev(depth), dev(mask))
    check(got, restate_up(pred, depth, mask), "4 x 114 x 152 -> 480 x 640")
    assert got[:, 7].sum() == mask.sum()


@pytest.mark.parametrize("n,start", [(10007, 1), (10007, 3), (5, 2), (3, 0), (1, 1), (4099, 0)])
def test_flat_odd_length_and_unaligned_start(n, start):
    """1-D call form on views that start 4, 8 or 12 bytes past a 16-byte boundary: lead-in and tail quads go element by element."""
    rng = np.random.default_rng(n + start)
    z = rng.uniform(0.02, 11.5, n + 8).astype(np.float32)
    p = (z * rng.uniform(0.6, 1.7, z.size)).astype(np.float32)
    zd, pd = dev(z)[start:start + n], dev(p)[(start + 1) % 4:(start + 1) % 4 + n]            # the two operands misaligned differently
    md = dev((rng.uniform(size=n + 8) < 0.7).astype(np.uint8))[3:3 + n]
    got = run_table(pd.view(1, 1, -1), zd.view(1, 1, -1), md.view(1, 1, -1))
    s2 = (start + 1) % 4
    check(got, R.table(p[s2:s2 + n], z[start:start + n], md.cpu().numpy()), f"n={n} start={start}")


def test_one_bucket_every_bucket_all_masked_and_odd_bucket_numbers():
    rng = np.random.default_rng(5)
    z = rng.uniform(2.30001, 2.39999, 70001).astype(np.float32)                                # all in bucket 23
    p = (z * rng.uniform(0.6, 1.7, z.size)).astype(np.float32)
    got = run_table(dev(p).view(1, 1, -1), dev(z).view(1, 1, -1))
    check(got, R.table(p, z), "one bucket")
    assert got[23, 7] == z.size and got[:, 7].sum() == z.size
    z = rng.permutation(np.repeat(np.arange(100), 37) / 10.0 + rng.uniform(0.001, 0.099, 3700)).astype(np.float32)   # neighbours in different buckets
    p = (z * rng.uniform(0.6, 1.7, z.size)).astype(np.float32)
    got = run_table(dev(p).view(1, 1, -1), dev(z).view(1, 1, -1))
    check(got, R.table(p, z), "every bucket, shuffled")
    assert (got[:, 7] > 0).all()
    got = run_table(dev(p).view(1, 1, -1), dev(z).view(1, 1, -1), dev(np.zeros(z.size, np.uint8)).view(1, 1, -1))
    assert not got.any()
    for nb, mult in ((7, 0.5), (256, 20.0)):
        check(run_table(dev(p).view(1, 1, -1), dev(z).view(1, 1, -1), None, nb, mult), R.table(p, z, None, mult, nb), f"bucket_num {nb}")


def test_nan_depths_and_non_positive_predictions():
    rng = np.random.default_rng(6)
    z = rng.uniform(0.5, 10.0, 5003).astype(np.float32)
    p = (z * rng.uniform(0.6, 1.7, z.size)).astype(np.float32)
    z[rng.choice(z.size, 400, replace=False)] = np.nan
    got = run_table(dev(p).view(1, 1, -1), dev(z).view(1, 1, -1))
    check(got, R.table(p, z), "NaN depths")
    assert got[:, 7].sum() == z.size - 400 and np.isfinite(got).all()
    z = rng.uniform(1.0, 3.0, 2001).astype(np.float32)
    p = (z * rng.uniform(0.6, 1.7, z.size)).astype(np.float32)
    p[z < 1.5] = rng.choice(np.array([0.0, -0.5], np.float32), int((z < 1.5).sum()))          # buckets 10-14: log(0) = -inf, log(-0.5) = NaN
    got = run_table(dev(p).view(1, 1, -1), dev(z).view(1, 1, -1))
    want = R.table(p, z)
    check(got, want, "non-positive predictions")
    assert not np.isfinite(got[10:15, 3]).any() and np.isfinite(got[15:30, 3]).all()
    assert np.array_equal(np.isnan(got), np.isnan(want["table"]))
    # pred = 0: the ratio is inf and passes no delta; pred < 0: maxOfTwo keeps the negative pred / depth, which the reference counts
    neg = np.bincount(R.bucket_of(z[p < 0]), minlength=100)[10:15]
    assert np.array_equal(got[10:15, 4:7], np.repeat(neg[:, None], 3, axis=1)) and neg.sum() > 0 and (p == 0).sum() > 0


# ---- one bucket rule: the FDS binning, the evaluator and the training loss against the restatement's ------------------------------------
def bucket_rule_depths(mult):
    """float32 depths on and next to every bucket edge k / mult (k = 0..260), the zeros, negatives, the int range's ends, +-inf and
    the smallest denormal; four copies in a seeded order, so that the vector spans several workgroups and mixes buckets in a wave."""
    f32 = np.float32
    edges = (np.arange(261, dtype=f32) / f32(mult)).astype(f32)
    special = np.array([0.0, -0.0, -1e-3, -0.5, -1.0, -7.3, -1e31, 1e31, np.inf, -np.inf, 1.4e-45], f32)
    z = np.concatenate([edges, np.nextafter(edges, f32(-np.inf)), np.nextafter(edges, f32(np.inf)), special]).astype(f32)
    return np.random.default_rng(11).permutation(np.tile(z, 4))


@pytest.mark.parametrize("mult,bucket_num", [(10.0, 100), (0.5, 7), (20.0, 256)])
def test_three_callers_of_the_bucket_rule_agree_with_the_restatement(mult, bucket_num):
    """``dir_fds_bin_scaled``, the NUM column of ``dir_depth_eval_accumulate`` and the weight lookup of ``dir_depth_loss`` put every
    depth into the bucket ``nyud2_eval_reference.bucket_of`` restates: all comparisons exact (integers, and float32 arithmetic
    restated operation by operation)."""
    from dirhip import ops
    from test_nyud2_loss_host import restate
    f32 = np.float32
    # inputs and the three expectations, on the CPU
    z = bucket_rule_depths(mult)
    assert z.dtype == f32 and not np.isnan(z).any() and 3000 < z.size < 5000
    want_bins = R.bucket_of(z, mult, bucket_num)
    want_num = np.bincount(want_bins, minlength=bucket_num)
    with np.errstate(all="ignore"):
        prod = z * f32(mult)
    assert (prod <= -1).any() and (prod >= bucket_num).any()                                   # both clamps are hit
    if (mult, bucket_num) == (10.0, 100):
        assert (want_num > 0).all()                                                            # every bucket occurs
    fin = np.isfinite(z) & (np.abs(z) < 1e15)
    zl = z[fin]
    pl = (zl * f32(1.25) + f32(0.125)).astype(f32)
    wtab = np.arange(1, bucket_num + 1, dtype=f32)                                             # table[b] = b + 1: the weight names the bucket
    want_dx = ((f32(1) / f32(zl.size)) * wtab[want_bins[fin]]) * (f32(2) * (pl - zl))
    assert want_dx.dtype == f32 and np.array_equal(restate(pl, zl, wtab, mult)["dx"], want_dx)  # the loss tests' restatement: same rule
    # the device
    zd = dev(z)
    assert np.array_equal(ops.bin_scaled(zd, mult, 0, bucket_num).cpu().numpy(), want_bins)
    got = run_table(zd.view(1, 1, -1), zd.view(1, 1, -1), None, bucket_num, mult)
    assert np.array_equal(got[:, 7], want_num)
    _, dx = ops.depth_loss(dev(pl), dev(zl), dev(wtab), mult, True)
    assert np.array_equal(dx.cpu().numpy().view(np.uint32), want_dx.view(np.uint32))
    # NaN depths have no bucket: FDS row -1 and not counted. The loss's weight for them cannot be seen on the device (d = pred - NaN
    # makes the term and dx_unit NaN whatever the weight): the loss part pins only that the finite pixels keep their weights, that
    # NaN comes out exactly where the depth is NaN, and that the call does not fault on a NaN bucket
    zn = np.array([np.nan, 0.35, np.nan, np.nan, 4.0, np.nan, np.nan], f32)
    pn = np.full(zn.size, 2.0, f32)
    bins = ops.bin_scaled(dev(zn), mult, 0, bucket_num).cpu().numpy()
    assert np.array_equal(bins, np.where(np.isnan(zn), -1, R.bucket_of(zn, mult, bucket_num)))
    got = run_table(dev(pn).view(1, 1, -1), dev(zn).view(1, 1, -1), None, bucket_num, mult)
    assert got[:, 7].sum() == 2 and np.isfinite(got).all()
    assert not run_table(dev(pn[:1]).view(1, 1, -1), dev(zn[:1]).view(1, 1, -1), None, bucket_num, mult).any()
    loss, dx = ops.depth_loss(dev(pn), dev(zn), dev(wtab), mult, True)
    want = restate(pn, zn, wtab, mult)
    assert want["w"][np.isnan(zn)].tolist() == [1.0] * 5 and np.isnan(loss.item())            # the weight 1 is the restatement's
    assert np.array_equal(dx.cpu().numpy(), want["dx"], equal_nan=True) and np.isnan(want["dx"]).sum() == 5


# ---- each bar rejects a plausible defect, emulated on the restatement ----------------------------------------------------------------
def test_bars_reject_emulated_defects():
    rng = np.random.default_rng(7)
    # float32 running sums: at F32_ACC_PIXELS pixels each addition rounds at 2^-24 relative, 4-5 orders above the 1e-12 bar
    z = rng.uniform(0.7, 9.0, F32_ACC_PIXELS).astype(np.float32)
    p = (z * rng.uniform(0.6, 1.7, z.size)).astype(np.float32)
    want = R.table(p, z)
    got = run_table(dev(p).view(1, 1, -1), dev(z).view(1, 1, -1))
    check(got, want, "3e5 pixels")
    bad = violations(R.table(p, z, acc_dtype=np.float32)["table"], want)
    assert {"d2", "d", "rel"} <= set(bad), bad
    # a dropped tail vector (the last n % 4 + up to 3 elements)
    n = 10007
    assert "counts" in violations(R.table(p[:n - n % 4], z[:n - n % 4])["table"], R.table(p[:n], z[:n]))
    # the bucket taken from the prediction
    assert "counts" in violations(R.table(p[:n], z[:n], bucket_from=p[:n])["table"], R.table(p[:n], z[:n]))
    # the mask ignored
    m = rng.uniform(size=n) < 0.9
    assert "counts" in violations(R.table(p[:n], z[:n])["table"], R.table(p[:n], z[:n], m))
    # <= turned < at a ratio of exactly 1.25 (and its squares): the kernel must count them
    z4 = np.array([2.0, 4.0, 1.6, 3.2, 2.0, 2.0], np.float32)
    p4 = np.array([2.5, 3.2, 2.5, 2.048, 3.90625, 1.0], np.float32)                              # 1.25, 1/1.25, 1.5625, 1/1.5625, 1.953125, 2
    got = run_table(dev(p4).view(1, 1, -1), dev(z4).view(1, 1, -1))
    assert got[:, 4:].sum(axis=0).tolist() == [2.0, 4.0, 5.0, 6.0]
    check(got, R.table(p4, z4), "ratios on the thresholds")
    # upsampling with align_corners=False
    pl, dp = smooth_case(rng, 2, 12, 16, 48, 64)
    want = restate_up(pl, dp)
    check(run_table(dev(pl), dev(dp)), want, "align_corners")
    bad = violations(R.table(R.bilinear_align_corners(pl, 48, 64, align_corners=False), dp)["table"], want)
    assert "d" in bad and "counts" in bad, bad


# ---- reproducibility, accumulation ---------------------------------------------------------------------------------------------
def test_bit_reproducible_and_accumulation_over_calls():
    from dirhip.eval_nyud2 import Evaluator
    rng = np.random.default_rng(8)
    pred, depth = smooth_case(rng, 6, 57, 76, 240, 320)
    mask = rng.uniform(size=depth.shape) < 0.85
    pd, dd, md = dev(pred), dev(depth), dev(mask)
    a, b = run_table(pd, dd, md), run_table(pd, dd, md)
    assert np.array_equal(a, b)
    ev = Evaluator()
    for i in range(0, 6, 2):
        ev.update(pd[i:i + 2, None], dd[i:i + 2, None], md[i:i + 2, None])
    several = ev.table.cpu().numpy()
    assert np.array_equal(several[:, 4:], a[:, 4:])
    want = restate_up(pred, depth, mask)
    check(several, want, "three calls")
    ev.reset()
    assert not ev.table.cpu().numpy().any()
    # the reference's call form on the concatenation of already-masked vectors == the fused form, counts exactly
    up = dev(R.bilinear_align_corners(pred, 240, 320))
    ev(up[md], dd[md])
    check(ev.table.cpu().numpy(), want, "reference call form")


# ---- evaluate_shot() vs the reference's recorded dicts -------------------------------------------------------------------------------
def _rows(d, keys):
    return np.array([[float(d[s][k]) for k in keys] for s in ("overall", "many", "medium", "few")])


def test_evaluate_shot_against_reference_goldens():
    from dirhip.eval_nyud2 import Evaluator
    g = np.load(os.path.join(GOLDEN, "nyud2_eval_ref.npz"))
    keys = [str(k) for k in g["keys"]]
    num = keys.index("NUM")
    ev = Evaluator()
    ev.update(dev(g["up_pred"]), dev(g["up_depth"]), dev(g["up_mask"]))
    cases = [("up", ev.evaluate_shot())]
    ev = Evaluator()
    for i in range(2):
        ev.update(dev(g["up2_pred"][i:i + 1]), dev(g["up2_depth"][i:i + 1]))
    cases.append(("up2", ev.evaluate_shot()))
    ev = Evaluator()
    ev(dev(g["flat_pred"]), dev(g["flat_depth"]))
    cases.append(("flat", ev.evaluate_shot()))
    for name, d in cases:
        got, ref = _rows(d, keys), g[name + "_dict"]
        assert np.array_equal(got[:, num], ref[:, num]), name
        assert all(isinstance(d[s]["NUM"], int) and isinstance(d[s]["RMSE"], float) for s in d)
        deltas = [keys.index(k) for k in ("DELTA1", "DELTA2", "DELTA3")]
        cnt_got, cnt_ref = got[:, deltas] * got[:, [num]], ref[:, deltas] * ref[:, [num]]
        if name == "flat":
            assert np.array_equal(np.rint(cnt_got), np.rint(cnt_ref)), name                       # identical per-pixel inputs: counts exact
        else:                                                                                      # torch's bilinear differs by <= 3 ulp: capped
            up = R.bilinear_align_corners(g[name + "_pred"], *g[name + "_depth"].shape[1:])
            cap = R.delta_flip_cap(up, g[name + "_depth"], 1e-6)
            assert cap <= 1e-3 * up.size and np.all(np.abs(np.rint(cnt_got) - np.rint(cnt_ref)) <= cap), (name, cap)
        cont = [keys.index(k) for k in ("MSE", "RMSE", "ABS_REL", "LG10", "MAE")]
        rel = np.abs(got[:, cont] - ref[:, cont]) / np.abs(ref[:, cont])
        print(name, "max relative difference to the reference's dict", rel.max())
        assert rel.max() <= REL_GOLDEN, (name, rel.max())
    d = Evaluator.evaluate(dev(g["nan_pred"]), dev(g["nan_depth"]))
    ref = g["nan_dict"]
    assert d["NUM"] == int(ref[num]) == 3700
    for i, k in enumerate(keys):
        assert abs(d[k] - ref[i]) <= REL_GOLDEN * abs(ref[i]) + (0.5 / ref[num] if k.startswith("DELTA") else 0), k
    empty = Evaluator().evaluate_shot()
    assert all(v == 0 for s in empty.values() for v in s.values())


# ---- no library kernel between the network output and the table ----------------------------------------------------------------
def test_fused_form_launches_only_the_two_library_kernels():
    from torch.profiler import ProfilerActivity, profile
    from dirhip.eval_nyud2 import Evaluator
    rng = np.random.default_rng(9)
    pred, depth = smooth_case(rng, 2, 57, 76, 240, 320)
    pd, dd, md = dev(pred)[:, None], dev(depth)[:, None], dev(depth > 1.0)[:, None]
    ev = Evaluator()
    ev.update(pd, dd, md)                                     # first call allocates table and workspace
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(3):
            ev.update(pd, dd, md)
        torch.cuda.synchronize()
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()]
    print(sorted(set(kernels)))
    assert len(kernels) == 6 and all("depth_eval" in k or "dir_table_fold" in k for k in kernels), kernels
    assert not any(("Memcpy" in e.name or "memcpy" in e.name) for e in prof.events())


# ---- two ranks ------------------------------------------------------------------------------------------------------------------
def _eval_worker(rank, world, port, tmp):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from dirhip.eval_nyud2 import Evaluator
    d = np.load(os.path.join(tmp, "eval_in.npz"))
    ev = Evaluator()
    for i in range(rank, d["pred"].shape[0], world):
        ev.update(dev(d["pred"][i:i + 1]), dev(d["depth"][i:i + 1]), dev(d["mask"][i:i + 1]))
    ev.merge_across_ranks()
    np.save(os.path.join(tmp, f"eval_out{rank}.npy"), ev.table.cpu().numpy())
    import json
    with open(os.path.join(tmp, f"eval_out{rank}.json"), "w") as f:
        json.dump(ev.evaluate_shot(), f)
    dist.destroy_process_group()


def test_two_ranks_merge_equals_one_rank(tmp_path):
    import json
    import torch.multiprocessing as mp
    from dirhip.eval_nyud2 import Evaluator
    rng = np.random.default_rng(10)
    pred, depth = smooth_case(rng, 6, 30, 40, 120, 160)
    mask = (rng.uniform(size=depth.shape) < 0.8).astype(np.uint8)
    np.savez(tmp_path / "eval_in.npz", pred=pred, depth=depth, mask=mask)
    port = 35000 + int(rng.integers(0, 2000))
    mp.spawn(_eval_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    ev = Evaluator()
    ev.update(dev(pred), dev(depth), dev(mask))
    single, one = ev.table.cpu().numpy(), ev.evaluate_shot()
    t0, t1 = np.load(tmp_path / "eval_out0.npy"), np.load(tmp_path / "eval_out1.npy")
    assert np.array_equal(t0, t1)
    assert np.array_equal(t0[:, 4:], single[:, 4:])
    assert np.all(np.abs(t0[:, :4] - single[:, :4]) <= 1e-12 * np.abs(single[:, :4]))              # positive terms: |sum| = sum of |terms|
    d0, d1 = json.load(open(tmp_path / "eval_out0.json")), json.load(open(tmp_path / "eval_out1.json"))
    assert d0 == d1
    for s in one:
        for k in one[s]:
            assert abs(d0[s][k] - one[s][k]) <= 1e-12 * abs(one[s][k]), (s, k)
