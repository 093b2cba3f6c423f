"""GPU tests of the balanced age evaluator (``dir_age_eval_accumulate`` / ``dirhip.eval_age.ShotEvaluator`` / ``validate`` with
``--device_eval``) against the float64 restatement ``tests/age_eval_reference.py``; its module docstring derives every bar used here:

  counts (e == 0, NUM)     exactly equal
  e*e, e columns           |table - restatement| <= 1e-12 * (the row's sum of |terms|)        float64 reordering of identical terms
  ln column                |table - restatement| <= ln_bound = (1.5 * 2^-53 + 1e-12) * (the row's sum of |ln e|)
"""
import json
import os
import types

import numpy as np
import pytest
import torch

import age_eval_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
REL_GOLDEN = 9.4e-7        # tests/test_age_eval_host.py::test_restatement_matches_reference_goldens: 4 x the measured 2.35e-7
F32_ACC_SAMPLES = 300_000  # samples of the float32-accumulation defect case: 2^-24 per addition vs the 1e-12 bar
NUM_LABELS = 101


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def run_table(pred, label, valid=None, num_labels=NUM_LABELS):
    from dirhip import ops
    t = torch.zeros(num_labels + 1, 5, dtype=torch.float64, device="cuda")
    ops.age_eval_accumulate(pred, label, valid, t)
    return t.cpu().numpy()


def violations(got, want):
    """Names of the bars that ``got`` [rows, 5] misses against the restatement dict ``want``."""
    bad = []
    ref = want["table"]
    if got.shape != ref.shape or not np.array_equal(got[:, 3:], ref[:, 3:]):
        return ["counts"]
    for k, name in enumerate(("se", "ae")):
        if not np.all(np.abs(got[:, k] - ref[:, k]) <= 1e-12 * want["abs"][:, k]):
            bad.append(name)
    if not np.all(np.abs(got[:, 2] - ref[:, 2]) <= want["ln_bound"]):
        bad.append("ln")
    return bad


def check(got, want, what, quiet=False):
    ref = want["table"]
    if not quiet:
        for k in range(3):
            err = np.abs(got[:, k] - ref[:, k])
            bar = want["ln_bound"] if k == 2 else 1e-12 * want["abs"][:, k]
            worst = np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0))
            print(f"{what}: column {R.COLUMNS[k]} max |err| {err.max():.3e}, worst err/bar {worst:.3e}")
    assert violations(got, want) == [], what


def age_case(n, seed, lo=0, hi=120):
    """Labels uniform in lo..hi (NUM_LABELS = 101: 101..120 go to the "other" row); a fixed 5 % are fractional (i % 20 == 7) and a
    fixed 2 % are predicted exactly (i % 50 == 3): the zero-count column and the e > 0 guard of the ln column."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    label = rng.integers(lo, hi + 1, n).astype(np.float32)
    label[i % 20 == 7] += np.float32(0.5)
    pred = (label + rng.normal(0, 6, n)).astype(np.float32)
    pred[i % 50 == 3] = label[i % 50 == 3]
    valid = (rng.uniform(size=n) < 0.8).astype(np.uint8)
    return pred, label, valid


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "validate.npz"))


# ---- table vs restatement ----------------------------------------------------------------------------------------------------
def test_golden_cases_table(g):
    _, num_labels = R.shot_of_rows(g["in_train_labels"])
    for ci in range(3):
        p, l = g[f"in_preds_{ci}"], g[f"in_labels_{ci}"]
        got = run_table(dev(p), dev(l), None, num_labels)
        check(got, R.table(p, l, num_labels), f"golden case {ci}")
        assert got[:, 4].sum() == p.size


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 16385])
def test_alignment_and_tails(n):
    """``pred`` and ``label`` start 0-3 elements past a 16-byte boundary, independently (the quad grid is anchored on ``label``; the
    vector load of ``pred`` needs the same offset), ``valid`` absent or 0-3 bytes past a 4-byte boundary: lead-in and tail quads go
    element by element. The buffers around the slices hold NaN / 1: a read outside [0, n) would show in the sums or in NUM."""
    pred, label, valid = age_case(n, 100 + n)
    want = {None: R.table(pred, label, NUM_LABELS), 1: R.table(pred, label, NUM_LABELS, valid)}
    if n >= 255:
        assert want[None]["table"][NUM_LABELS, 4] > 0 and want[None]["table"][:, 3].sum() > 0       # "other" row and exact predictions occur
    pbuf = [torch.full((n + 8,), float("nan"), device="cuda") for _ in range(4)]
    lbuf = [torch.full((n + 8,), float("nan"), device="cuda") for _ in range(4)]
    vbuf = [torch.ones(n + 8, dtype=torch.uint8, device="cuda") for _ in range(4)]
    pd, ld, vd = dev(pred), dev(label), dev(valid)
    for o in range(4):
        pbuf[o][o:o + n], lbuf[o][o:o + n], vbuf[o][o:o + n] = pd, ld, vd
        assert pbuf[o].data_ptr() % 16 == 0 and lbuf[o].data_ptr() % 16 == 0 and vbuf[o].data_ptr() % 16 == 0
    first = {}
    for po in range(4):
        for lo in range(4):
            for vo in (None, 0, 1, 2, 3):
                v = None if vo is None else vbuf[vo][vo:vo + n]
                got = run_table(pbuf[po][po:po + n], lbuf[lo][lo:lo + n], v)
                key = None if vo is None else 1
                check(got, want[key], f"n={n} pred+{po} label+{lo} valid {vo}", quiet=(po, lo) != (1, 2))
                assert got[:, 4].sum() == (n if vo is None else valid.sum())
                # the sum order depends on the label's offset only (it anchors the quad grid): everything else is bit-equal
                assert np.array_equal(first.setdefault((lo, key), got), got)


def test_skew_one_row_and_every_row_in_every_wave():
    rng = np.random.default_rng(3)
    n = 100_000
    label = np.full(n, 37, np.float32)                                                           # every lane of every wave on one LDS row
    pred = (label + rng.normal(0, 6, n)).astype(np.float32)
    got = run_table(dev(pred), dev(label))
    check(got, R.table(pred, label, NUM_LABELS), "one row")
    assert got[37, 4] == n and got[:, 4].sum() == n
    label = (np.arange(n) % NUM_LABELS).astype(np.float32)                                       # a wave's 256 samples cover all 101 rows
    pred = (label + rng.normal(0, 6, n)).astype(np.float32)
    got = run_table(dev(pred), dev(label))
    check(got, R.table(pred, label, NUM_LABELS), "every row in every wave")
    assert (got[:NUM_LABELS, 4] >= n // NUM_LABELS).all() and got[NUM_LABELS, 4] == 0
    for nl in (1, 255):                                                                          # smallest and largest table
        pred, label, valid = age_case(5000, nl, hi=300)
        check(run_table(dev(pred), dev(label), dev(valid), nl), R.table(pred, label, nl, valid), f"num_labels {nl}")


# ---- reproducibility, accumulation ---------------------------------------------------------------------------------------------
def test_bit_reproducible_and_accumulation_over_calls():
    from dirhip.eval_age import ShotEvaluator
    pred, label, valid = age_case(20011, 8)
    pd, ld, vd = dev(pred), dev(label), dev(valid)
    a, b = run_table(pd, ld, vd), run_table(pd, ld, vd)
    assert np.array_equal(a, b)
    want = R.table(pred, label, NUM_LABELS, valid)
    check(a, want, "one call")
    ev = ShotEvaluator(np.arange(NUM_LABELS))
    cuts = [0, 1, 6, 263, 1287, 1290, 9001, 20011]                                               # 7 ragged calls
    for s, e in zip(cuts[:-1], cuts[1:]):
        ev.update(pd[s:e].view(-1, 1), ld[s:e].view(-1, 1), vd[s:e].bool() if s % 2 else vd[s:e])
    several = ev.table.cpu().numpy()
    assert np.array_equal(several[:, 3:], a[:, 3:])
    check(several, want, "seven calls")
    assert np.all(np.abs(several[:, :2] - a[:, :2]) <= 1e-12 * want["abs"][:, :2]) and np.all(np.abs(several[:, 2] - a[:, 2]) <= 1e-12 * want["abs"][:, 2])
    ev.reset()
    assert not ev.table.cpu().numpy().any()
    ev.update(pd, ld)                                                                            # [B] form, no mask
    check(ev.table.cpu().numpy(), R.table(pred, label, NUM_LABELS), "after reset")
    ev.update(pd[:0], ld[:0])                                                                    # an empty batch adds nothing
    assert ev.results()["overall"]["num"] == 20011


# ---- results() vs the reference's recorded numbers -----------------------------------------------------------------------------------
def test_results_against_reference_goldens_and_masked_garbage(g):
    from dirhip.eval_age import ShotEvaluator
    train = g["in_train_labels"]
    rng = np.random.default_rng(11)
    for ci in range(3):
        p, l, bs = g[f"in_preds_{ci}"], g[f"in_labels_{ci}"], int(g[f"batch_{ci}"])
        ev, masked = ShotEvaluator(train), ShotEvaluator(train)
        for s in range(0, len(l), bs):
            pb, lb = p[s:s + bs], l[s:s + bs]
            ev.update(dev(pb).view(-1, 1), dev(lb).view(-1, 1))
            junk = len(lb) + 5                                                                   # an appended block of rows that must not count
            pj = np.concatenate([pb, rng.choice(np.array([np.nan, np.inf, -1e30, 0.0], np.float32), junk)])
            lj = np.concatenate([lb, rng.choice(np.array([np.nan, 12.0, 25.5, -7.0], np.float32), junk)])
            vj = np.concatenate([np.ones(len(lb), bool), np.zeros(junk, bool)])
            masked.update(dev(pj).view(-1, 1), dev(lj).view(-1, 1), dev(vj))
        res = ev.results()
        tri, rows = R.golden_rows(res)
        ref_tri, ref_rows = g[f"ref_validate_{ci}"], g[f"ref_shot_{ci}"]
        rel = max((np.abs(tri - ref_tri) / np.abs(ref_tri)).max(), (np.abs(rows - ref_rows) / np.abs(ref_rows)).max())
        print(f"case {ci}: max relative difference to the reference's numbers {rel:.3e}")
        assert rel <= REL_GOLDEN, (ci, rel)
        assert res["overall"]["num"] == len(l) and all(isinstance(res[s]["num"], int) and isinstance(res[s]["mse"], float) for s in res)
        assert np.array_equal(masked.table.cpu().numpy(), ev.table.cpu().numpy())                # bit-equal: skipped rows add nothing
        assert masked.results() == res


# ---- the float64 bar has teeth -------------------------------------------------------------------------------------------------------
def test_float32_accumulation_misses_the_bar_the_kernel_meets():
    rng = np.random.default_rng(7)
    label = np.full(F32_ACC_SAMPLES, 42, np.float32)
    pred = (label + rng.normal(0, 6, label.size)).astype(np.float32)
    want = R.table(pred, label, NUM_LABELS)
    pd, ld = dev(pred), dev(label)
    check(run_table(pd, ld), want, "3e5 samples in one row")
    e = (pd - ld).abs()                                                                          # the same float32 terms, summed in float32 by torch
    defect = want["table"].copy()
    defect[42, 0], defect[42, 1] = float((e * e).sum(dtype=torch.float32).item()), float(e.sum(dtype=torch.float32).item())
    bad = violations(defect, want)
    print("float32 sums: relative error", abs(defect[42, 0] - want["table"][42, 0]) / want["abs"][42, 0], abs(defect[42, 1] - want["table"][42, 1]) / want["abs"][42, 1])
    assert {"se", "ae"} <= set(bad), bad
    assert {"se", "ae"} <= set(violations(R.table(pred, label, NUM_LABELS, acc_dtype=np.float32)["table"], want))
    # a dropped tail, the mask ignored, fractional labels truncated into their integer's row: each shows in the counts
    p, l, v = age_case(10007, 9)
    full = R.table(p, l, NUM_LABELS, v)
    assert violations(R.table(p[:10004], l[:10004], NUM_LABELS, v[:10004])["table"], full) == ["counts"]
    assert violations(R.table(p, l, NUM_LABELS)["table"], full) == ["counts"]
    assert violations(R.table(p, np.trunc(l), NUM_LABELS, v)["table"], full) == ["counts"]


# ---- validate(--device_eval), one and two ranks -------------------------------------------------------------------------------------
class _Echo(torch.nn.Module):
    def forward(self, inputs):
        return inputs.reshape(inputs.shape[0], -1)[:, :1].clone()


def _device_validate(preds, labels, train, bs, rank, world):
    """``validate`` with ``--device_eval`` over this rank's ``eval_shard`` of (preds, labels), an echo model returning the prediction
    its 'image' carries. Returns the triple and the evaluator's (merged) table."""
    from dirhip.eval_age import ShotEvaluator
    from dirhip.train_main import eval_shard, validate
    idx, valid = eval_shard(len(labels), rank, world, device_eval=True)

    def batches():
        for s in range(0, len(idx), bs):
            i = idx[s:s + bs].numpy()
            inp = torch.zeros(len(i), 3, 2, 2, device="cuda")
            inp[:, 0, 0, 0] = dev(preds[i])
            out = (inp, dev(labels[i]).view(-1, 1), torch.ones(len(i), 1, device="cuda"))
            yield out if valid is None else out + (valid[s:s + bs],)
    ev = ShotEvaluator(train)
    args = types.SimpleNamespace(print_freq=3, device_eval=True)
    tri = validate(batches, (len(idx) + bs - 1) // bs, _Echo(), args, train_labels=train, evaluator=ev)
    return [float(x) for x in tri], ev.table.cpu().numpy()


def _validate_worker(rank, world, port, tmp):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    d = np.load(os.path.join(tmp, "val_in.npz"))
    tri, tab = _device_validate(d["preds"], d["labels"], d["train"], int(d["bs"]), rank, world)
    np.save(os.path.join(tmp, f"val_table{rank}.npy"), tab)
    with open(os.path.join(tmp, f"val_out{rank}.json"), "w") as f:
        json.dump(tri, f)
    dist.destroy_process_group()


def test_validate_device_eval_two_ranks_equal_one_rank(g, tmp_path):
    import torch.multiprocessing as mp
    train = g["in_train_labels"]
    n = 2 * 166 + 1                                                                              # odd: rank 1's shard ends in a padded row
    preds, labels, bs = g["in_preds_1"][:n], g["in_labels_1"][:n], 50
    np.savez(tmp_path / "val_in.npz", preds=preds, labels=labels, train=train, bs=bs)
    port = 37000 + int(np.random.default_rng().integers(0, 2000))
    mp.spawn(_validate_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    tri, single = _device_validate(preds, labels, train, bs, 0, 1)
    _, num_labels = R.shot_of_rows(train)
    want = R.table(preds, labels, num_labels)
    check(single, want, "one process")
    t0, t1 = np.load(tmp_path / "val_table0.npy"), np.load(tmp_path / "val_table1.npy")
    r0, r1 = json.load(open(tmp_path / "val_out0.json")), json.load(open(tmp_path / "val_out1.json"))
    assert np.array_equal(t0, t1) and r0 == r1                                                   # every rank reports the same numbers
    assert np.array_equal(t0[:, 3:], single[:, 3:]) and t0[:, 4].sum() == n                      # the padded row is in no count
    check(t0, want, "two ranks merged")
    assert np.all(np.abs(t0[:, :3] - single[:, :3]) <= 1e-12 * want["abs"])
    # mse, l1: sums of positive terms over NUM; gmean = exp(sum ln e / NUM): a relative 1e-12 * sum|ln e| / NUM from the sum, plus the
    # roundings of the division and exp
    ln_rel = 1e-12 * want["abs"][:, 2].sum() / n + 4 * 2.0 ** -52
    for k, bar in enumerate((1e-12 + 2.0 ** -52, 1e-12 + 2.0 ** -52, ln_rel)):
        assert abs(r0[k] - tri[k]) <= bar * abs(tri[k]), (k, r0[k], tri[k])
    ref = g["ref_validate_1"]                                                                    # the set is golden case 1: the reference's own numbers
    assert np.all(np.abs(np.array(tri) - ref) <= REL_GOLDEN * np.abs(ref)), (tri, ref)


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors_raise_and_do_not_fault():
    from dirhip import ops
    from dirhip._lib import DirHipError
    from dirhip.eval_age import ShotEvaluator
    ev = ShotEvaluator(np.arange(NUM_LABELS))
    x, t = torch.ones(8, device="cuda"), torch.zeros(NUM_LABELS + 1, 5, dtype=torch.float64, device="cuda")
    with pytest.raises(DirHipError, match="no CPU fallback"):
        ev.update(x.cpu(), x)
    with pytest.raises(DirHipError, match="no CPU fallback"):
        ev.update(x, x.cpu())
    with pytest.raises(DirHipError, match="no CPU fallback"):
        ev.update(x, x, torch.ones(8, dtype=torch.bool))
    with pytest.raises(DirHipError):
        ops.age_eval_accumulate(x.cpu(), x, None, t)
    with pytest.raises(TypeError):
        ev.update(x.double(), x)
    with pytest.raises(TypeError):
        ev.update(x, x.half())
    with pytest.raises(TypeError):
        ev.update(x, x, torch.ones(8, device="cuda"))
    with pytest.raises(TypeError):
        ops.age_eval_accumulate(x, x, None, t.float())
    with pytest.raises(ValueError):
        ev.update(x, x[:7])
    with pytest.raises(ValueError):
        ev.update(x, x, torch.ones(9, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.age_eval_accumulate(x, x, None, torch.zeros(NUM_LABELS + 1, 8, dtype=torch.float64, device="cuda"))
    big = torch.zeros(257, 5, dtype=torch.float64, device="cuda")                                # num_labels + 1 = 257 > 256
    with pytest.raises(DirHipError, match="dir_age_eval_accumulate"):
        ops.age_eval_accumulate(x, x, None, big)
    with pytest.raises(DirHipError, match="label rows"):
        ShotEvaluator(np.arange(256))
    torch.cuda.synchronize()
    assert not big.cpu().numpy().any() and not t.cpu().numpy().any() and ev.table is None        # nothing was launched
    ops.age_eval_accumulate(x, x, None, t)                                                       # and the device still works
    assert t.cpu().numpy()[1].tolist() == [0.0, 0.0, 0.0, 8.0, 8.0]
