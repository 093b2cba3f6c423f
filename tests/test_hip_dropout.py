"""-m gpu: dropout of the fused network tail (resnet50(dropout=p): nn.Dropout(p) between FDS.smooth and Linear(2048, 1),
resnet.py:98-101,146-147) — the Philox mask of dir_dropout_mask against the numpy restatement bit for bit, dir_tail_dropout_fwd /
dir_tail_dropout_bwd against the package's own unfused chain with the mask applied by torch ops (and a float64 restatement), no
library kernel in a training step with dropout, the model's train / eval contract, reproducibility through torch's generator,
and the train.py command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import dropout_reference as R
from conftest import PKG, assert_close, records_dir

pytestmark = pytest.mark.gpu

FDS_KW = dict(bucket_num=100, bucket_start=0, start_update=0, start_smooth=1, kernel="gaussian", ks=5, sigma=2, momentum=0.9)


@pytest.fixture(autouse=True)
def _restore_global_rng():
    """These tests seed and advance torch's global generators; later test files draw their weights from them (nn.Linear)."""
    with torch.random.fork_rng(devices=[torch.cuda.current_device()]):
        yield


def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


@pytest.mark.parametrize("b,c", [(1, 64), (300, 128), (256, 2048)])
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9, 1.0])
def test_dropout_mask_equals_numpy_restatement(b, c, p):
    from dirhip.tail import dropout_mask
    for seed, offset in [(0, 0), (12345, 2 ** 32 + 12), (2 ** 40 + 3, 8), (0xfedcba9876543210, 0xffff_ffff_fffc)]:
        keep = dropout_mask(seed, offset, p, b, c, torch.device("cuda")).cpu().numpy()
        want = R.mask(seed, offset, p, b, c)
        assert np.array_equal(keep, want), (seed, offset, int((keep != want).sum()))
        n = b * c
        assert abs(keep.mean() - (1 - p)) <= 6 * np.sqrt(p * (1 - p) / n), (seed, offset, keep.mean())


def _fds(c, seed):
    from dirhip.fds import FDS
    f = FDS(c, bucket_num=30, bucket_start=3, start_update=0, start_smooth=1, kernel="gaussian", ks=5, sigma=2, momentum=0.9).cuda()
    g = torch.Generator(device="cuda").manual_seed(seed)
    lab = torch.randint(0, 34, (600,), device="cuda", generator=g).float()
    for ep in range(2):
        feats = torch.rand(600, c, device="cuda", generator=g) * 0.5 + 0.02 * lab[:, None]
        f.update_last_epoch_stats(ep)
        f.update_running_stats(feats, lab, ep)
    return f


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("with_denc", [True, False])
@pytest.mark.parametrize("b,c,p", [(64, 2048, 0.5), (300, 128, 0.2), (16, 2048, 1.0)])
def test_fused_dropout_tail_equals_unfused_chain_and_float64(dtype, smooth, with_denc, b, c, p):
    from dirhip.pool import global_avgpool_flat
    from dirhip.tail import dropout_mask, tail_forward
    g = torch.Generator(device="cuda").manual_seed(b + c)
    fds = _fds(c, 5) if smooth else None
    pool, lin = nn.AvgPool2d(7, stride=1), nn.Linear(c, 1).cuda()
    x0 = torch.relu(torch.randn(b, c, 7, 7, device="cuda", generator=g)).to(dtype).contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, 34, (b, 1), device="cuda", generator=g).float()
    dpred = torch.randn(b, 1, device="cuda", generator=g)
    denc = torch.randn(b, c, device="cuda", generator=g) * 0.01 if with_denc else None

    def loss(pred, enc):
        out = (pred * dpred).sum()
        return out + (enc * denc).sum() if with_denc else out

    # ---- fused: (seed, offset) come from the default generator, which moves on by 4
    torch.cuda.manual_seed(77)
    seed, offset = _gen().initial_seed(), _gen().get_offset()
    xf = x0.clone().requires_grad_(True)
    pred_f, enc_f = tail_forward(xf, lin, fds, labels, dropout=p)
    assert _gen().get_offset() == offset + 4 and _gen().initial_seed() == seed
    loss(pred_f, enc_f).backward()
    gw_f, gb_f = lin.weight.grad.clone(), lin.bias.grad.clone()
    lin.zero_grad()
    # ---- unfused chain of the package's kernels + the same mask by torch ops
    keep = dropout_mask(seed, offset, p, b, c, x0.device)
    scale = float(R.scale(p))
    xu = x0.clone().requires_grad_(True)
    enc_u = global_avgpool_flat(xu, pool)
    if smooth:
        enc_u = fds.smooth(enc_u, labels, 5)
    pred_u = lin(torch.where(keep, enc_u * scale, torch.zeros_like(enc_u)))
    loss(pred_u, enc_u).backward()
    assert torch.equal(enc_f, enc_u)                                           # pre-dropout encoding, same float32 operations
    assert torch.equal(xf.grad, xu.grad)
    assert_close(pred_f.detach().cpu().numpy(), pred_u.detach().cpu().numpy(), rtol=1e-5, atol_scale=1e-5, msg="pred vs unfused")
    assert_close(gw_f.cpu().numpy(), lin.weight.grad.cpu().numpy(), rtol=1e-5, atol_scale=1e-6, msg="dW vs unfused")
    assert_close(gb_f.cpu().numpy(), lin.bias.grad.cpu().numpy(), rtol=1e-5, atol_scale=1e-6, msg="db vs unfused")
    # ---- float64 restatement of dropout -> linear and its gradients on the (bit-checked) encoding
    enc64 = enc_f.detach().double().cpu()
    drop64 = torch.where(keep.cpu(), enc64 * scale, torch.zeros_like(enc64))
    w64, b64, dp64 = lin.weight.detach().double().cpu(), lin.bias.detach().double().cpu(), dpred.double().cpu()
    assert_close(pred_f.detach().cpu().numpy(), (drop64 @ w64.t() + b64).numpy(), rtol=1e-5, atol_scale=1e-5, msg="pred vs float64")
    assert_close(gw_f.cpu().numpy(), (dp64.t() @ drop64).numpy(), rtol=1e-5, atol_scale=1e-5, msg="dW vs float64")
    assert_close(gb_f.cpu().numpy(), dp64.sum(0).numpy(), rtol=1e-5, atol_scale=1e-5, msg="db vs float64")
    if p == 1.0:
        assert torch.equal(pred_f.detach(), lin.bias.detach().expand(b, 1)) and not gw_f.any()


def _model(dropout, amp_dtype=torch.bfloat16, seed=0):
    from dirhip.parallel import DataParallelEngine
    from dirhip.resnet import resnet50
    torch.manual_seed(seed)
    model = resnet50(fds=True, dropout=dropout, **FDS_KW).cuda()
    g = torch.Generator(device="cuda").manual_seed(9)                           # live FDS statistics: calibration changes the encoding
    lab = torch.randint(0, 100, (512,), device="cuda", generator=g).float()
    for ep in range(2):
        model.FDS.update_last_epoch_stats(ep)
        model.FDS.update_running_stats(torch.rand(512, 2048, device="cuda", generator=g) + 0.01 * lab[:, None], lab, ep)
    model.FDS.update_last_epoch_stats(2)
    eng = DataParallelEngine(model, amp_dtype=amp_dtype, channels_last=True)
    eng.train()
    return model, eng


def _batch():
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(8, 3, 224, 224, device="cuda", generator=g)
    y = torch.tensor([[25.0], [31.0], [64.0], [25.0], [3.0], [99.0], [47.0], [12.0]], device="cuda")
    return x, y


def test_training_step_with_dropout_has_no_library_kernels():
    """resnet50(dropout=0.5): the tail stays on the fused kernels (their dropout variants) — no rocBLAS gemv / GEMM, no MIOpen,
    no torch dropout or bernoulli kernel in a bf16 training step with the FDS calibration live."""
    from torch.profiler import ProfilerActivity, profile
    from dirhip.train_loop import resolve_loss, train_step
    model, eng = _model(0.5)
    opt = torch.optim.SGD(eng.parameters(), lr=1e-4)
    x, y = _batch()
    w = torch.ones(8, 1, device="cuda")
    train_step(eng, opt, x, y, w, 2, resolve_loss("l1"))
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        train_step(eng, opt, x, y, w, 2, resolve_loss("l1"))
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad = [n for n in names if n.startswith("Cijk_") or "gemv" in n.lower() or "miopen" in n.lower() or "bernoulli" in n.lower()
           or ("dropout" in n.lower() and "DirDropout" not in n)]
    assert not bad, bad
    for k in ("tail_fwd_kernel", "tail_bwd_dx_kernel", "tail_bwd_dw_partial_kernel"):
        assert any(k in n and "DirDropout" in n for n in names), (k, names)


def test_dropout_changes_pred_not_encoding_and_nothing_in_eval():
    """Same weights, FDS statistics and batch, smoothing live (epoch 2): dropout=0.5 returns the same encoding as dropout=None
    (the calibrated, pre-dropout tensor, A.2) but another prediction; in eval mode dropout is the identity."""
    m0, e0 = _model(None)
    m1, e1 = _model(0.5)
    assert all(torch.equal(a, b) for a, b in zip(m0.state_dict().values(), m1.state_dict().values()))   # (dropout draws no weights)
    x, y = _batch()
    with torch.no_grad():
        p0, enc0 = e0(x, y, 2)
        p1, enc1 = e1(x, y, 2)
    assert torch.equal(enc0, enc1) and not torch.equal(p0, p1)
    e0.eval(); e1.eval()
    with torch.no_grad():
        q0, q1 = e0(x, y, 2), e1(x, y, 2)
    assert torch.equal(q0, q1)


@pytest.mark.parametrize("amp_dtype", [None, torch.bfloat16])
def test_dropout_reproducible_through_torch_generator(amp_dtype):
    from dirhip.train_loop import resolve_loss
    loss_fn = resolve_loss("l1")
    x, y = _batch()
    w = torch.ones(8, 1, device="cuda")

    def step(seed):
        model, eng = _model(0.5, amp_dtype)
        torch.manual_seed(seed)
        pred, _ = eng(x, y, 2)
        loss = loss_fn(pred, y, w)
        loss.backward()
        return loss.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    # the same torch.manual_seed: identical loss and gradients after one step
    l1, g1 = step(3)
    l2, g2 = step(3)
    assert torch.equal(l1, l2) and g1.keys() == g2.keys() and all(torch.equal(g1[k], g2[k]) for k in g1)
    assert "linear.weight" in g1 and "conv1.weight" in g1
    model, eng = _model(0.5, amp_dtype)
    torch.manual_seed(4)
    with torch.no_grad():
        state = torch.cuda.get_rng_state()
        pa, ea = eng(x, y, 2)
        pb, eb = eng(x, y, 2)                           # consecutive forwards: a fresh mask (the encoding is the same)
        assert torch.equal(ea, eb) and not torch.equal(pa, pb)
        torch.cuda.set_rng_state(state)
        pc, _ = eng(x, y, 2)                            # restoring the generator replays the first mask
        assert torch.equal(pa, pc)
    torch.cuda.set_rng_state(state)
    pd, ed = eng(x, y, 2)                               # a grad forward from the same state: the no_grad forward's result
    assert torch.equal(pa, pd.detach()) and torch.equal(ea, ed.detach())


def test_train_py_cli_dropout(tmp_path):
    """python train.py --synthetic 1024 --fds --dropout 0.5 --epoch 2, then --evaluate on its checkpoint (drop-in folder)."""
    script = os.path.join(PKG, "imdb-wiki-dir", "train.py")
    base = ["--synthetic", "1024", "--fds", "--dropout", "0.5", "--batch_size", "64", "--store_root", str(tmp_path), "--print_freq", "8"]

    def cli(args, log):
        p = subprocess.run([sys.executable, script] + args, cwd=os.path.dirname(script), capture_output=True, text=True, timeout=900,
                           stdin=subprocess.DEVNULL)
        out = p.stdout + p.stderr
        with open(os.path.join(records_dir(), log), "w") as f:
            f.write(" ".join(args) + "\n" + out)
        assert p.returncode == 0, out[-3000:]
        return out

    out = cli(base + ["--epoch", "2"], "cli_dropout_train.log")
    assert "Using dropout: 0.5" in out and "Epoch #1: Train loss" in out and "Test loss: MSE" in out, out[-2000:]
    store = tmp_path / "imdb_wiki_resnet50_fds_gau_5_1_0_1_0.9_dropout_0.5_adam_l1_0.001_64"
    assert (store / "ckpt.best.pth.tar").is_file(), os.listdir(tmp_path)
    out = cli(base + ["--evaluate", "--resume", str(store / "ckpt.best.pth.tar")], "cli_dropout_evaluate.log")
    assert "Using dropout: 0.5" in out and "Test: " in out and " * Overall: MSE" in out, out[-2000:]
