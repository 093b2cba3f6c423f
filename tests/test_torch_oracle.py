"""Pins oracle/torch_oracle.py (the CPU 'port' used as bench.py's cpu_baseline and as the differentiable
checker of the end-to-end GPU tests) against the reference: same init stream, same loss trajectory,
same FDS buffers on identical inputs. The reference's side is tests/golden/port_training_ref.npz, recorded
from the live reference by tests/golden/gen_golden_pins.py (which also runs this comparison live).

Both sides run in a child process with the host's CPU arithmetic pinned (PINNED_ENV, no oneDNN, exact_sqrt): Adam
turns gradients that are pure rounding noise into full-size updates and the FDS calibration divides by variances of
one to three samples, so a trajectory recorded with one CPU's vectorised / BLAS kernels is not reproducible with
another's (1e-4 after two epochs), while the pinned kernels give the same bits on every x86-64 host."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FDS_KW = dict(bucket_num=100, bucket_start=0, start_update=0, start_smooth=1, kernel="gaussian", ks=5, sigma=2, momentum=0.9)
# scalar ATen kernels, one thread, MKL's conditional-numerical-reproducibility branch that every x86-64 CPU takes
PINNED_ENV = {"ATEN_CPU_CAPABILITY": "default", "OMP_NUM_THREADS": "1", "MKL_NUM_THREADS": "1", "MKL_CBWR": "COMPATIBLE"}
SAMPLE = 64          # initial values kept per tensor (fixed positions: seed 0 per tensor size)


def exact_sqrt():
    """float32 sqrt as the correctly rounded float64 sqrt (exact for sqrt): MKL's float32 vector sqrt, which torch.sqrt uses,
    rounds differently on different CPUs in every MKL_CBWR branch. Both sides of a pin run with it (torch.sqrt for the FDS
    calibration, Tensor.sqrt / _foreach_sqrt for Adam)."""
    f_sqrt = torch.sqrt

    def sq(t):
        return f_sqrt(t.double()).to(t.dtype) if t.dtype == torch.float32 else f_sqrt(t)

    def foreach_sqrt_(ts):
        for t in ts:
            t.copy_(sq(t))
    torch.sqrt = sq
    torch.Tensor.sqrt = sq
    torch._foreach_sqrt = lambda ts: [sq(t) for t in ts]
    torch._foreach_sqrt_ = foreach_sqrt_


def sample_positions(numel):
    return np.sort(np.random.default_rng(0).choice(numel, size=min(SAMPLE, numel), replace=False))


def batches():
    g = torch.Generator().manual_seed(0)
    return [(torch.randn(3, 3, 224, 224, generator=g), torch.tensor([[25.0], [40.0], [25.0 + i]]),
             torch.rand(3, 1, generator=g) + 0.5) for i in range(2)]


def init_record(model):
    """State-dict keys and shapes, a float64 checksum and a fixed sample of every initial tensor."""
    out = {"init_keys": np.array(json.dumps([[k, list(v.shape)] for k, v in model.state_dict().items()]))}
    for k, v in model.state_dict().items():
        a = v.detach().reshape(-1).double().numpy()
        out[f"init_sum_{k}"] = np.array(a.sum())
        out[f"init_{k}"] = v.detach().reshape(-1)[torch.as_tensor(sample_positions(v.numel()))].numpy().copy()
    return out


def port_run():
    """The port through the reference's loop (train.py:246-281): six steps over three epochs, an epoch tail after each epoch."""
    from oracle import torch_oracle
    torch.manual_seed(7)
    port = torch_oracle.RefResNet50(fds=True, **FDS_KW)
    out = init_record(port)
    opt = torch.optim.Adam(port.parameters(), lr=1e-3)
    bs = batches()
    losses = []
    for epoch in range(3):
        for x, y, w in bs:
            losses.append(torch_oracle.train_step(port, opt, x, y, w, epoch, "l1"))
        torch_oracle.epoch_tail(port, [(x, y) for x, y, _ in bs], epoch)
        for k, v in port.FDS.state_dict().items():
            out[f"e{epoch}_fds_{k}"] = v.numpy().copy()
    out["losses"] = np.array(losses, np.float64)
    return out


def run_pinned(what, out_path):
    """`what` (port_run here, the reference's run in gen_golden_pins.py) in a child process with PINNED_ENV, result -> out_path (.npz)."""
    env = dict(os.environ, **PINNED_ENV)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, HERE, os.path.join(ROOT, "tests", "golden")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    code = (f"import sys, numpy as np, torch; torch.backends.mkldnn.enabled = False; torch.set_num_threads(1); "
            f"import test_torch_oracle; test_torch_oracle.exact_sqrt(); "
            f"import {what.rsplit('.', 1)[0]} as m; np.savez(sys.argv[1], **m.{what.rsplit('.', 1)[1]}())")
    p = subprocess.run([sys.executable, "-c", code, out_path], env=env, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return np.load(out_path)


def test_port_matches_live_reference_training(golden, tmp_path):
    ref = golden("port_training_ref.npz")
    got = run_pinned("test_torch_oracle.port_run", str(tmp_path / "port.npz"))
    assert json.loads(str(got["init_keys"])) == json.loads(str(ref["init_keys"]))
    for k, _ in json.loads(str(ref["init_keys"])):
        assert np.array_equal(got[f"init_{k}"], ref[f"init_{k}"]), k
        assert float(got[f"init_sum_{k}"]) == float(ref[f"init_sum_{k}"]), k
    for i, (lp, lr) in enumerate(zip(got["losses"], ref["losses"])):
        assert abs(lp - lr) <= 1e-6 * abs(lr), (i, lp, lr)
    assert len(got["losses"]) == len(ref["losses"]) == 6
    for epoch in range(3):
        keys = [k for k in ref.files if k.startswith(f"e{epoch}_fds_")]
        assert keys and sorted(keys) == sorted(k for k in got.files if k.startswith(f"e{epoch}_fds_"))
        for k in keys:
            assert torch.allclose(torch.from_numpy(ref[k]), torch.from_numpy(got[k]), rtol=1e-6, atol=1e-7), k
