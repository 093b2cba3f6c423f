"""Wall time of ``train_main.validate`` on a synthetic validation set, default path against ``--device_eval``, same process, same GPU
(profiles/age_eval_validate.txt).

    python tools/time_age_validate.py [--val 11000 --train 191509 --batch 256 --reps 3 --out F]

The model and the batches are those ``train.py --synthetic`` builds (ResNet-50 in bf16 under ``DataParallelEngine``, channels-last
random images generated on the device, labels of the same clipped half-normal); only the size of the validation set differs from the
command line's fixed 1000. Per call two host clocks: the whole call, and from the return of the last forward to the return of the
function (the forwards are enqueued asynchronously, so this span also holds the wait for the GPU to finish them: it is what the
host still has to sit through once the loop is over). The arms alternate after one warm-up call each."""
import argparse
import json
import logging
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "imbalanced-regression_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dirhip import datasets  # noqa: E402
from dirhip.parallel import DataParallelEngine  # noqa: E402
from dirhip.resnet import resnet50  # noqa: E402
from dirhip.train_main import validate  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--val", type=int, default=11000)
ap.add_argument("--train", type=int, default=191509)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
logging.basicConfig(level=logging.WARNING)
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)

rng = np.random.default_rng(0)
pool = np.clip(np.round(np.abs(rng.normal(0, 18, a.train + a.val)) + 20), 0, 120).astype(np.float32)
train_labels, val_set = pool[:a.train], datasets.SyntheticAgeDataset(pool[a.train:], 224, seed=2)
torch.manual_seed(0)
net = resnet50(fds=False, bucket_num=100, bucket_start=0, start_update=0, start_smooth=1, kernel="gaussian", ks=5, sigma=1, momentum=0.9)
model = DataParallelEngine(net.to(dev), amp_dtype=torch.bfloat16, channels_last=True, f32_arith="exact")
n_val = (len(val_set) + a.batch - 1) // a.batch
last_forward = [0.0]


class Stamped(torch.nn.Module):
    """The model, with the host time of every forward's return."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        y = self.inner(x)
        last_forward[0] = time.perf_counter()
        return y


stamped = Stamped(model)


def batches():
    return val_set.device_batches(torch.arange(len(val_set)), a.batch, dev)


def one(device_eval):
    args = types.SimpleNamespace(print_freq=10, device_eval=device_eval)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = validate(batches, n_val, stamped, args, train_labels=train_labels)
    t1 = time.perf_counter()
    return {"whole_call_s": t1 - t0, "after_last_forward_s": t1 - last_forward[0], "result": [float(x) for x in out]}


for flag in (False, True):
    one(flag)
runs = {"default": [], "device_eval": []}
for _ in range(a.reps):
    runs["default"].append(one(False))
    runs["device_eval"].append(one(True))
res = {"val_samples": len(val_set), "train_labels": int(a.train), "batch": a.batch, "reps": a.reps, "gpus_visible": torch.cuda.device_count(), **runs}
text = json.dumps(res, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
