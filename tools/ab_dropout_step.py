"""B=256 bf16 training steps of the bench workload (ResNet-50 + FDS live + LDS weights, Adam) with and without dropout 0.5
(profiles/dropout_tail_step.txt).

    python tools/ab_dropout_step.py --mode ab [--steps K --blocks N --out F] one model, blocks of K steps alternating the two arms
                                                                      (same weights), wall ms per step of every block
    rocprofv3 --kernel-trace --stats -d OUT -o drop --output-format csv -- python tools/ab_dropout_step.py --mode drop --steps 20
                                                                      per-kernel device times of one arm (--mode nodrop: the other)
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (puts the package on sys.path)
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="ab", choices=["ab", "nodrop", "drop"])
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--blocks", type=int, default=6)
ap.add_argument("--out", default=None, help="--mode ab: also write the result as JSON to this file")
a = ap.parse_args()

from dirhip.train_loop import resolve_loss, train_step  # noqa: E402

dev = torch.device("cuda:0")
model, engine, opt, batches = bench.build(types.SimpleNamespace(batch=256, epoch_len=4), dev, 0)
model.dropout = nn.Dropout(0.5)                              # = resnet50(dropout=0.5): no weights, same initialisation stream
loss_fn = resolve_loss("l1")


def run(drop, k):
    model.use_dropout = drop
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(k):
        loss = train_step(engine, opt, *batches[s % len(batches)], 2, loss_fn)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3, float(loss)


if a.mode != "ab":
    run(a.mode == "drop", 3)
    ms, loss = run(a.mode == "drop", a.steps)
    print(json.dumps({"mode": a.mode, "ms_per_step": ms, "loss": loss}))
else:
    run(False, 3); run(True, 3)
    rows = {"nodrop": [], "drop": []}
    for i in range(a.blocks):
        for drop in ((False, True) if i % 2 == 0 else (True, False)):
            ms, loss = run(drop, a.steps)
            rows["drop" if drop else "nodrop"].append(round(ms, 3))
    out = {k: {"ms_per_step": v, "median": sorted(v)[len(v) // 2]} for k, v in rows.items()}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
