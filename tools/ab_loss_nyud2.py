"""NYUD2-DIR training loss, forward + backward: the fused call against the composition it replaces, same GPU, same process
(``--out profiles/nyud2_loss.txt``).

    python tools/ab_loss_nyud2.py [--batch 32 --steps 200 --reps 11 --out F]

Inputs: ``--batch`` maps of 114 x 152 (prediction and depth, float32, resident on the device), LDS bucket weights ('inverse').
  (a) fused        PixelWeights.loss(output, depth)  +  torch.autograd.grad            (dir_depth_loss: one streaming launch + its fold;
                   backward = one scale kernel)
  (b) composition  w = PixelWeights.weights(depth); torch.mean(((output - depth) ** 2) * w)  +  torch.autograd.grad
A repetition is ``--steps`` steps between two device events (and a host clock around them, ending in a synchronise); the arms alternate,
medians over ``--reps`` repetitions after a warm-up repetition of each. Launches per step are counted in a separate profiled step."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "imbalanced-regression_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

from dirhip.lds_nyud2 import PixelWeights, get_bucket_weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("ab_loss_nyud2.py measures on the GPU; none found")
dev = torch.device("cuda:0")
H, W = 114, 152

torch.manual_seed(0)
depth = (0.7 + 9.3 * torch.rand(a.batch, 1, H, W, device=dev)).contiguous()
output = (depth * (0.75 + 0.6 * torch.rand_like(depth))).requires_grad_(True)
pw = PixelWeights(get_bucket_weights("inverse", lds=True))


def fused():
    loss = pw.loss(output, depth)
    (g,) = torch.autograd.grad(loss, output)
    return loss, g


def composition():
    w = pw.weights(depth)
    loss = torch.mean(((output - depth) ** 2) * w)
    (g,) = torch.autograd.grad(loss, output)
    return loss, g


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(a.steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return e0.elapsed_time(e1) * 1e-3 / a.steps, wall / a.steps


def launches(fn):
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name.split("(")[0][:90] for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


arms = {"fused": fused, "composition": composition}
for fn in arms.values():                                      # warm-up: library load, table upload, workspace, allocator
    timed(fn)
rows = {k: {"device_s": [], "wall_s": []} for k in arms}
for _ in range(a.reps):
    for k, fn in arms.items():
        d, w = timed(fn)
        rows[k]["device_s"].append(d); rows[k]["wall_s"].append(w)
med = lambda v: sorted(v)[len(v) // 2]
(la, ga), (lb, gb) = fused(), composition()
kern = {k: launches(fn) for k, fn in arms.items()}
n = depth.numel()
out = {"batch": a.batch, "pixels": n, "steps_per_repetition": a.steps, "repetitions": a.reps,
       "launches_per_step": {k: len(v) for k, v in kern.items()}, "kernels": kern,
       "median_device_us_per_step": {k: round(med(r["device_s"]) * 1e6, 2) for k, r in rows.items()},
       "median_wall_us_per_step": {k: round(med(r["wall_s"]) * 1e6, 2) for k, r in rows.items()},
       "device_us_per_step_all": {k: [round(x * 1e6, 2) for x in r["device_s"]] for k, r in rows.items()},
       "composition_over_fused_device": med(rows["composition"]["device_s"]) / med(rows["fused"]["device_s"]),
       "composition_over_fused_wall": med(rows["composition"]["wall_s"]) / med(rows["fused"]["wall_s"]),
       "bytes_fused_needs": n * 12, "loss_fused": la.item(), "loss_composition": lb.item(),
       "gradient_elements_that_differ": int((ga != gb).sum().item()),
       "weight_map_bytes_not_written": n * 4,
       "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
assert np.isfinite(out["loss_fused"])
text = json.dumps(out, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
