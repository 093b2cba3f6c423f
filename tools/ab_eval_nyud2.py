"""NYUD2-DIR test-set evaluation, fused evaluator against the reference's sequence on the same GPU (profiles/nyud2_eval.txt).

    python tools/ab_eval_nyud2.py [--images 654 --batch 8 --reps 5 --ref-reps 2 --out F]

Synthetic test set: ``--images`` x (114 x 152 prediction, 480 x 640 depth, mask), resident on the device before timing starts.
  (a) fused      Evaluator.update(pred, depth, mask) per batch, then evaluate_shot()  (one read-back of 800 numbers)
  (b) reference  the sequence of nyud2-dir/test.py:52-54 and util.py restated with torch ops: per batch F.interpolate(bilinear,
                 align_corners=True), output[mask] / depth[mask], .cpu(), torch.cat on the host; then the bucket index as a torch
                 expression (kinder than the reference's per-pixel Python map) and the nine metrics as torch reductions over the
                 host vectors, once overall and once per shot group.
The arms alternate; wall seconds per test set, all repetitions listed. The kernel's own time is taken with device events around
the update calls of (a); its achieved bytes/s (4 B depth + 1 B mask per target pixel + the low-resolution predictions) is set against
a device-to-device copy of 1 GiB measured in the same process (read + write bytes counted)."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "imbalanced-regression_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dirhip.eval_nyud2 import Evaluator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=654)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ref-reps", type=int, default=2)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
h, w, H, W = 114, 152, 480, 640

torch.manual_seed(0)
yy = torch.linspace(0, 1, H, device=dev)[:, None]
xx = torch.linspace(0, 1, W, device=dev)[None, :]
expo = 1.0 + 0.5 * torch.rand(a.images, 1, 1, 1, device=dev)
depth = (0.4 + 9.8 * (0.55 * xx + 0.45 * yy)[None, None] ** expo + 0.03 * torch.randn(a.images, 1, H, W, device=dev)).clamp_(0.3, 11.0)
pred = F.interpolate(depth, size=(h, w), mode="bilinear", align_corners=True) * (0.75 + 0.6 * torch.rand(a.images, 1, h, w, device=dev))
mask = torch.rand(a.images, 1, H, W, device=dev) < 0.85
torch.cuda.synchronize()


def fused():
    ev = Evaluator()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for i in range(0, a.images, a.batch):
        ev.update(pred[i:i + a.batch], depth[i:i + a.batch], mask[i:i + a.batch])
    e1.record()
    d = ev.evaluate_shot()
    wall = time.perf_counter() - t0
    return wall, e0.elapsed_time(e1) * 1e-3, d


def metrics(o, z):
    n = float(z.numel())
    if n == 0:
        return {"NUM": 0}
    d = (o - z).abs()
    r = torch.maximum(o / z, z / o)
    lg = (torch.log(o) / math.log(10) - torch.log(z) / math.log(10)).abs()
    mse = float(d.pow(2).sum() / n)
    return {"MSE": mse, "RMSE": math.sqrt(mse), "ABS_REL": float((d / z).sum() / n), "LG10": float(lg.sum() / n), "MAE": float(d.sum() / n),
            "DELTA1": float((r <= 1.25).float().sum() / n), "DELTA2": float((r <= 1.25 ** 2).float().sum() / n),
            "DELTA3": float((r <= 1.25 ** 3).float().sum() / n), "NUM": int(n)}


def reference():
    shots = Evaluator().shot_idx
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs, deps = [], []
    for i in range(0, a.images, a.batch):
        m = mask[i:i + a.batch]
        up = F.interpolate(pred[i:i + a.batch], size=(H, W), mode="bilinear", align_corners=True)
        outs.append(up[m].cpu())
        deps.append(depth[i:i + a.batch][m].cpu())
    o, z = torch.cat(outs), torch.cat(deps)
    t1 = time.perf_counter()
    bucket = (z * 10).to(torch.int64).clamp_(max=99)
    d = {"overall": metrics(o, z)}
    for s, idx in shots.items():
        sel = torch.isin(bucket, torch.tensor(idx))
        d[s] = metrics(o[sel], z[sel])
    t2 = time.perf_counter()
    return t2 - t0, t1 - t0, d


def copy_rate():
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    return 2 * 10 * (1 << 30) / (e0.elapsed_time(e1) * 1e-3)


fused(); fused()                                                  # warm-up: library load, workspace, allocator
rows = {"fused_wall_s": [], "fused_kernels_s": [], "reference_wall_s": [], "reference_until_host_vectors_s": []}
dict_a = dict_b = None
for r in range(max(a.reps, a.ref_reps)):
    if r < a.reps:
        wall, kern, dict_a = fused()
        rows["fused_wall_s"].append(round(wall, 6)); rows["fused_kernels_s"].append(round(kern, 6))
    if r < a.ref_reps:
        wall, part, dict_b = reference()
        rows["reference_wall_s"].append(round(wall, 3)); rows["reference_until_host_vectors_s"].append(round(part, 3))
med = lambda v: sorted(v)[len(v) // 2]
nbytes = a.images * (H * W * 5 + h * w * 4)
rate, box = nbytes / med(rows["fused_kernels_s"]), copy_rate()
agree = max(abs(dict_a[s][k] - dict_b[s][k]) / max(abs(dict_b[s][k]), 1e-30) for s in dict_b for k in dict_b[s])
out = {"images": a.images, "batch": a.batch, "pixels_kept": dict_a["overall"]["NUM"], **rows,
       "fused_median_s": med(rows["fused_wall_s"]), "reference_median_s": med(rows["reference_wall_s"]),
       "speedup": med(rows["reference_wall_s"]) / med(rows["fused_wall_s"]),
       "kernel_bytes": nbytes, "kernel_bytes_per_s": rate, "device_copy_bytes_per_s": box, "fraction_of_copy_rate": rate / box,
       "max_relative_difference_of_the_two_dicts": agree, "fused_overall": dict_a["overall"]}
text = json.dumps(out, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
