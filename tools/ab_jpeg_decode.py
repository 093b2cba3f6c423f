"""JPEG decode split (host entropy stage + HIP reconstruction) against Pillow's full decode, on Pillow-written files of 320^2-like sizes.

    python tools/ab_jpeg_decode.py [--n 256 --reps 5 --threads 8 --workers 8 --out F]

Host half (runs anywhere, one core): per image
  (a) dir_jpeg_inspect + dir_jpeg_entropy_decode (markers + Huffman -> int16 coefficients)
  (b) Pillow ``Image.open(BytesIO(f)).convert('RGB')`` (libjpeg-turbo's whole decode)
and the same with ``--threads`` threads in one process (the ctypes call and Pillow's decoder both release the GIL).
GPU half (only when a GPU is present; otherwise the output says "not measured"):
  (c) dir_jpeg_reconstruct alone on a device-resident staged batch (HIP events)
  (d) files -> DataLoader(raw="bytes", bytes_collate) -> DeviceJpeg -> DeviceResize(224)                       (--gpu_decode)
  (e) files -> DataLoader(raw="decoded", ragged_collate) -> DeviceResize(224)                                  (--gpu_resize)
  (f) files -> DataLoader(raw=True: Pillow decode + resize in the workers) -> copy of the uint8 batch           (--gpu_augment)
each of (d) - (f) timed over whole passes of the set with ``--workers`` loader workers, after a warm-up pass, ending with the resized
uint8 batch on the device. Medians over ``--reps``. The images: sums of sinusoids plus noise, quality 85, 4:2:0 (what photographs
mostly are), W and H uniform on [256, 384]."""
import argparse
import io
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "imbalanced-regression_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from dirhip import jpeg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--threads", type=int, default=8)
ap.add_argument("--workers", type=int, default=8)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--out", default=None)
a = ap.parse_args()

rng = np.random.default_rng(0)
files = []
for k in range(a.n):
    h, w = int(rng.integers(256, 385)), int(rng.integers(256, 385))
    yy, xx = np.mgrid[0:h, 0:w]
    arr = np.stack([128 + 60 * np.sin(xx / (11 + 3 * c) + k) * np.cos(yy / (17 - 2 * c)) + 40 * np.sin((xx + yy) / (41 + c)) for c in range(3)], -1)
    buf = io.BytesIO()
    Image.fromarray(np.clip(arr + rng.normal(0, 6, arr.shape), 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=85, subsampling=2)
    files.append(buf.getvalue())
pixels = sum(int(np.prod(Image.open(io.BytesIO(f)).size)) for f in files)
lines = [f"ab_jpeg_decode: {a.n} files, {sum(map(len, files)) / a.n / 1024:.1f} KiB and {pixels / a.n / 1e3:.0f} kpixel per file on average, quality 85, 4:2:0",
         f"host: {os.cpu_count()} CPUs visible, torch threads {torch.get_num_threads()}; GPU: {torch.cuda.get_device_name(0) if torch.cuda.is_available() else 'none'}"]


def native_one(f):
    rc, info = jpeg.inspect(f)
    assert rc == 0, rc
    out = np.empty(info.ncoef, dtype=np.int16)
    assert jpeg.entropy_decode(f, info, out) == 0
    return out


def pillow_one(f):
    return Image.open(io.BytesIO(f)).convert("RGB")


def per_image(fn, pool=None):
    ts = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        if pool is None:
            for f in files:
                fn(f)
        else:
            list(pool.map(fn, files))
        ts.append((time.perf_counter() - t0) / len(files))
    return statistics.median(ts[1:])


t_nat, t_pil = per_image(native_one), per_image(pillow_one)
lines.append(f"(a) host entropy stage, one core : {t_nat * 1e6:8.1f} us/image = {1 / t_nat:8.0f} images/s/core")
lines.append(f"(b) Pillow full decode, one core : {t_pil * 1e6:8.1f} us/image = {1 / t_pil:8.0f} images/s/core   (a) / (b) = {t_nat / t_pil:.2f}")
with ThreadPoolExecutor(a.threads) as pool:
    tt_nat, tt_pil = per_image(native_one, pool), per_image(pillow_one, pool)
lines.append(f"(a) with {a.threads} threads, one process: {1 / tt_nat:8.0f} images/s;  (b) with {a.threads} threads: {1 / tt_pil:8.0f} images/s")

if not torch.cuda.is_available():
    lines.append("GPU half (c) - (f): not measured (no GPU on this machine)")
else:
    import pandas as pd
    from torch.utils.data import DataLoader
    from dirhip.datasets import AgeDB, DeviceResize, bytes_collate, ragged_collate, split_files
    dev = torch.device("cuda:0")
    dj = jpeg.DeviceJpeg(dev, threads=a.threads)
    # (c) the reconstruct call alone
    plan = dj.host_stage(files[:a.batch])
    stage_d = plan["stage"].to(dev)
    flat = torch.empty(plan["flat_bytes"], dtype=torch.uint8, device=dev)
    ts = []
    for _ in range(a.reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dj.reconstruct(plan, stage_d, flat)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    t = statistics.median(ts[2:])
    nb = min(a.batch, a.n)
    lines.append(f"(c) dir_jpeg_reconstruct, {nb} images: {t * 1e3:.3f} ms = {nb / t:.0f} images/s, "
                 f"{(3 * plan['ncoef'] + 2 * plan['flat_bytes']) / t / 1e9:.0f} GB/s of coefficient + plane + pixel traffic")
    with tempfile.TemporaryDirectory() as d:
        for k, f in enumerate(files):
            with open(os.path.join(d, f"{k}.jpg"), "wb") as fh:
                fh.write(f)
        df = pd.DataFrame([{"path": f"{k}.jpg", "age": 30.0, "split": "train"} for k in range(a.n)])
        resize = DeviceResize(224, dev)
        kw = dict(batch_size=a.batch, num_workers=a.workers, persistent_workers=a.workers > 0)

        def arm_bytes(b):
            return resize(*dj.decode(split_files(b[0], b[1])))

        def arm_decoded(b):
            return resize(b[0], b[1])

        def arm_resized(b):
            return b[0].to(dev, non_blocking=True)
        arms = [("(d) bytes -> DeviceJpeg -> DeviceResize", AgeDB(df, d, 224, "val", raw="bytes"), bytes_collate, arm_bytes),
                ("(e) decoded in workers -> DeviceResize  ", AgeDB(df, d, 224, "val", raw="decoded"), ragged_collate, arm_decoded),
                ("(f) decoded + resized in workers        ", AgeDB(df, d, 224, "val", raw=True), None, arm_resized)]
        for name, ds, collate, fn in arms:
            loader = DataLoader(ds, collate_fn=collate, **kw)
            ts = []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                for b in loader:
                    out = fn(b)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            t = statistics.median(ts[1:])
            lines.append(f"{name}: {a.n / t:8.0f} images/s ({a.workers} workers, {a.threads} decode threads, batch {a.batch})")
            del loader
    lines.append(f"DeviceJpeg counters: taken {dj.taken}, fallback {dj.fallback}, failed {dj.failed}")

text = "\n".join(lines)
print(text)
if a.out:
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
