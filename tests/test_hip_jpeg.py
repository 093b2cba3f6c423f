"""-m gpu: JPEG decode with the GPU doing the data-parallel half (dirhip.jpeg.DeviceJpeg: host entropy decode + dir_jpeg_reconstruct)
against Pillow, bit for bit, on the fixtures of tests/jpeg_fixtures.py — singly, as one ragged batch, mixed with files the native
decoder leaves to Pillow — then through DeviceResize against the raw="decoded" path, and through the train.py command line.
The arithmetic itself is pinned without a GPU in tests/test_jpeg_host.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
import jpeg_fixtures as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def taken():
    files = F.taken_fixtures() + F.narrow_fixtures()
    return [(name, data, F.pillow_rgb(data)) for name, data in files]          # Pillow's decode: computed once, shared, never modified


def test_every_fixture_singly_and_all_as_one_shuffled_batch(taken):
    from dirhip.jpeg import DeviceJpeg
    dj = DeviceJpeg(threads=4)
    for name, data, want in taken:
        flat, sizes = dj.decode([data])                                          # B = 1
        assert sizes.tolist() == [list(want.shape[:2])], name
        got = flat.cpu().numpy()
        assert got.size == want.size and np.array_equal(got.reshape(want.shape), want), (name, int((got.reshape(want.shape) != want).sum()))
    assert (dj.taken, dj.fallback, dj.failed) == (len(taken), 0, 0)              # nothing routed to Pillow
    order = np.random.default_rng(3).permutation(len(taken))
    dj = DeviceJpeg(threads=4)
    flat, sizes = dj.decode([taken[i][1] for i in order])
    want = np.concatenate([taken[i][2].reshape(-1) for i in order])
    assert sizes.tolist() == [list(taken[i][2].shape[:2]) for i in order]
    assert flat.dtype == torch.uint8 and flat.is_cuda and np.array_equal(flat.cpu().numpy(), want)
    assert (dj.taken, dj.fallback, dj.failed) == (len(taken), 0, 0)
    again, _ = dj.decode([taken[i][1] for i in order])                           # the same batch twice: identical bytes
    assert torch.equal(again, flat)


def test_mixed_batch_falls_back_per_file_and_garbage_raises_before_any_launch(taken):
    from dirhip import _lib
    from dirhip.jpeg import DeviceJpeg
    other = dict(F.not_taken_fixtures())
    by_name = {name: (data, want) for name, data, want in taken}
    files = [by_name["colour_17x23_s2_noise"][0], other["progressive"], by_name["gray_9x31_smooth"][0], other["cmyk"], by_name["larger_noise"][0]]
    dj = DeviceJpeg(threads=2)
    flat, sizes = dj.decode(files)
    got, at = flat.cpu().numpy(), 0
    for k, f in enumerate(files):
        want = F.pillow_rgb(f)
        assert sizes[k].tolist() == list(want.shape[:2])
        assert np.array_equal(got[at:at + want.size].reshape(want.shape), want), k
        at += want.size
    assert at == got.size and (dj.taken, dj.fallback, dj.failed) == (3, 2, 0)
    garbage = bytes(np.random.default_rng(4).integers(0, 256, 300, dtype=np.uint8))
    with pytest.raises(_lib.DirHipError, match=r"file 5 of the batch"):
        dj.decode(files + [garbage])
    assert (dj.taken, dj.fallback, dj.failed) == (3, 2, 1)                      # raised before the batch was counted or launched
    torch.cuda.synchronize()


def test_device_jpeg_plus_resize_equals_decoded_path(tmp_path, taken):
    """Files on disk -> raw="bytes" + bytes_collate -> DeviceJpeg -> DeviceResize(64) == raw="decoded" + ragged_collate -> DeviceResize(64)."""
    import pandas as pd
    from torch.utils.data import DataLoader
    from dirhip.datasets import AgeDB, DeviceResize, bytes_collate, ragged_collate, split_files
    from dirhip.jpeg import DeviceJpeg
    rows = []
    for k, (name, data, _) in enumerate(taken):
        (tmp_path / f"{name}.jpg").write_bytes(data)
        rows.append({"path": f"{name}.jpg", "age": float(20 + k), "split": "train"})
    df = pd.DataFrame(rows)
    n = len(rows)
    blob, lengths, lab, wts = next(iter(DataLoader(AgeDB(df, str(tmp_path), img_size=64, split="val", raw="bytes"), batch_size=n, collate_fn=bytes_collate)))
    flat2, sizes2, lab2, wts2 = next(iter(DataLoader(AgeDB(df, str(tmp_path), img_size=64, split="val", raw="decoded"), batch_size=n, collate_fn=ragged_collate)))
    assert lengths.tolist() == [len(d) for _, d, _ in taken] and torch.equal(lab, lab2) and torch.equal(wts, wts2)
    dj = DeviceJpeg(threads=4)
    flat, sizes = dj.decode(split_files(blob, lengths))
    assert torch.equal(sizes, sizes2) and torch.equal(flat.cpu(), flat2) and dj.fallback == 0
    assert torch.equal(DeviceResize(64)(flat, sizes), DeviceResize(64)(flat2, sizes2))


def _first_step_loss(out):
    line = next(l for l in out.splitlines() if "Epoch: [0][0/" in l)
    return re.search(r"Loss \(L1\) ([0-9.]+)", line).group(1)


def test_train_py_cli_gpu_decode_matches_gpu_resize_first_step(tmp_path):
    """train.py --gpu_decode on a tiny generated JPEG folder: two steps and a validation pass; with --workers 0 and the same seed the
    first step's loss is that of the --gpu_resize run (same pixels reach the network)."""
    import pandas as pd
    from PIL import Image
    from conftest import records_dir
    rng = np.random.default_rng(5)
    data = tmp_path / "data"
    (data / "imgs").mkdir(parents=True)
    ages = [30] * 110 + [40] * 28 + [50] * 12 + [30, 40, 50] * 4 + [30, 40, 50] * 4     # many-, median- and low-shot labels, each in val and test
    splits = ["train"] * 150 + ["val"] * 12 + ["test"] * 12
    rows = []
    for k, (age, split) in enumerate(zip(ages, splits)):
        h, w = int(rng.integers(60, 120)), int(rng.integers(60, 120))
        yy, xx = np.mgrid[0:h, 0:w]
        arr = np.stack([128 + 90 * np.sin(xx / (5 + c) + k) * np.cos(yy / (7 - c)) for c in range(3)], -1) + rng.normal(0, 8, (h, w, 3))
        kw = [dict(subsampling=2), dict(subsampling=0, optimize=True), dict(subsampling=1), dict(progressive=True)][k % 4]      # one in four falls back
        Image.fromarray(np.clip(arr, 0, 255).astype(np.uint8)).save(data / "imgs" / f"{k}.jpg", quality=85, **kw)
        rows.append({"age": age, "path": f"imgs/{k}.jpg", "split": split})
    pd.DataFrame(rows).to_csv(data / "agedb.csv", index=False)
    base = ["--dataset", "agedb", "--data_dir", str(data), "--batch_size", "32", "--epoch", "1", "--workers", "0", "--img_size", "224",
            "--print_freq", "1", "--max_steps", "2"]
    # agedb-dir/train.py itself, as `python train.py ...` runs it, behind a fixed seed (the command line has none): weights, the loader's
    # order and the crop / flip draws are then the same in both runs
    script = os.path.join(PKG, "agedb-dir", "train.py")
    driver = ("import os, runpy, sys, torch; torch.manual_seed(0); sys.argv = sys.argv[1:]; sys.path.insert(0, os.path.dirname(sys.argv[0])); "
              "runpy.run_path(sys.argv[0], run_name='__main__')")
    losses = {}
    for tag, extra in (("gpu_decode", ["--gpu_decode"]), ("gpu_resize", ["--gpu_resize"])):
        cmd = [sys.executable, "-c", driver, script] + base + extra + ["--store_root", str(tmp_path / tag)]
        p = subprocess.run(cmd, cwd=os.path.dirname(script), capture_output=True, text=True, timeout=600)
        out = p.stdout + p.stderr
        with open(os.path.join(records_dir(), f"cli_files_{tag}_jpeg.log"), "w") as f:
            f.write(" ".join(cmd) + "\n" + out)
        assert p.returncode == 0, out[-3000:]
        for needle in ("Training data size: 150", "Validation data size: 12", "Epoch: [0][1/", " * Overall: MSE", "Test loss: MSE"):
            assert needle in out, (tag, needle)
        losses[tag] = _first_step_loss(out)
    assert losses["gpu_decode"] == losses["gpu_resize"], losses
