"""JPEG files for tests/test_jpeg_host.py and tests/test_hip_jpeg.py, written by Pillow from seeded numpy arrays (no file from anywhere
else): every size group as white noise (range limiting, large coefficients) and as a smooth gradient plus low noise. The sizes are the
smallest at which each code path can go wrong: partial MCUs on both edges, one-block images, chroma rows of 3 samples, restart resets."""
import io

import numpy as np
from PIL import Image

GRAY_SIZES = [(8, 8), (9, 31)]                                          # (W, H)
COLOUR_SIZES = [(16, 16), (17, 23), (23, 17), (40, 8), (6, 5)]


def _pixels(kind, w, h, channels, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        a = rng.integers(0, 256, (h, w, channels))
    else:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        a = np.stack([40 + 170 * (xx * (c + 1) + yy * (3 - c)) / max(1.0, (w - 1) * (c + 1) + (h - 1) * (3 - c)) for c in range(channels)], -1)
        a = a + rng.normal(0, 3, a.shape)
    a = np.clip(a, 0, 255).astype(np.uint8)
    return a[:, :, 0] if channels == 1 else a


def jpeg_bytes(arr, **save):
    buf = io.BytesIO()
    (arr if isinstance(arr, Image.Image) else Image.fromarray(arr)).save(buf, "JPEG", **save)
    return buf.getvalue()


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def taken_fixtures():
    """[(name, file bytes)]: every file here must be TAKEN by the native decoder."""
    out, seed = [], 0
    for kind in ("noise", "smooth"):
        for (w, h) in GRAY_SIZES:
            seed += 1
            out.append((f"gray_{w}x{h}_{kind}", jpeg_bytes(_pixels(kind, w, h, 1, seed), quality=75)))
        for (w, h) in COLOUR_SIZES:
            for sub in (0, 1, 2):
                seed += 1
                out.append((f"colour_{w}x{h}_s{sub}_{kind}", jpeg_bytes(_pixels(kind, w, h, 3, seed), quality=75, subsampling=sub)))
        for q in (30, 75, 95, 100):
            seed += 1
            out.append((f"quality{q}_{kind}", jpeg_bytes(_pixels(kind, 17, 23, 3, seed), quality=q, subsampling=2)))
        seed += 1
        out.append((f"optimize_{kind}", jpeg_bytes(_pixels(kind, 17, 23, 3, seed), quality=75, subsampling=2, optimize=True)))
        seed += 1
        out.append((f"restart_blocks_{kind}", jpeg_bytes(_pixels(kind, 17, 23, 3, seed), quality=75, subsampling=2, restart_marker_blocks=1)))
        seed += 1
        out.append((f"restart_rows_{kind}", jpeg_bytes(_pixels(kind, 17, 23, 3, seed), quality=75, subsampling=2, restart_marker_rows=1)))
        seed += 1
        out.append((f"larger_{kind}", jpeg_bytes(_pixels(kind, 67, 131, 3, seed), quality=75, subsampling=2)))
    return out


def narrow_fixtures():
    """Widths 1 .. 4 (chroma rows of one or two samples: the library's upsampler replicates) — taken as well."""
    out = []
    for w in (1, 2, 3, 4):
        for sub in (1, 2):
            out.append((f"narrow_{w}x11_s{sub}", jpeg_bytes(_pixels("noise", w, 11, 3, 100 + 4 * w + sub), quality=90, subsampling=sub)))
    return out


def not_taken_fixtures():
    """Valid JPEGs the native decoder must leave to Pillow."""
    rgb = _pixels("smooth", 24, 20, 3, 200)
    cmyk = Image.frombytes("CMYK", (24, 20), np.concatenate([rgb, rgb[:, :, :1]], -1).tobytes())
    # Pillow does not write 4:4:0; a 16 x 16 4:2:2 file has the same two MCUs of four blocks, so swapping the luma sampling byte of its
    # SOF0 (h2 v1 -> h1 v2) leaves a valid 4:4:0 stream (of another picture)
    s440 = bytearray(jpeg_bytes(_pixels("smooth", 16, 16, 3, 201), quality=75, subsampling=1))
    at = s440.index(b"\xff\xc0") + 11
    assert s440[at] == 0x21
    s440[at] = 0x12
    return [("progressive", jpeg_bytes(rgb, quality=75, progressive=True)),
            ("cmyk", jpeg_bytes(cmyk, quality=75)),
            ("rgb_coded", jpeg_bytes(rgb, quality=75, keep_rgb=True)),
            ("s440", bytes(s440))]
