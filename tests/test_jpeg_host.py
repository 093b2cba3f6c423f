"""-m "not gpu": the host half of the JPEG decoder (csrc/dir_jpeg_host.cpp: dir_jpeg_inspect, dir_jpeg_entropy_decode) against Pillow,
and the arithmetic the device half (csrc/dir_jpeg.hip) must implement, restated here in numpy integers: applied to the host stage's
coefficients it reproduces np.asarray(Image.open(f).convert('RGB')) bit for bit on every fixture of tests/jpeg_fixtures.py.
The GPU side of the same fixtures is tests/test_hip_jpeg.py."""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

from conftest import ROOT
import jpeg_fixtures as F

OK, EINVAL, EUNSUPPORTED = 0, -1, -2


# ---------------------------------------------------------------- numpy restatement of the device stage (libjpeg's integer arithmetic)
def _idct_pass(v):
    """jidctint.c's 1-D pass on axis -1 (eight values), before the descale; int64 like the library's long."""
    z2, z3 = v[..., 2], v[..., 6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    z2, z3 = v[..., 0], v[..., 4]
    tmp0, tmp1 = (z2 + z3) << 13, (z2 - z3) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[..., 7], v[..., 5], v[..., 3], v[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3], -1)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def idct_islow(coef, quant):
    """coef int [n, 64] natural order, quant [64] -> uint8 [n, 8, 8]: dequantise, column pass, row pass, range limit."""
    v = (coef.astype(np.int64) * quant.astype(np.int64)).reshape(-1, 8, 8)
    ws = _descale(_idct_pass(v.transpose(0, 2, 1)), 13 - 2).transpose(0, 2, 1)          # columns: the 1-D pass along axis 1
    out = _descale(_idct_pass(ws), 13 + 2 + 3)
    s = ((out & 1023) ^ 512) - 512                                                      # the range-limit table: low 10 bits, signed
    return np.clip(s + 128, 0, 255).astype(np.uint8)


def _plane(blocks, bw, bh):
    return blocks.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _upsample(p, W, H, hs, vs):
    """jdsample.c: a chroma plane (padded) -> [H, W] int; the filters' edges are the TRUE down-sampled size."""
    cw, ch = -(-W // hs), -(-H // vs)
    p = p[:ch, :cw].astype(np.int64)
    x, y = np.arange(W), np.arange(H)
    if hs == 1:
        return p[:H, :W]
    cx = x >> 1
    cy = y >> 1 if vs == 2 else y
    if cw <= 2:                                                                         # fancy upsampling needs more than two samples
        return p[cy][:, cx]
    nx = np.where(x & 1, np.minimum(cx + 1, cw - 1), np.maximum(cx - 1, 0))
    if vs == 1:
        return (3 * p[:, cx] + p[:, nx] + np.where(x & 1, 2, 1)) >> 2
    ny = np.where(y & 1, np.minimum(cy + 1, ch - 1), np.maximum(cy - 1, 0))
    col = 3 * p[cy] + p[ny]                                                             # vertical stage, [H, cw]
    return (3 * col[:, cx] + col[:, nx] + np.where(x & 1, 7, 8)) >> 4


def reconstruct(info, coef):
    """The device stage on one image: RGB uint8 [H, W, 3]."""
    W, H = info.width, info.height
    planes, at = [], 0
    for c in range(info.ncomp):
        bw, bh = info.blocks_w[c], info.blocks_h[c]
        q = np.ctypeslib.as_array(info.quant)[c]
        planes.append(_plane(idct_islow(coef[at:at + bw * bh * 64].reshape(-1, 64), q), bw, bh))
        at += bw * bh * 64
    assert at == info.ncoef
    Y = planes[0][:H, :W].astype(np.int64)
    if info.ncomp == 1:
        return np.stack([Y, Y, Y], -1).astype(np.uint8)
    cb = _upsample(planes[1], W, H, info.hsamp, info.vsamp) - 128
    cr = _upsample(planes[2], W, H, info.hsamp, info.vsamp) - 128
    fix = lambda v: int(v * 65536 + .5)                                                 # noqa: E731  (jdcolor.c's FIX)
    R = Y + ((fix(1.40200) * cr + 32768) >> 16)
    G = Y + ((-fix(0.34414) * cb + 32768 - fix(0.71414) * cr) >> 16)
    B = Y + ((fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], -1), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- helpers
def _decode(data):
    from dirhip import jpeg
    rc, info = jpeg.inspect(data)
    if rc != OK:
        return rc, info, None
    coef = np.full(info.ncoef + 64, 0x5A5A, dtype=np.int16)                              # 64 guard elements behind the capacity
    rc = jpeg.entropy_decode(data, info, coef[:info.ncoef])
    assert np.all(coef[info.ncoef:] == 0x5A5A), "wrote past capacity"
    return rc, info, coef[:info.ncoef]


@pytest.fixture(scope="module")
def taken():
    return F.taken_fixtures()


# ---------------------------------------------------------------- tests
def test_every_fixture_is_taken_with_pillows_geometry_and_tables(taken):
    from dirhip import jpeg
    for name, data in taken + F.narrow_fixtures():
        rc, info = jpeg.inspect(data)
        assert rc == OK, (name, rc)
        im = Image.open(io.BytesIO(data))
        assert (info.width, info.height) == im.size, name
        assert info.ncomp == len(im.layer) == (1 if im.mode == "L" else 3), name
        assert (info.hsamp, info.vsamp) == (im.layer[0][1], im.layer[0][2]), name
        hs, vs = info.hsamp, info.vsamp
        mx, my = -(-info.width // (8 * hs)), -(-info.height // (8 * vs))
        want_w = [mx * hs] + [mx] * (info.ncomp - 1)
        want_h = [my * vs] + [my] * (info.ncomp - 1)
        assert list(info.blocks_w)[:info.ncomp] == want_w and list(info.blocks_h)[:info.ncomp] == want_h, name
        assert info.ncoef == 64 * sum(w * h for w, h in zip(want_w, want_h)), name
        # Image.quantization of this Pillow: table id -> 64 values in natural (row-major) order; pin that on the standard luminance
        # table's first row (16 11 10 16 ... scaled), which zig-zag order would give as 16 11 12 14 ...
        q = np.ctypeslib.as_array(info.quant)
        for c, layer in enumerate(im.layer):
            assert list(q[c]) == list(im.quantization[layer[3]]), (name, c)
        if "restart_blocks" in name:
            assert info.restart_interval == 1, name
        elif "restart_rows" in name:
            assert info.restart_interval == mx, name
        else:
            assert info.restart_interval == 0, name
    std = Image.open(io.BytesIO(F.jpeg_bytes(np.zeros((8, 8), np.uint8), quality=50))).quantization[0]
    assert list(std[:8]) == [16, 11, 10, 16, 24, 40, 51, 61]


def test_restated_device_arithmetic_on_host_coefficients_equals_pillow(taken):
    """Fails with an import error before the feature exists. Host entropy decode + numpy IDCT / upsampling / colour == Pillow, bit for bit."""
    for name, data in taken + F.narrow_fixtures():
        rc, info, coef = _decode(data)
        assert rc == OK, (name, rc)
        got, want = reconstruct(info, coef), F.pillow_rgb(data)
        assert got.shape == want.shape and np.array_equal(got, want), (name, int((got != want).sum()))


def test_files_outside_the_list_are_not_taken():
    from dirhip import jpeg
    for name, data in F.not_taken_fixtures():
        assert F.pillow_rgb(data).ndim == 3, name                                    # a valid file: Pillow decodes it
        rc, _ = jpeg.inspect(data)
        assert rc == EUNSUPPORTED, (name, rc)
    rc, _ = jpeg.inspect(b"\x89PNG\r\n\x1a\n" + bytes(64))
    assert rc == EINVAL
    rc, _ = jpeg.inspect(b"")
    assert rc == EINVAL


def test_truncation_at_every_offset_never_passes_a_short_scan(taken):
    for name in ("colour_17x23_s2_noise", "restart_blocks_smooth", "gray_9x31_noise"):
        data = dict(taken)[name]
        rc, info, full = _decode(data)
        assert rc == OK
        for cut in range(len(data)):
            rc, _, coef = _decode(data[:cut])
            assert rc in (OK, EINVAL, EUNSUPPORTED), (name, cut, rc)
            if rc == OK and coef is not None:                                         # only once the whole scan is there (EOI may be missing)
                assert np.array_equal(coef, full), (name, cut)
                assert cut >= len(data) - 2, (name, cut)
            if coef is None:
                assert rc == EINVAL, (name, cut, rc)                                  # a cut header is invalid, never "not taken"


def test_corrupted_scan_bytes_give_ok_or_einval(taken):
    rng = np.random.default_rng(7)
    for name in ("colour_17x23_s2_noise", "optimize_noise", "restart_rows_noise", "larger_smooth"):
        data = dict(taken)[name]
        start = data.index(b"\xff\xda")
        for pos in rng.integers(start + 2, len(data), 200):
            for val in (0x00, 0xFF, int(rng.integers(0, 256))):
                bad = bytearray(data)
                bad[pos] = val
                rc, _, _ = _decode(bytes(bad))
                assert rc in (OK, EINVAL, EUNSUPPORTED) and (rc != EUNSUPPORTED or pos < start + 14), (name, int(pos), val, rc)


def test_capacity_one_short_and_foreign_info_are_refused(taken):
    from dirhip import jpeg
    data = dict(taken)["colour_17x23_s2_noise"]
    rc, info = jpeg.inspect(data)
    coef = np.full(info.ncoef, 0x5A5A, dtype=np.int16)
    assert jpeg.entropy_decode(data, info, coef[:info.ncoef - 1]) == EINVAL
    assert np.all(coef == 0x5A5A)                                                     # nothing written
    other = dict(taken)["colour_16x16_s0_noise"]
    assert jpeg.entropy_decode(other, info, coef) == EINVAL                           # info of another file
    assert jpeg.entropy_decode(data, info, coef) == OK
    lib = __import__("dirhip")._lib.lib()
    assert lib.dir_jpeg_inspect(None, 10, ctypes.byref(info)) == EINVAL and lib.dir_jpeg_inspect(data, len(data), None) == EINVAL


def test_entropy_decode_from_many_threads_is_deterministic(taken):
    from concurrent.futures import ThreadPoolExecutor
    files = [d for _, d in taken]
    ref = [_decode(d)[2] for d in files]
    with ThreadPoolExecutor(8) as pool:
        for _ in range(3):
            got = list(pool.map(lambda d: _decode(d)[2], files))
            assert all(np.array_equal(a, b) for a, b in zip(got, ref))


def test_surface_header_signatures_exports_abi():
    from dirhip import _lib
    from dirhip.jpeg import JpegInfo
    header = open(os.path.join(ROOT, "include", "dir_hip.h")).read()
    declared = set(re.findall(r"\b(dir_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("dir_jpeg_inspect", "dir_jpeg_entropy_decode", "dir_jpeg_reconstruct_workspace", "dir_jpeg_reconstruct"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(handle, name) and f" T {name}\n" in exported, name
    c = ctypes
    assert _lib.SIGNATURES["dir_jpeg_inspect"] == (c.c_int, [c.c_void_p, c.c_size_t, c.c_void_p])
    assert _lib.SIGNATURES["dir_jpeg_entropy_decode"] == (c.c_int, [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_size_t])
    assert _lib.SIGNATURES["dir_jpeg_reconstruct_workspace"] == (c.c_size_t, [c.c_longlong])
    assert len(_lib.SIGNATURES["dir_jpeg_reconstruct"][1]) == 13
    assert ctypes.sizeof(JpegInfo) == 48 + 8 + 3 * 64 * 2                              # dir_jpeg_info: 12 int32, int64, uint16 [3][64]
    assert "#define DIR_ABI_VERSION 4" in header and _lib.lib().dir_abi_version() == _lib.ABI_VERSION == 4
    lib = _lib.lib()
    assert lib.dir_jpeg_reconstruct_workspace(0) == 0 and lib.dir_jpeg_reconstruct_workspace(640) >= 640
    assert lib.dir_jpeg_reconstruct(None, 64, None, 1, None, 1, 1, 64, None, 192, None, 0, None) == EINVAL      # null pointers: no launch
