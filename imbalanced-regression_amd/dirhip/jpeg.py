"""JPEG decode with the GPU doing the data-parallel half.

``DeviceJpeg.decode(files)`` takes the compressed bytes of a batch and returns ``(flat, sizes)`` — the ragged uint8 RGB batch
``datasets.DeviceResize`` consumes — bit for bit ``np.asarray(Image.open(f).convert('RGB'))``:

  * host, in threads of this process: ``dir_jpeg_inspect`` (markers) and ``dir_jpeg_entropy_decode`` (Huffman) on the file bytes, into
    one pinned int16 coefficient buffer (the ctypes calls release the GIL);
  * one host-to-device copy (row table, quantisation tables and coefficients share the staging buffer);
  * ``dir_jpeg_reconstruct``: dequantise + inverse DCT, chroma upsampling + YCbCr -> RGB, two HIP launches.

What the native decoder takes is listed in ``csrc/dir_jpeg_host.cpp``: baseline / extended-sequential Huffman files with one
interleaved scan, grayscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0, up to 8192 x 8192. Every other file that Pillow can open (progressive, CMYK,
Adobe-marked, other sampling, PNG ...) and every file the native stage rejects is decoded by Pillow on the host and its pixels are
copied into its slice of ``flat``; ``taken`` / ``fallback`` / ``failed`` count the files. The GPU stage has no fallback of its own.
"""
import ctypes
import io
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib as L

ROW = 8                                     # DIR_JPEG_ROW
MAX_THREADS = 16


class JpegInfo(ctypes.Structure):
    """``dir_jpeg_info`` of include/dir_hip.h."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ncomp", ctypes.c_int32), ("hsamp", ctypes.c_int32),
                ("vsamp", ctypes.c_int32), ("blocks_w", ctypes.c_int32 * 3), ("blocks_h", ctypes.c_int32 * 3),
                ("restart_interval", ctypes.c_int32), ("ncoef", ctypes.c_int64), ("quant", (ctypes.c_uint16 * 64) * 3)]


def _as_array(f):
    """File bytes as a contiguous uint8 numpy array, without a copy where the input allows it (bytes, uint8 tensors, arrays)."""
    if isinstance(f, torch.Tensor):
        f = f.numpy()
    if isinstance(f, np.ndarray):
        assert f.dtype == np.uint8 and f.ndim == 1
        return np.ascontiguousarray(f)
    return np.frombuffer(f, dtype=np.uint8)


def inspect(data):
    """``(rc, info)``: rc 0 = taken, ``DIR_EUNSUPPORTED`` = a JPEG the native decoder leaves to Pillow, ``DIR_EINVAL`` = invalid."""
    data, info = _as_array(data), JpegInfo()
    rc = L.lib().dir_jpeg_inspect(ctypes.c_void_p(data.ctypes.data), data.size, ctypes.byref(info))
    return rc, info


def entropy_decode(data, info, out):
    """Quantised coefficients of a taken file into ``out`` (a contiguous int16 numpy array of at least ``info.ncoef`` elements); returns rc."""
    assert out.dtype == np.int16 and out.flags["C_CONTIGUOUS"]
    data = _as_array(data)
    return L.lib().dir_jpeg_entropy_decode(ctypes.c_void_p(data.ctypes.data), data.size, ctypes.byref(info), ctypes.c_void_p(out.ctypes.data), out.size)


def _pillow_rgb(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data.tobytes())).convert("RGB"), dtype=np.uint8)      # (a copy: writable, for torch.from_numpy)


class DeviceJpeg:
    def __init__(self, device=None, threads=8):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise L.DirHipError(f"DeviceJpeg: target device {self.device}; the reconstruction kernels run only on the GPU")
        self.threads = max(1, min(int(threads), MAX_THREADS))
        self.pool = ThreadPoolExecutor(self.threads) if self.threads > 1 else None
        self.taken = self.fallback = self.failed = 0
        # pinned staging buffers, reused round robin and grown in powers of two: a fresh pinned block of another size per batch would
        # fragment the host caching allocator; the event says when the copy out of a buffer has finished
        self._ring, self._next = [[None, None] for _ in range(3)], 0

    def _stage(self, nbytes):
        slot = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        if slot[1] is not None:
            slot[1].synchronize()
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(max(1 << 20, 1 << (nbytes - 1).bit_length()), dtype=torch.uint8, pin_memory=True)
        return slot

    def _map(self, fn, items):
        return list(self.pool.map(fn, items)) if self.pool is not None and len(items) > 1 else [fn(x) for x in items]

    def decode(self, files):
        """``files``: a list of ``bytes`` (or 1-D uint8 tensors / arrays). Returns ``flat`` uint8 on the device and ``sizes`` int64 ``[B, 2]`` = (H, W) on the
        host. A file neither stage can decode raises ``DirHipError`` naming its index before anything is launched."""
        plan = self.host_stage(files)
        flat = torch.empty(plan["flat_bytes"], dtype=torch.uint8, device=self.device)
        if plan["native"]:
            slot = plan["slot"]
            stage_d = plan["stage"].to(self.device, non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record(torch.cuda.current_stream(self.device))
            self.reconstruct(plan, stage_d, flat)
        for off, px in plan["host"]:
            flat[off:off + px.size].copy_(torch.from_numpy(px.reshape(-1)))
        return flat, torch.from_numpy(plan["sizes"])

    def host_stage(self, files):
        """Everything before the copy: inspect, entropy decode (thread pool) and Pillow fallbacks. The plan holds the pinned staging bytes
        ``[row table int64 [B][8]][quant uint16 [B][3][64]][coefficients int16]`` and what ``reconstruct`` needs to launch on a device copy of them."""
        files = [_as_array(f) for f in files]
        n = len(files)
        if n == 0:
            raise ValueError("DeviceJpeg.decode: empty batch")
        probed = self._map(inspect, files)
        native = [i for i, (rc, _) in enumerate(probed) if rc == 0]
        coef_off, total = {}, 0
        for i in native:
            coef_off[i] = total
            total += int(probed[i][1].ncoef)
        table_bytes = n * ROW * 8
        quant_bytes = n * 3 * 64 * 2
        head = (table_bytes + quant_bytes + 15) // 16 * 16
        slot = self._stage(head + 2 * total)
        stage = slot[0][:head + 2 * total]
        stage_np = stage.numpy()
        table = stage_np[:table_bytes].view(np.int64).reshape(n, ROW)
        quant = stage_np[table_bytes:table_bytes + quant_bytes].view(np.uint16).reshape(n, 3, 64)
        coef = stage_np[head:].view(np.int16)
        table[:] = 0
        quant[:] = 0

        def run(i):
            info = probed[i][1]
            return entropy_decode(files[i], info, coef[coef_off[i]:coef_off[i] + int(info.ncoef)])
        rcs = dict(zip(native, self._map(run, native)))
        native = [i for i in native if rcs[i] == 0]                 # a scan the native stage rejects is Pillow's to judge
        host, sizes = {}, np.zeros((n, 2), dtype=np.int64)
        for i in range(n):
            if rcs.get(i) == 0:
                sizes[i] = (probed[i][1].height, probed[i][1].width)
                continue
            try:
                host[i] = _pillow_rgb(files[i])
            except Exception as e:                                  # noqa: BLE001  (whatever Pillow raises for this file)
                self.failed += 1
                raise L.DirHipError(f"DeviceJpeg.decode: file {i} of the batch ({files[i].size} bytes) cannot be decoded: {e}") from e
            sizes[i] = host[i].shape[:2]
        nbytes = sizes[:, 0] * sizes[:, 1] * 3
        flat_off = np.cumsum(nbytes) - nbytes
        max_blocks = max_pixels = 0
        for k, i in enumerate(native):                              # row k <-> quant slot k: the native files, in batch order
            info = probed[i][1]
            table[k] = (coef_off[i], flat_off[i], info.width, info.height, info.ncomp, info.hsamp, info.vsamp, k)
            quant[k] = np.ctypeslib.as_array(info.quant)
            max_blocks = max(max_blocks, int(info.ncoef) // 64)
            max_pixels = max(max_pixels, info.width * info.height)
        self.taken += len(native)
        self.fallback += len(host)
        return dict(slot=slot, stage=stage, head=head, table_bytes=table_bytes, ncoef=total, native=len(native), max_blocks=max_blocks,
                    max_pixels=max_pixels, flat_bytes=int(nbytes.sum()), sizes=sizes, host=[(int(flat_off[i]), px) for i, px in host.items()])

    def reconstruct(self, plan, stage_d, flat):
        """The two HIP launches on ``stage_d``, the device copy of the plan's staging bytes; writes the native files' pixels into ``flat``."""
        lib = L.lib()
        ws_bytes = lib.dir_jpeg_reconstruct_workspace(plan["ncoef"])
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        base = stage_d.data_ptr()
        L.check(lib.dir_jpeg_reconstruct(ctypes.c_void_p(base + plan["head"]), plan["ncoef"], ctypes.c_void_p(base + plan["table_bytes"]), plan["native"],
                                         ctypes.c_void_p(base), plan["native"], plan["max_blocks"], plan["max_pixels"], L.ptr(flat), flat.numel(),
                                         L.ptr(ws), ws_bytes, L.stream_ptr(self.device)), "dir_jpeg_reconstruct")
