"""numpy restatement of the tail's dropout mask (a helper module, imported by tests/test_dropout_host.py and
tests/test_hip_dropout.py): Philox4x32-10 with the Random123 constants, and the mask of include/dir_hip.h

    key = (seed & 0xffffffff, seed >> 32), counter = ((e >> 2) & 0xffffffff, (e >> 2) >> 32, offset & 0xffffffff, offset >> 32),
    r = philox(counter, key)[e & 3], keep = r < min(floor((1 - p) * 2^32), 2^32 - 1), scale = float32(1 / (1 - p)) (0 at p = 1)

for element e = b * C + c of a [B, C] tensor.
"""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_LO = np.uint64(0xffffffff)
_SH = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 uint32 arrays (or ints), key: 2 -> the 4 output words (uint32 arrays)."""
    c = [np.asarray(x, dtype=np.uint32) for x in counter]
    k0, k1 = np.asarray(key[0], dtype=np.uint32), np.asarray(key[1], dtype=np.uint32)
    with np.errstate(over="ignore"):
        for i in range(10):
            if i:
                k0, k1 = k0 + W0, k1 + W1
            p0, p1 = M0 * c[0].astype(np.uint64), M1 * c[2].astype(np.uint64)
            hi0, lo0 = (p0 >> _SH).astype(np.uint32), (p0 & _LO).astype(np.uint32)
            hi1, lo1 = (p1 >> _SH).astype(np.uint32), (p1 & _LO).astype(np.uint32)
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return c


def threshold(p):
    return min(math.floor((1.0 - p) * 2.0 ** 32), 2 ** 32 - 1)


def scale(p):
    return np.float32(0.0) if p == 1.0 else np.float32(1.0 / (1.0 - p))


def mask(seed, offset, p, b, c):
    """keep [b, c] (bool) of the tail's dropout for (seed, offset, p)."""
    e = np.arange(b * c, dtype=np.uint64)
    q = e >> np.uint64(2)
    words = philox4x32_10(((q & _LO).astype(np.uint32), (q >> _SH).astype(np.uint32),
                           np.full(q.shape, offset & 0xffffffff, np.uint32), np.full(q.shape, offset >> 32, np.uint32)),
                          (seed & 0xffffffff, seed >> 32))
    r = np.choose((e & np.uint64(3)).astype(np.int64), words)
    return (r.astype(np.uint64) < np.uint64(threshold(p))).reshape(b, c)
