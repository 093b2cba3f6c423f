"""CPU-side tests of the fused tail's dropout: the numpy restatement of the Philox4x32-10 mask against the Random123 known-answer
vectors, the three C-ABI entry points (exported, declared, typed; argument errors without a GPU), and the --dropout flag."""
import ctypes
import os
import re

import numpy as np
import pytest

import dropout_reference as R
from conftest import ROOT

NEW_SYMBOLS = ("dir_tail_dropout_fwd", "dir_tail_dropout_bwd", "dir_dropout_mask")


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox4x32_10_known_answers(counter, key, want):
    assert tuple(int(w) for w in R.philox4x32_10(counter, key)) == want


def test_mask_restatement_layout_and_rate():
    seed, offset = 0x1234_5678_9abc_def0, 0x1_0000_0008
    keep = R.mask(seed, offset, 0.5, 3, 40)
    # element e = b * C + c reads word e & 3 of the Philox call at counter (e >> 2, offset)
    for b, c in [(0, 0), (0, 3), (1, 5), (2, 39)]:
        e = b * 40 + c
        w = R.philox4x32_10((e >> 2, 0, offset & 0xffffffff, offset >> 32), (seed & 0xffffffff, seed >> 32))[e & 3]
        assert bool(keep[b, c]) == (int(w) < 2 ** 31)
    assert R.threshold(0.0) == 2 ** 32 - 1 and R.threshold(1.0) == 0 and R.threshold(0.5) == 2 ** 31
    assert R.scale(1.0) == 0.0 and R.scale(0.5) == np.float32(2.0) and R.scale(0.1) == np.float32(1.0 / 0.9)
    big = R.mask(7, 4, 0.3, 64, 512)
    n = big.size
    assert abs(big.mean() - 0.7) < 6 * np.sqrt(0.7 * 0.3 / n)
    assert not R.mask(7, 4, 1.0, 4, 16).any() and (R.mask(7, 8, 0.3, 64, 512) != big).any()


def test_dropout_entry_points_exported_declared_and_typed():
    from dirhip import _lib
    header = open(os.path.join(ROOT, "include", "dir_hip.h")).read()
    declared = set(re.findall(r"\b(dir_[a-z0-9_]+)\s*\(", header))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(handle, name), name
    u64 = ctypes.c_uint64
    assert _lib.SIGNATURES["dir_dropout_mask"][1][:3] == [u64, u64, ctypes.c_double]
    for name, base in (("dir_tail_dropout_fwd", "dir_tail_fwd"), ("dir_tail_dropout_bwd", "dir_tail_bwd")):
        # <the plain entry's arguments>, seed, offset, p, stream
        assert _lib.SIGNATURES[name][1] == _lib.SIGNATURES[base][1][:-1] + [u64, u64, ctypes.c_double, ctypes.c_void_p]
    assert "#define DIR_ABI_VERSION 4" in header
    assert _lib.lib().dir_abi_version() == _lib.ABI_VERSION == 4


def test_dropout_argument_errors_without_gpu():
    from dirhip import _lib
    L = _lib.lib()
    einval = -1
    for p in (-0.1, 1.5, float("nan")):
        assert L.dir_dropout_mask(1, 0, p, 4, 8, None, None) == einval
        assert L.dir_tail_dropout_fwd(None, _lib.DIR_F32, None, None, 4, 49, 8, 0, 1, None, None, None, None, None, None, None, None,
                                      1, 0, p, None) == einval
        assert L.dir_tail_dropout_bwd(None, None, None, None, None, None, 4, 49, 8, _lib.DIR_F32, None, None, None, None, 0,
                                      1, 0, p, None) == einval
    assert L.dir_dropout_mask(1, 0, 0.5, 0, 8, None, None) == 0                  # empty: nothing to launch
    assert L.dir_dropout_mask(1, 0, 0.5, 4, 8, None, None) == einval             # no output buffer
    assert L.dir_tail_dropout_fwd(None, _lib.DIR_F32, None, None, 0, 49, 8, 0, 1, None, None, None, None, None, None, None, None,
                                  1, 0, 0.5, None) == 0


def test_dropout_cli_flag():
    from dirhip.train_main import build_parser, make_store_name
    base = ["--fds", "--reweight", "sqrt_inv"]
    a = build_parser().parse_args(base)
    assert a.dropout is None
    plain = make_store_name(a)
    assert plain == "imdb_wiki_resnet50_sqrt_inv_fds_gau_5_1_0_1_0.9_adam_l1_0.001_256"            # unchanged without the flag
    d = build_parser().parse_args(base + ["--dropout", "0.5"])
    assert d.dropout == 0.5
    assert make_store_name(d) == plain.replace("_0.9_adam", "_0.9_dropout_0.5_adam")
    assert build_parser("agedb").parse_args(["--dropout", "0.1"]).dropout == 0.1
