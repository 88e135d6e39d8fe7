"""The decoder's LZ stage on the GPU is part of the C-ABI: include/agmv_hip.h declares it, libagmv_hip.so exports it and
AgmvHip wraps it (the GPU behaviour is pinned by tests/test_gpu_lz_decode.py)."""
import ctypes as C
import os
import re

import numpy as np

import lz_decode_cases as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("agmv_hip_lz_decode_frames_dev", "agmv_hip_lz_decode_commit_dev", "agmv_hip_lz_decode_fallback_frames",
         "agmv_hip_lz_decode_frames")


def test_header_declares_the_lz_decode_stage():
    hdr = open(os.path.join(ROOT, "include", "agmv_hip.h")).read()
    for f in FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % f, hdr), f


def test_library_exports_and_wrapper_methods():
    from libagmv_amd import build, hip
    from libagmv_amd.hip import AgmvHip
    build.build()
    L = C.CDLL(hip.lib_path())
    for f in FUNCS:
        assert hasattr(L, f), f
        assert f in hip.ABI_SYMBOLS, f
    for m in ("lz_decode_frames_dev", "lz_decode_commit_dev", "lz_decode_fallback_frames", "lz_decode_frames"):
        assert callable(getattr(AgmvHip, m, None)), m


def test_batch_reference_and_commit_restatement():
    """the helpers the GPU tests compare against: a crafted stream through the host stage, and the commit loop"""
    fr = [Z.lzss_frame([("L", 1), ("L", 2), ("M", 2, 6)], csize=5), Z.lz77_frame([(0, 0, 7), (1, 4, 8)]),
          Z.lzss_frame([("L", 3)] * 5, csize=6)]
    before, rows, bpos, used, per = Z.host_batch(1, fr[:1] + fr[2:], 64, persist=np.arange(64, dtype=np.uint8))
    assert list(bpos) == [8, 5] and list(before[0, :8]) == [1, 2, 1, 2, 1, 2, 1, 2]
    assert Z.host_batch(1, [Z.lzss_frame([("L", 1), ("L", 2), ("M", 2, 6)])], 64)[2][0] == 2   # csize 4: the match reads guard bits
    assert list(rows[1, 5:21]) == list(before[0, 5:8]) + list(range(8, 21))
    assert list(per[:8]) == [3, 3, 3, 3, 3, 2, 1, 2] and list(per[8:]) == list(range(8, 64))
    _, _, bpos, used, _ = Z.host_batch(3, fr[1:2], 64)
    assert list(bpos) == [6] and used[0] == 8
