"""The encoder's LZ77 stage on the GPU is part of the C-ABI: include/agmv_hip.h declares it, libagmv_hip.so exports it and
AgmvHip wraps it (the GPU behaviour is pinned by tests/test_gpu_lz77.py)."""
import ctypes as C
import os
import re

import numpy as np

import lz77_cases as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("agmv_hip_lz77_peek_dev", "agmv_hip_lz77_frames_dev", "agmv_hip_lz77_frames", "agmv_hip_lz77_reparsed_segments")


def test_header_declares_the_lz77_stage():
    hdr = open(os.path.join(ROOT, "include", "agmv_hip.h")).read()
    assert re.search(r"\bsize_t\s+agmv_hip_lz77_max_csize\s*\(", hdr)
    for f in FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % f, hdr), f


def test_library_exports_and_wrapper_methods():
    from libagmv_amd import hip
    from libagmv_amd.hip import AgmvHip
    L = hip.load_library()
    for f in FUNCS + ("agmv_hip_lz77_max_csize",):
        assert hasattr(L, f), f
        assert f in hip.ABI_SYMBOLS, f
    for m in ("lz77_max_csize", "lz77_peek_dev", "lz77_frames_dev", "lz77_frames", "lz77_reparsed_segments"):
        assert callable(getattr(AgmvHip, m, None)), m


def test_max_csize_closed_form():
    from libagmv_amd import hip
    L = hip.load_library()
    for n in (0, 1, 2, 255, 256, 4096, (1 << 24) - 1, 1 << 24, 1 << 33):
        assert L.agmv_hip_lz77_max_csize(n) == 4 * n


def test_calls_without_a_context_fail_loudly():
    from libagmv_amd import hip
    L = hip.load_library()
    buf = np.zeros(64, np.uint8)
    sizes = np.array([4], np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    s = sizes.ctypes.data_as(C.c_void_p)
    assert L.agmv_hip_lz77_frames(None, p, 16, s, 1, None, 0, p, 16, s) == -1
    assert b"NULL context" in L.agmv_hip_last_error()
    assert L.agmv_hip_lz77_frames_dev(None, p, 16, s, 1, None, p, 16, s, None) == -1
    assert L.agmv_hip_lz77_peek_dev(None, p, 16, s, 1, p, 16, p, None) == -1
    assert L.agmv_hip_lz77_reparsed_segments(None, None) == -1


def test_zero_closed_form_and_peek_restatement():
    """the helpers the GPU tests compare against: the closed form of an all-zero stream is the host stage's output, and
    the peek loop reads the byte behind a stream before the stream lands in the buffer"""
    for n, peek in ((0, 0), (1, 9), (2, 9), (256, 9), (257, 9), (258, 9), (66049, 3), (70000, 0x5A)):
        assert Z.same(Z.zeros_closed_form(n, peek), Z.host77(np.zeros(n, np.uint8), peek)), n
    head = Z.zeros_closed_form(300000)
    assert list(head[:12]) == [0, 0, 0, 0, 1, 0, 255, 0, 1, 1, 255, 0] and list(head[-4:]) == [255, 255, 0xDF, 0]
    persist = np.array([1, 2, 3, 4, 5, 6], np.uint8)
    rows = [np.array([10, 11, 12, 13, 14, 15, 16, 17], np.uint8), np.array([20, 21, 0, 0, 0, 0, 0, 0], np.uint8),
            np.array([30, 31, 32, 33, 34, 35, 36, 37], np.uint8), np.zeros(8, np.uint8)]
    peek = Z.prepare_batch_peek(rows, [4, 2, 8, 5], persist)
    assert list(peek) == [5, 12, 0, 35] and list(persist) == [0, 0, 0, 0, 0, 35]
