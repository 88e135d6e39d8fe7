"""ctypes view of libagmv_amd/libagmv.so (the libagmv-compatible host library) for tests."""
import ctypes as C
import os

import numpy as np

from libagmv_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "libagmv_amd", "libagmv.so")

u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")

# exports of libagmv.so that exist for the tests alone and stand in no public header
TEST_ONLY = {
    "agmv_lzss_mem": (C.c_ulong, (u8p, C.c_size_t, u8p)),
    "agmv_lz77_mem": (C.c_ulong, (u8p, C.c_size_t, u8p)),
    "agmv_lz_decode_mem": (C.c_ulong, (C.c_int, u8p, C.c_size_t, C.c_ulong, C.c_ulong, u8p, C.c_size_t, C.POINTER(C.c_size_t))),
    "agmv_bmp_save": (C.c_int, (C.c_char_p, u32p, C.c_uint32, C.c_uint32)),
    "agmv_bmp_load": (C.c_int, (C.c_char_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))),
    "agmv_source_index": (C.POINTER(C.c_uint32), (C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32)),
}
# pointer slots of abi.AGMV that the tests fill with numpy arrays (the header's u32 has 8 bytes)
ARRAYS = {"AGMV_SetICP0": {1: u64p}, "AGMV_SetICP1": {1: u64p}, "AGMV_EncodeFrame": {2: u64p}, "AGMV_BuildPalette": {0: u32p, 3: u64p, 4: u64p},
          "AGMV_SynthFrame": {0: u32p}, "AGMV_BubbleSort": {0: u64p, 1: u64p}, "AGMV_FindNearestColor": {0: u64p},
          "AGMV_FindNearestEntry": {0: u64p, 1: u64p}, "AGMV_CompareFrameSimilarity": {0: u64p, 1: u64p}}

_lib = None


def bind(L, missing_ok=False):
    """a loaded libagmv.so (or, with missing_ok, the compiled reference, which shares the API) bound from the tables"""
    abi.bind(L, abi.AGMV, missing_ok)
    abi.bind(L, TEST_ONLY, missing_ok)
    for name, slots in ARRAYS.items():
        f = getattr(L, name, None)
        if f is not None:
            args = list(f.argtypes)
            for i, t in slots.items():
                assert args[i] is C.c_void_p, (name, i)
                args[i] = t
            f.argtypes = args
    return L


def lib():
    global _lib
    if _lib is None:
        from libagmv_amd import build
        build.build()
        _lib = bind(C.CDLL(SO))
    return _lib


def lzss(data):
    data = np.ascontiguousarray(data, np.uint8)
    out = np.zeros(2 * len(data) + 64, np.uint8)
    cs = lib().agmv_lzss_mem(np.concatenate([data, np.zeros(8, np.uint8)]), len(data), out)
    return out[:cs].copy(), int(cs)


def lz77(data, tail_byte=0):
    data = np.ascontiguousarray(data, np.uint8)
    out = np.zeros(4 * len(data) + 64, np.uint8)
    buf = np.concatenate([data, np.full(8, tail_byte, np.uint8)])
    cs = lib().agmv_lz77_mem(buf, len(data), out)
    return out[:cs].copy(), int(cs)


def write_bmp(path, frame):
    frame = np.ascontiguousarray(frame, np.uint32)
    h, w = frame.shape
    assert lib().agmv_bmp_save(path.encode(), frame.reshape(-1), w, h) == 0
