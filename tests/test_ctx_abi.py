"""Every entry point of include/agmv_hip.h that takes a context and returns int refuses a NULL context: a negative return,
no crash, and -- except for the two calls that have never set a text -- "NULL context" in agmv_hip_last_error().  No device is
touched: the refusal comes before the first HIP call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_TEXT = ("agmv_hip_enable_timing", "agmv_hip_ctx_device")     # return -1 and leave the error text alone


def _prototypes():
    """(return type, name, [(type, name)]) of every function the header declares"""
    hdr = open(os.path.join(ROOT, "include", "agmv_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    out = []
    for ret, name, args in re.findall(r"\b([A-Za-z_][\w \*]*?)\s*\b(agmv_hip_\w+)\s*\(([^)]*)\)\s*;", hdr):
        params = []
        for a in args.split(","):
            a = " ".join(a.split())
            if a and a != "void":
                m = re.match(r"(.*?)(\w+)(\[\d*\])?$", a)
                params.append((m.group(1).strip() + ("*" if m.group(3) else ""), m.group(2)))
        out.append((ret.strip(), name, params))
    return out


PROTOS = _prototypes()
CTX_INT = [(n, p) for r, n, p in PROTOS if r == "int" and p and p[0][0].replace(" ", "") == "agmv_hip_ctx*"]


@pytest.fixture(scope="module")
def lib():
    from libagmv_amd import abi, hip
    hip.load_library()                                           # builds nothing, raises when the library is missing
    return abi.bind(C.CDLL(hip.lib_path()), abi.HIP)             # a handle of its own


def test_the_header_parses():
    assert len(PROTOS) >= 81 and len(CTX_INT) >= 55
    names = [n for n, _ in CTX_INT]
    for n in ("agmv_hip_set_palette", "agmv_hip_decode_frames_dev", "agmv_hip_lzss_frames_dev", "agmv_hip_lz77_frames",
              "agmv_hip_lz_decode_commit_dev", "agmv_hip_scale_area_dev", "agmv_hip_palette_refine_dev",
              "agmv_hip_audio_expand_async", "agmv_hip_measure_frames_async", "agmv_hip_memset_async") + NO_TEXT:
        assert n in names, n


@pytest.mark.parametrize("name,params", CTX_INT, ids=[n for n, _ in CTX_INT])
def test_null_context_is_refused(lib, name, params):
    f = getattr(lib, name)
    bufs = [C.create_string_buffer(4096) for _ in params]
    args = [None]
    for (t, pname), b in zip(params[1:], bufs):
        args.append((None if pname == "stream" else C.cast(b, C.c_void_p)) if "*" in t else 0)
    assert f(*args) < 0
    if name not in NO_TEXT:
        assert b"NULL context" in lib.agmv_hip_last_error()
