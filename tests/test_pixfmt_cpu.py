"""What the pixel formats of the memory sequences do before they touch the GPU: the enum and the entry points exist in the
headers and the libraries, agmv_hip_pixfmt_frame_bytes answers without a device, AGMV_EncodeFramesFmtDev refuses what cannot be
encoded before it reads the frames or creates a file, AGMV_DecodeFramesFmtDev reads a header for every format, and
libagmv_amd.encode_frames refuses a tensor whose format it cannot tell before it calls the library."""
import ctypes as C
import os
import re

import pytest

import hostlib as H
from libagmv_amd import abi
import pixfmt_cases as P

ROOT = H.ROOT
HIP_FUNCS = ["agmv_hip_pixfmt_frame_bytes", "agmv_hip_pixels_to_xrgb_dev", "agmv_hip_pixels_from_xrgb_dev", "agmv_hip_gather_fmt_dev",
             "agmv_hip_histogram_fmt_dev", "agmv_hip_similarity_fmt_dev"]
HOST_FUNCS = ["AGMV_EncodeFramesFmtDev", "AGMV_DecodeFramesFmtDev"]


def host():
    L = H.lib()
    from libagmv_amd.seq import AGMV_INFO
    return L, AGMV_INFO


def hip_lib():
    H.lib()
    return abi.bind(C.CDLL(os.path.join(ROOT, "libagmv_amd", "libagmv_hip.so")), abi.HIP)


def test_headers_declare_the_enum_and_the_functions():
    hdr = open(os.path.join(ROOT, "include", "agmv.h")).read()
    enum = re.search(r"typedef enum AGMV_PIXFMT \{(.*?)\} AGMV_PIXFMT;", hdr, re.S)
    assert enum
    values = dict((k, int(v)) for k, v in re.findall(r"(AGMV_PIXFMT_\w+)\s*=\s*(\d+)", enum.group(1)))
    assert values == {"AGMV_PIXFMT_XRGB32": 1, "AGMV_PIXFMT_RGB24": 2, "AGMV_PIXFMT_BGR24": 3, "AGMV_PIXFMT_RGBA32": 4, "AGMV_PIXFMT_RGB8P": 5}
    for f in HOST_FUNCS:
        assert re.search(r"\bint %s\(" % f, hdr), f
    hip_hdr = open(os.path.join(ROOT, "include", "agmv_hip.h")).read()
    assert re.search(r"\bsize_t agmv_hip_pixfmt_frame_bytes\(int fmt, size_t n_pixels\);", hip_hdr)
    for f in HIP_FUNCS[1:]:
        assert re.search(r"\bint %s\(agmv_hip_ctx\* ctx, int fmt," % f, hip_hdr), f


def test_both_libraries_export_the_functions():
    L, G = H.lib(), hip_lib()
    for f in HIP_FUNCS:
        assert hasattr(G, f), f
    for f in HOST_FUNCS:
        assert hasattr(L, f), f
    import libagmv_amd
    assert libagmv_amd.PIXFMT == {"xrgb32": 1, "rgb24": 2, "bgr24": 3, "rgba32": 4, "rgb8p": 5}
    for m in ("pixels_to_xrgb_dev", "pixels_from_xrgb_dev", "gather_fmt_dev", "histogram_fmt_dev", "similarity_fmt_dev"):
        assert callable(getattr(libagmv_amd.AgmvHip, m)), m


def test_frame_bytes_needs_no_device():
    G = hip_lib()
    for n in (0, 1, 7, 160 * 128, 1920 * 1080, (1 << 33) + 5):
        assert [G.agmv_hip_pixfmt_frame_bytes(f, n) for f in range(0, 7)] == [0, 4 * n, 3 * n, 3 * n, 4 * n, 3 * n, 0], n
    assert [P.frame_bytes(f, 10) for f in (1, 2, 3, 4, 5)] == [G.agmv_hip_pixfmt_frame_bytes(f, 10) for f in (1, 2, 3, 4, 5)]


def test_unencodable_arguments_are_refused_before_the_frames_are_read(tmp_path):
    """(the pointer is never read and no device is opened: every one of these returns first)"""
    L, _ = host()
    out = str(tmp_path / "x.agmv").encode()
    d = C.c_void_p(4096)
    ok = [8, 16, 16, 24, 3, 3, 1, 2]                              # n, w, h, fps, opt, quality, compression, schedule
    for fmt in (0, 6, -1, 255):
        assert L.AGMV_EncodeFramesFmtDev(out, d, fmt, *ok) == -1, fmt
    for fmt in (1, 2, 3, 4, 5):
        assert L.AGMV_EncodeFramesFmtDev(out, None, fmt, *ok) < 0, fmt
        assert L.AGMV_EncodeFramesFmtDev(None, d, fmt, *ok) < 0, fmt
        assert L.AGMV_EncodeFramesFmtDev(out, d, fmt, 8, 18, 16, 24, 3, 3, 1, 2) < 0, fmt        # 18 x 16, an opt that does not scale
        assert L.AGMV_EncodeFramesFmtDev(out, d, fmt, 3, 16, 16, 24, 3, 3, 1, 2) < 0, fmt        # fewer frames than the first group reads
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("fmt", [1, 2, 3, 4, 5])
def test_null_destination_reads_the_header_for_every_format(fmt, golden, golden_dir):
    L, AGMV_INFO = host()
    g = golden["agmv_splash"]
    info = AGMV_INFO()
    path = os.path.join(golden_dir, "agmv_splash.agmv").encode()
    assert L.AGMV_DecodeFramesFmtDev(path, None, fmt, 0, C.byref(info)) == 0
    assert (info.width, info.height, info.number_of_frames, info.version) == (g["w"], g["h"], g["n"], g["version"])


def test_decode_refuses_an_unknown_format(golden_dir):
    L, AGMV_INFO = host()
    info = AGMV_INFO()
    path = os.path.join(golden_dir, "agmv_splash.agmv").encode()
    for fmt in (0, 6):
        assert L.AGMV_DecodeFramesFmtDev(path, None, fmt, 0, C.byref(info)) == -1
    assert info.width == 0 and info.number_of_frames == 0


def test_encode_frames_refuses_tensors_whose_format_it_cannot_tell(tmp_path, monkeypatch):
    """before any library call: load_library is made to fail the test if it is reached"""
    import torch
    import libagmv_amd
    from libagmv_amd import seq

    def reached():
        raise AssertionError("the library was called")
    monkeypatch.setattr(seq, "load_library", reached)
    out = str(tmp_path / "x.agmv")
    with pytest.raises(ValueError, match="fmt"):
        libagmv_amd.encode_frames(out, torch.zeros((2, 16, 16), dtype=torch.float32))
    with pytest.raises(ValueError, match="fmt"):
        libagmv_amd.encode_frames(out, torch.zeros((2, 3, 8, 3), dtype=torch.uint8))        # rgb24 of 3 x 8 or planes of 8 x 3
    with pytest.raises(ValueError, match="fmt"):
        libagmv_amd.encode_frames(out, torch.zeros((2, 16, 16, 3), dtype=torch.uint8).transpose(1, 2))     # not contiguous
    with pytest.raises(ValueError, match="fmt"):
        libagmv_amd.encode_frames(out, torch.zeros((2, 16, 16, 3), dtype=torch.uint8), fmt="rgb8p")
    with pytest.raises(ValueError, match="fmt"):
        libagmv_amd.encode_frames(out, torch.zeros((2, 16, 16, 3), dtype=torch.uint8), fmt="yuv420")
    assert not os.listdir(tmp_path)
