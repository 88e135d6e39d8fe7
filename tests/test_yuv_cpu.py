"""What the YUV 4:2:0 formats (AGMV_PIXFMT_NV12 / AGMV_PIXFMT_I420, include/agmv.h) do before they touch the GPU: the frame size
answers without a device, the numpy statement of the definition (tests/yuv_cases.py) gives the known answers,
AGMV_EncodeFramesFmtDev refuses unknown flags and what cannot be encoded before it reads the frames or creates a file,
AGMV_DecodeFramesFmtDev reads a header for a format with flags, and libagmv_amd.seq refuses yuv= / full_range= on an RGB layout
before it loads the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hostlib as H
from libagmv_amd import abi
import yuv_cases as Y

ROOT = H.ROOT
HIP_FUNCS = ["agmv_hip_yuv_frame_bytes", "agmv_hip_yuv_to_xrgb_dev", "agmv_hip_yuv_from_xrgb_dev", "agmv_hip_yuv_gather_dev",
             "agmv_hip_yuv_histogram_dev", "agmv_hip_yuv_similarity_dev"]


def host():
    L = H.lib()
    from libagmv_amd.seq import AGMV_INFO
    return L, AGMV_INFO


def hip_lib():
    H.lib()
    return abi.bind(C.CDLL(os.path.join(ROOT, "libagmv_amd", "libagmv_hip.so")), abi.HIP)


def test_headers_and_libraries_hold_the_formats_and_the_functions():
    hdr = open(os.path.join(ROOT, "include", "agmv.h")).read()
    values = dict((k, int(v, 0)) for k, v in re.findall(r"\b(AGMV_PIXFMT_NV12|AGMV_PIXFMT_I420|AGMV_YUV_BT709|AGMV_YUV_FULL_RANGE)\s*=\s*(\w+)", hdr))
    assert values == {"AGMV_PIXFMT_NV12": 16, "AGMV_PIXFMT_I420": 17, "AGMV_YUV_BT709": 0x100, "AGMV_YUV_FULL_RANGE": 0x200}
    for row in list(Y.READ.values()) + [(a + (yo,) + b + c) for a, yo, b, c in Y.WRITE.values()]:
        assert re.search(r"\s+".join(str(v) for v in row), hdr), row           # the tables of the definition are in the header
    hip_hdr = open(os.path.join(ROOT, "include", "agmv_hip.h")).read()
    G = hip_lib()
    for f in HIP_FUNCS:
        assert re.search(r"\b%s\(" % f, hip_hdr) and hasattr(G, f), f
    import libagmv_amd
    assert libagmv_amd.YUVFMT == {"nv12": 16, "i420": 17}
    assert libagmv_amd.PIXFMT == {"xrgb32": 1, "rgb24": 2, "bgr24": 3, "rgba32": 4, "rgb8p": 5}
    for m in ("yuv_to_xrgb_dev", "yuv_from_xrgb_dev", "yuv_gather_dev", "yuv_histogram_dev", "yuv_similarity_dev"):
        assert callable(getattr(libagmv_amd.AgmvHip, m)), m


def test_frame_bytes_needs_no_device():
    G = hip_lib()
    exp = {(1, 1): 3, (2, 2): 6, (3, 3): 17, (1920, 1080): 3110400, (121, 81): 14803}        # w * h + 2 * cw * ch, by hand
    for (w, h), b in exp.items():
        for fmt in Y.LAYOUTS:
            for flags in Y.FLAGS:
                assert G.agmv_hip_yuv_frame_bytes(fmt | flags, w, h) == b == Y.frame_bytes(fmt | flags, w, h), (fmt, flags, w, h)
        for fmt in (0, 1, 2, 5, 6, 15, 18, 255, 16 | 0x400, 17 | 0x1000, 2 | 0x100):
            assert G.agmv_hip_yuv_frame_bytes(fmt, w, h) == 0 == Y.frame_bytes(fmt, w, h), fmt
    for fmt in (16, 17, 16 | 0x100):
        assert G.agmv_hip_pixfmt_frame_bytes(fmt, 100) == 0, fmt          # the function of the pixel-count layouts does not know them


def one(flags, y, u, v):
    return int(Y.yuv_to_rgb(flags, np.array([y]), np.array([u]), np.array([v]))[0])


def test_known_answers():
    assert one(0, 16, 128, 128) == 0x000000
    assert one(0, 235, 128, 128) == 0xFFFFFF
    assert one(0, 81, 90, 240) == 0xFF0000
    red = np.full((1, 2, 2), 0xFF0000, np.uint32)
    for fmt in Y.LAYOUTS:
        assert list(Y.from_packed(fmt | Y.FULL_RANGE, red, 2, 2)[0]) == [77] * 4 + [85, 255]
    # the layouts, by hand: 2 x 2 pixels, Y 1..4, U 5, V 6 and 3 x 1 pixels with two chroma samples
    assert Y.planes(Y.NV12, np.array([[1, 2, 3, 4, 5, 6]], np.uint8), 2, 2)[1][0, 0, 0] == 5
    raw = np.array([[10, 20, 30, 1, 2, 3, 4]], np.uint8)
    _, u, v = Y.planes(Y.NV12, raw, 3, 1)
    assert (list(u[0, 0]), list(v[0, 0])) == ([1, 3], [2, 4])
    _, u, v = Y.planes(Y.I420, raw, 3, 1)
    assert (list(u[0, 0]), list(v[0, 0])) == ([1, 2], [3, 4])


@pytest.mark.parametrize("flags", Y.FLAGS, ids=[Y.FLAG_NAMES[f] for f in Y.FLAGS])
def test_greys_and_random_colours_round_trip(flags):
    """greys come back within 1 with U = V = 128; random colours (flat 2 x 2 blocks, so the mean is the colour) within 3 per channel"""
    g = np.arange(256, dtype=np.uint32)
    grey = (g << 16 | g << 8 | g).reshape(1, 16, 16)
    rng = np.random.default_rng(flags + 1)
    flat = np.repeat(np.repeat(rng.integers(0, 1 << 24, (1, 32, 32), dtype=np.uint32), 2, axis=1), 2, axis=2)
    for fmt in Y.LAYOUTS:
        raw = Y.from_packed(fmt | flags, grey, 16, 16)
        _, u, v = Y.planes(fmt, raw, 16, 16)
        assert (u == 128).all() and (v == 128).all()
        back = Y.to_packed(fmt | flags, raw, 16, 16)
        assert np.abs((back & 255).astype(int) - g.reshape(1, 16, 16)).max() <= 1
        assert ((back >> 16) == (back & 255)).all() and (((back >> 8) & 255) == (back & 255)).all()
        back = Y.to_packed(fmt | flags, Y.from_packed(fmt | flags, flat, 64, 64), 64, 64)
        for s in (16, 8, 0):
            assert np.abs(((back >> s) & 255).astype(int) - ((flat >> s) & 255).astype(int)).max() <= 3


def test_odd_edges_average_the_pixels_that_exist():
    """3 x 3: the blocks have 4, 2, 2 and 1 pixels; (sum + (cnt >> 1)) / cnt by hand on the blue channel under BT.601 full range"""
    pix = np.array([[[1, 2, 4], [3, 5, 7], [8, 11, 101]]], np.uint32)
    raw = Y.from_packed(Y.I420 | Y.FULL_RANGE, pix, 3, 3)
    means = [(1 + 2 + 3 + 5 + 2) // 4, (4 + 7 + 1) // 2, (8 + 11 + 1) // 2, 101]
    assert list(raw[0, 9:13]) == [min(255, ((128 * m + 128) >> 8) + 128) for m in means]
    assert list(raw[0, 13:17]) == [((-21 * m + 128) >> 8) + 128 for m in means]


def test_unencodable_arguments_are_refused_before_the_frames_are_read(tmp_path):
    """(the pointer is never read and no device is opened: every one of these returns first)"""
    L, _ = host()
    out = str(tmp_path / "x.agmv").encode()
    d = C.c_void_p(4096)
    ok = [8, 16, 16, 24, 3, 3, 1, 2]                              # n, w, h, fps, opt, quality, compression, schedule
    for fmt in (2 | 0x100, 16 | 0x400, 18):
        assert L.AGMV_EncodeFramesFmtDev(out, d, fmt, *ok) == -1, fmt
    for fmt in (1 | 0x200, 5 | 0x300, 17 | 0x800, 16 | 0x10000, 15, 0x100, 0x411):
        assert L.AGMV_EncodeFramesFmtDev(out, d, fmt, *ok) == -1, fmt
    for base in Y.LAYOUTS:
        for fmt in (base, base | 0x100, base | 0x200, base | 0x300):
            # the codes of a known format: an unknown one (every YUV value, before these formats existed) gives -1 for all three
            assert L.AGMV_EncodeFramesFmtDev(out, None, fmt, *ok) == -1, fmt
            assert L.AGMV_EncodeFramesFmtDev(out, d, fmt, 8, 18, 16, 24, 3, 3, 1, 2) == -3, fmt      # 18 x 16, an opt that does not scale
            assert L.AGMV_EncodeFramesFmtDev(out, d, fmt, 3, 16, 16, 24, 3, 3, 1, 2) == -2, fmt      # fewer frames than the first group reads
    assert not os.listdir(tmp_path)


def test_null_destination_reads_the_header_for_a_format_with_flags(golden, golden_dir):
    L, AGMV_INFO = host()
    g = golden["agmv_splash"]
    path = os.path.join(golden_dir, "agmv_splash.agmv").encode()
    for fmt in (17 | 0x300, 16, 16 | 0x100):
        info = AGMV_INFO()
        assert L.AGMV_DecodeFramesFmtDev(path, None, fmt, 0, C.byref(info)) == 0
        assert (info.width, info.height, info.number_of_frames, info.version) == (g["w"], g["h"], g["n"], g["version"])
    info = AGMV_INFO()
    for fmt in (18, 16 | 0x400, 2 | 0x100):
        assert L.AGMV_DecodeFramesFmtDev(path, None, fmt, 0, C.byref(info)) == -1
    assert info.width == 0 and info.number_of_frames == 0


def test_seq_refuses_yuv_options_on_rgb_layouts_before_the_library_is_loaded(tmp_path, monkeypatch):
    import torch
    import libagmv_amd
    from libagmv_amd import seq

    def reached():
        raise AssertionError("the library was called")
    monkeypatch.setattr(seq, "load_library", reached)
    out = str(tmp_path / "x.agmv")
    rgb = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="yuv="):
        libagmv_amd.encode_frames(out, rgb, fmt="rgb24", yuv="bt709")
    with pytest.raises(ValueError, match="full_range="):
        libagmv_amd.encode_frames(out, rgb, fmt="rgb24", full_range=True)
    with pytest.raises(ValueError, match="yuv="):
        libagmv_amd.encode_frames(out, rgb, yuv="bt601")                               # inferred rgb24
    with pytest.raises(ValueError, match="fmt"):
        libagmv_amd.encode_frames(out, torch.zeros((2, 24, 16), dtype=torch.uint8))    # a YUV layout is never inferred
    with pytest.raises(ValueError, match="fmt"):
        libagmv_amd.encode_frames(out, torch.zeros((2, 25, 16), dtype=torch.uint8), fmt="nv12")       # rows no multiple of 3
    with pytest.raises(ValueError, match="fmt"):
        libagmv_amd.encode_frames(out, torch.zeros((2, 24, 15), dtype=torch.uint8), fmt="i420")       # odd width
    with pytest.raises(ValueError, match="yuv"):
        libagmv_amd.encode_frames(out, torch.zeros((2, 24, 16), dtype=torch.uint8), fmt="nv12", yuv="bt2020")
    with pytest.raises(ValueError, match="yuv="):
        libagmv_amd.decode_frames(out, fmt="rgb24", yuv="bt709")
    with pytest.raises(ValueError, match="full_range="):
        libagmv_amd.decode_frames(out, full_range=True)
    assert not os.listdir(tmp_path)
