"""What the scale stage (AGMV_EncodeFramesScaledDev, agmv_hip_scale_area_dev, encode_frames(size=, scale=)) does before it touches
the GPU: the header holds the definition and the libraries the symbols, the numpy statement of both rules (tests/scale_cases.py)
gives the answers worked out by hand, AGMV_EncodeFramesScaledDev refuses what it cannot encode before it reads the frames, opens a
device or creates a file, and libagmv_amd.seq refuses a misuse of size= / scale= before it loads the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hostlib as H
import memseq_cases as MC
import scale_cases as SC

ROOT = H.ROOT


def host():
    L = H.lib()
    return L


def test_header_and_libraries_hold_the_definition_and_the_functions():
    hdr = open(os.path.join(ROOT, "include", "agmv.h")).read()
    values = dict((k, int(v, 0)) for k, v in re.findall(r"\b(AGMV_SCALE_NEAREST|AGMV_SCALE_AREA)\s*=\s*(\w+)", hdr))
    assert values == {"AGMV_SCALE_NEAREST": 1, "AGMV_SCALE_AREA": 2}
    assert re.search(r"\bint\s+AGMV_EncodeFramesScaledDev\(", hdr)
    flat = re.sub(r"\s+", " ", hdr)
    for words in ("((2X + 1) * sw) div (2 * dw)", "((2Y + 1) * sh) div (2 * dh)",                    # NEAREST
                  "[i * dw, (i + 1) * dw)", "[X * sw, (X + 1) * sw)", "+ (sw * sh) div 2) div (sw * sh)",    # AREA
                  "sw * sh <= 2^24", "never in YUV", "4 * width * height * num_of_frames"):
        assert words in flat, words
    assert hasattr(host(), "AGMV_EncodeFramesScaledDev")
    G = C.CDLL(os.path.join(ROOT, "libagmv_amd", "libagmv_hip.so"))
    assert hasattr(G, "agmv_hip_scale_area_dev")
    assert re.search(r"\bint\s+agmv_hip_scale_area_dev\(", open(os.path.join(ROOT, "include", "agmv_hip.h")).read())
    import libagmv_amd
    assert callable(libagmv_amd.AgmvHip.scale_area_dev)
    assert libagmv_amd.SCALE == {"nearest": SC.NEAREST, "area": SC.AREA}


def chan(values):
    """a one-frame clip holding `values` (a 2-d list) in all three channels"""
    v = np.array(values, np.uint32)
    return (v << 16 | v << 8 | v)[None]


def test_known_answers_of_the_area_rule():
    assert SC.scale_area(chan([[1, 2], [3, 5]]), 1, 1).tolist() == chan([[3]]).tolist()               # (11 + 2) div 4
    assert SC.weights(3, 2).tolist() == [[2, 1, 0], [0, 1, 2]]
    # 3 -> 2 columns on one row: (2 * 10 + 1 * 40 + 1) div 3 = 20 and (1 * 40 + 2 * 100 + 1) div 3 = 80
    assert SC.scale_area(chan([[10, 40, 100]]), 2, 1).tolist() == chan([[20, 80]]).tolist()
    rng = np.random.default_rng(3)
    pix = rng.integers(0, 1 << 24, (2, 9, 12), dtype=np.uint32)
    assert (SC.scale_area(pix, 12, 9) == pix).all()                                                   # identity
    got = SC.scale_area(pix, 4, 3)                                                                    # factor 3: the rounded block mean
    for s in (16, 8, 0):
        c = ((pix >> s) & 255).astype(np.int64).reshape(2, 3, 3, 4, 3).sum(axis=(2, 4))
        assert (((got >> s) & 255) == (c + 4) // 9).all()
    assert (SC.scale_area(np.full((1, 7, 5), 0xFFFFFF, np.uint32), 3, 2) == 0xFFFFFF).all()
    # the channels do not leak into each other
    assert SC.scale_area(np.array([[[0xFF0000, 0x00FF00], [0x0000FF, 0x000000]]], np.uint32), 1, 1).tolist() == [[[0x404040]]]


@pytest.mark.parametrize("shape", SC.STARRED + SC.MORE, ids=[SC.shape_id(s) for s in SC.STARRED + SC.MORE])
def test_the_streamed_statement_equals_the_dense_one(shape):
    """scale_area_streamed (prefix sums) against scale_area (weight matrices), before a GPU test relies on the former"""
    sw, sh, dw, dh = shape
    rng = np.random.default_rng(sw * 31 + dw)
    for pix in (rng.integers(0, 1 << 32, (2, sh, sw), dtype=np.uint32), np.full((2, sh, sw), 0xFFFFFFFF, np.uint32)):
        got, exp = SC.scale_area_streamed(pix, dw, dh), SC.scale_area(pix, dw, dh)
        assert got.dtype == exp.dtype and got.shape == exp.shape and (got == exp).all(), np.argwhere(got != exp)[:4]
    assert (SC.scale_area_streamed(np.full((1, sh, sw), 0xFFFFFFFF, np.uint32), dw, dh) == 0xFFFFFF).all()


def test_the_streamed_statement_by_hand_and_the_wide_shapes():
    assert SC.scale_area_streamed(chan([[1, 2], [3, 5]]), 1, 1).tolist() == chan([[3]]).tolist()
    assert SC.scale_area_streamed(chan([[10, 40, 100]]), 2, 1).tolist() == chan([[20, 80]]).tolist()
    assert SC._area_axis(np.array([10, 40, 100], np.int64), 2).tolist() == [60, 240]                  # 2 * 10 + 1 * 40, 1 * 40 + 2 * 100
    for shape, small in SC.WIDE_U + [SC.WIDE_TILES, SC.WIDE_BOUND]:
        sw, sh, dw, dh = shape
        assert SC.area_small(shape) == small and dw <= sw and dh <= sh and sw * sh <= SC.AREA_MAX_SOURCE
    assert 65536 * 65536 == 1 << 32 and 65536 * 65535 == (1 << 32) - 65536 and SC.WIDE_BOUND[0][0] * SC.WIDE_BOUND[0][1] == SC.AREA_MAX_SOURCE
    # 65536 -> 65535 columns on one row: target X takes 65535 - X units of pixel X and X + 1 of pixel X + 1
    row = np.random.default_rng(6).integers(0, 256, 65536).astype(np.int64)
    X = np.arange(65535, dtype=np.int64)
    assert (SC._area_axis(row, 65535) == (65535 - X) * row[:-1] + (X + 1) * row[1:]).all()


def test_known_answers_of_the_nearest_rule():
    row = np.arange(4, dtype=np.uint32)[None, None, :] + 0x100
    assert SC.scale_nearest(row, 2, 1).tolist() == [[[0x101, 0x103]]]                                 # ((2X + 1) * 4) div 4 = 2X + 1
    assert SC.scale_nearest(row, 4, 1).tolist() == row.tolist()
    assert SC.scale_nearest(row, 8, 2).tolist() == [[[0x100, 0x100, 0x101, 0x101, 0x102, 0x102, 0x103, 0x103]] * 2]     # an upscale
    assert SC.scale_nearest(np.arange(3, dtype=np.uint32).reshape(1, 1, 3), 2, 1).tolist() == [[[0, 2]]]    # (1 * 3) div 4, (3 * 3) div 4
    assert SC.scale_nearest(np.full((1, 2, 2), 0xAB123456, np.uint32), 1, 1).tolist() == [[[0x123456]]]    # bits >= 24 are not pixels


def test_the_doubled_mixed_clip_scales_back_to_the_mixed_clip():
    """the input condition of the golden test in tests/test_gpu_scale_files.py"""
    clip = MC.mixed_clip()
    big = SC.doubled(clip)
    assert big.shape == (MC.MIXED_T, 256, 320)
    assert (SC.scale_area(big, MC.MIXED_W, MC.MIXED_H) == clip).all()
    assert (SC.scale_nearest(big, MC.MIXED_W, MC.MIXED_H) == clip).all()


# n, sw, sh, w, h, filter, fps, opt, quality, compression, schedule
OK = dict(n=8, sw=32, sh=32, w=16, h=16, filt=SC.AREA, fps=24, opt=3, quality=3, compression=1, schedule=2)
REFUSALS = [
    ("filter-0", dict(filt=0), -1), ("filter-3", dict(filt=3), -1),
    ("fmt-6", dict(fmt=6), -1), ("fmt-rgb24-with-a-yuv-flag", dict(fmt=2 | 0x100), -1), ("fmt-nv12-unknown-flag", dict(fmt=16 | 0x400), -1),
    ("opt-9", dict(opt=9), -1), ("quality-0", dict(quality=0), -1), ("compression-3", dict(compression=3), -1), ("schedule-4", dict(schedule=4), -1),
    ("3-frames-light-pdifs", dict(n=3), -2), ("1-frame-heavy-pdifs", dict(n=1, opt=1), -2), ("0-frames-full", dict(n=0, schedule=1), -2),
    ("target-18x16", dict(w=18), -3), ("target-16x18", dict(h=18), -3), ("target-0x16", dict(w=0), -3), ("target-16x0", dict(h=0), -3),
    ("source-0x32", dict(sw=0), -3), ("source-32x0", dict(sh=0), -3),
    ("opt-gba-i", dict(opt=5), -3), ("opt-gba-iii", dict(opt=7), -3), ("opt-nds", dict(opt=8), -3),
    ("area-upscale-in-x", dict(sw=16, sh=16, w=32, h=16), -3), ("area-upscale-in-y", dict(sw=16, sh=16, w=16, h=32), -3),
    ("area-source-4097x4096", dict(sw=4097, sh=4096), -3),
    # the same two are no refusal for NEAREST: with too few frames the call gets as far as -2 (the sizes are looked at before the count)
    ("nearest-upscale", dict(filt=SC.NEAREST, sw=16, sh=16, w=32, h=16, n=3), -2),
    ("nearest-source-4097x4096", dict(filt=SC.NEAREST, sw=4097, sh=4096, n=3), -2),
    ("area-upscale-3-frames", dict(sw=16, sh=16, w=32, h=16, n=3), -3), ("area-source-4097x4096-3-frames", dict(sw=4097, sh=4096, n=3), -3),
    ("area-source-4096x4096-3-frames", dict(sw=4096, sh=4096, n=3), -2),                      # 2^24 source pixels are allowed
    ("source-not-a-multiple-of-4-3-frames", dict(sw=50, sh=38, n=3), -2),
]


@pytest.mark.parametrize("name,change,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_unencodable_arguments_are_refused_before_the_frames_are_read(name, change, code, tmp_path):
    """(the pointer is never read, no device is opened and no file is created: every one of these returns first)"""
    L = host()
    a = dict(dict(OK, fmt=2), **change)
    out = str(tmp_path / "x.agmv").encode()
    args = [a["fmt"], a["n"], a["sw"], a["sh"], a["w"], a["h"], a["filt"], a["fps"], a["opt"], a["quality"], a["compression"], a["schedule"]]
    for fmt in ([a["fmt"]] if "fmt" in change else SC.LAYOUTS + SC.YUV_709F):
        args[0] = fmt
        assert L.AGMV_EncodeFramesScaledDev(out, C.c_void_p(4096), *args) == code, fmt
    assert L.AGMV_EncodeFramesScaledDev(out, None, *args) == -1                              # NULL frames, whatever else
    assert L.AGMV_EncodeFramesScaledDev(None, C.c_void_p(4096), *args) == -1
    assert not os.listdir(tmp_path)


def test_seq_refuses_a_misuse_of_size_and_scale_before_the_library_is_loaded(tmp_path, monkeypatch):
    import torch
    import libagmv_amd
    from libagmv_amd import seq

    def reached():
        raise AssertionError("the library was called")
    monkeypatch.setattr(seq, "load_library", reached)
    out = str(tmp_path / "x.agmv")
    rgb = torch.zeros((8, 38, 50, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="size="):
        libagmv_amd.encode_frames(out, rgb, scale="nearest")                                # a filter without a target
    for name in ("bilinear", "AREA", None, 2):
        with pytest.raises(ValueError, match="scale"):
            libagmv_amd.encode_frames(out, rgb, size=(16, 24), scale=name)
        with pytest.raises(ValueError, match="scale"):
            libagmv_amd.encode_frames(out, rgb, scale=name)
    for size in ((16,), (16, 24, 3), (0, 24), (16, -4), (16.0, 24), "16x24", 16, (True, 24)):
        with pytest.raises(ValueError, match="size"):
            libagmv_amd.encode_frames(out, rgb, size=size)
    with pytest.raises(ValueError, match="yuv="):
        libagmv_amd.encode_frames(out, rgb, fmt="rgb24", yuv="bt709", size=(16, 24))        # the older refusals still come first
    assert not os.listdir(tmp_path)
