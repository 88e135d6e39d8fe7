"""What the decoder's scaling sink (AGMV_DecodeFramesScaledDev, agmv_hip_scale_frames_async, decode_frames(size=, scale=)) does before
it touches the GPU: the header holds the bilinear rule and the libraries the symbols, the numpy statement of the rule
(tests/upscale_cases.py) gives the answers worked out by hand and has the properties the header states, AGMV_DecodeFramesScaledDev
refuses what it cannot deliver in the header's order before it opens a device, and libagmv_amd.seq refuses a misuse of size= /
scale= before it loads the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hostlib as H
import scale_cases as SC
import upscale_cases as U

ROOT = H.ROOT
SPLASH = os.path.join(ROOT, "tests", "golden", "agmv_splash.agmv")         # 119 frames of 320 x 240


def host():
    from libagmv_amd.seq import AGMV_INFO
    L = H.lib()
    return L


def chan(values):
    """a one-frame clip holding `values` (a 2-d list) in all three channels"""
    v = np.array(values, np.uint32)
    return (v << 16 | v << 8 | v)[None]


def test_header_and_libraries_hold_the_definition_and_the_functions():
    hdr = open(os.path.join(ROOT, "include", "agmv.h")).read()
    values = dict((k, int(v, 0)) for k, v in re.findall(r"\b(AGMV_SCALE_\w+)\s*=\s*(\w+)", hdr))
    assert values == {"AGMV_SCALE_NEAREST": 1, "AGMV_SCALE_AREA": 2, "AGMV_SCALE_BILINEAR": 3}
    assert re.search(r"\bint\s+AGMV_DecodeFramesScaledDev\(", hdr)
    flat = re.sub(r"\s+", " ", hdr)
    for words in ("p = (2X + 1) * s - d", "i0 = p div 2d", "r = p mod 2d", "f = (256 * r + d) div 2d", "i1 = min(i0 + 1, s - 1)",
                  "((256 - fy) * ((256 - fx) * S(x0, y0) + fx * S(x1, y0))", "+ fy * ((256 - fx) * S(x0, y1) + fx * S(x1, y1)) + 32768) >> 16",
                  "255 * 65536 + 32768 < 2^32", "is the identity", "a flat frame stays flat", "between the smallest and the largest of its four taps",
                  "interpolated in RGB, never in YUV", "aliases"):
        assert words in flat, words
    assert hasattr(host(), "AGMV_DecodeFramesScaledDev")
    G = C.CDLL(os.path.join(ROOT, "libagmv_amd", "libagmv_hip.so"))
    assert hasattr(G, "agmv_hip_scale_frames_async")
    assert re.search(r"\bint\s+agmv_hip_scale_frames_async\(", open(os.path.join(ROOT, "include", "agmv_hip.h")).read())
    import libagmv_amd
    assert callable(libagmv_amd.AgmvHip.scale_frames_async)
    assert libagmv_amd.DECODE_SCALE == {"nearest": 1, "area": 2, "bilinear": 3}
    assert libagmv_amd.SCALE == {"nearest": 1, "area": 2}                                          # the encoder's filters stay two


def test_known_answers_of_the_bilinear_rule():
    assert U.scale_bilinear(chan([[0, 255]]), 4, 1).tolist() == chan([[0, 64, 191, 255]]).tolist()
    assert U.scale_bilinear(chan([[0, 255]]), 8, 1).tolist() == chan([[0, 0, 32, 96, 159, 223, 255, 255]]).tolist()
    assert U.scale_bilinear(chan([[10], [200]]), 1, 3).tolist() == chan([[10], [105], [200]]).tolist()
    assert U.scale_bilinear(np.full((1, 2, 2), 0xAB123456, np.uint32), 3, 3).tolist() == [[[0x123456] * 3] * 3]      # bits >= 24 are not pixels
    # the channels do not leak into each other: red to the left, blue to the right
    assert U.scale_bilinear(np.array([[[0xFF0000, 0x0000FF]]], np.uint32), 4, 1).tolist() == [[[0xFF0000, 0xBF0040, 0x4000BF, 0x0000FF]]]


def test_the_taps():
    i0, i1, f = U.taps(2, 4)                         # p = -2, 2, 6, 10 over 2d = 8
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1] and f.tolist() == [0, 64, 192, 64]
    i0, i1, f = U.taps(7, 7)
    assert i0.tolist() == list(range(7)) and not f.any()                                           # the same size: every weight on one pixel
    i0, i1, f = U.taps(1, 16)
    assert not i0.any() and not i1.any()                                                           # one source pixel: every tap clamped
    assert U.taps(5, 512)[2].max() == 256                                                          # f = 256 is reached ...
    assert U.taps(320, 1920)[2].max() < 256 and U.taps(240, 1080)[2].max() < 256                   # ... but never at the flagship ratio
    for s, d in ((5, 512), (3, 4), (12, 8), (320, 1920), (1080, 240), (7, 3)):
        i0, i1, f = U.taps(s, d)
        assert 0 <= f.min() and f.max() <= 256 and i0.min() >= 0 and i1.max() <= s - 1 and ((i1 == i0 + 1) | (i1 == s - 1)).all()


def test_the_32_bit_predicate_on_its_boundaries():
    """U.up_small restates the rule under which the kernels divide in 32 bits; the four boundary shapes lie where the GPU tests say"""
    assert (2 * 32768 - 1) * 65536 + 32768 == (1 << 32) - 32768 and U.up_small(65536, 32768)
    assert (2 * 32768 - 1) * 65537 + 32768 == (1 << 32) + 32767 and not U.up_small(65537, 32768)
    assert 513 * 8372240 == (1 << 32) - 8176 and U.up_small(3, 8372240)
    assert 513 * 8372256 == (1 << 32) + 32 and not U.up_small(3, 8372256)
    assert 8372240 % 16 == 0 and 8372256 - 8372240 == 16                                           # neighbours among the widths the band kernel takes
    assert [U.axes_small(s) for s, _ in U.BOUNDARY_P + U.BOUNDARY_F] == [(True, True), (False, True), (True, True), (False, True)]
    # the terms the 32-bit form computes, at their largest, on the small side of both pairs
    for s, d in ((65536, 32768), (3, 8372240)):
        p = (2 * np.arange(d, dtype=np.int64) + 1) * s + d
        assert int(p.max()) < 1 << 32 and int((256 * (p % (2 * d)) + d).max()) < 1 << 32
    for s, d in ((1, 1), (320, 1920), (4096, 4096), (1 << 28, 1), (1, 1 << 22)):
        assert U.up_small(s, d)
    assert not U.up_small(1 << 28, 9) and not U.up_small(1, 1 << 24)


@pytest.mark.parametrize("shape,small", U.NEW_SHAPES, ids=[U.shape_id(s) for s, _ in U.NEW_SHAPES])
def test_the_taps_of_the_wide_and_degenerate_shapes(shape, small):
    """every shape is on the side of the predicate it was chosen for, and its taps stay inside the source with f <= 256"""
    assert U.axes_small(shape) == small
    sw, sh, dw, dh = shape
    for s, d in ((sw, dw), (sh, dh)):
        i0, i1, f = U.taps(s, d)
        assert len(i0) == d and i0.min() >= 0 and i1.max() <= s - 1 and (i0 <= i1).all() and ((i1 == i0 + 1) | (i1 == s - 1)).all()
        assert 0 <= f.min() and f.max() <= 256
        near = ((2 * np.arange(d, dtype=np.int64) + 1) * s) // (2 * d)
        assert near.min() >= 0 and near.max() <= s - 1


@pytest.mark.parametrize("shape", U.SHAPES, ids=[U.shape_id(s) for s in U.SHAPES])
def test_properties_on_random_frames(shape):
    sw, sh, dw, dh = shape
    rng = np.random.default_rng(sw * 1000 + dw)
    pix = rng.integers(0, 1 << 24, (2, sh, sw), dtype=np.uint32)
    assert (U.scale_bilinear(pix, sw, sh) == pix).all()                                            # identity
    assert (U.scale_bilinear(np.full((1, sh, sw), 0x7F01FE, np.uint32), dw, dh) == 0x7F01FE).all()  # flat stays flat
    sums = []
    got = U.scale_bilinear(np.concatenate([pix, np.full((1, sh, sw), 0xFFFFFF, np.uint32)]), dw, dh, sums)
    assert max(sums) < 1 << 32 and max(sums) == 255 * 65536 + 32768                                # every sum fits 32 bits
    lo, hi = U.tap_bounds(pix, dw, dh)
    for s in (16, 8, 0):
        c = (got[:2] >> s) & 255
        assert (c >= (lo >> s) & 255).all() and (c <= (hi >> s) & 255).all()
    if (sw, sh, dw, dh) == (5, 3, 512, 4):
        assert U.taps(5, 512)[2].max() == 256


# fmt, w, h, filter on the splash file (320 x 240) with a pointer that is never read
REFUSALS = [
    ("fmt-6", dict(fmt=6), -1), ("fmt-rgb24-with-a-yuv-flag", dict(fmt=2 | 0x100), -1), ("fmt-nv12-unknown-flag", dict(fmt=16 | 0x400), -1),
    ("filter-0", dict(filt=0), -1), ("filter-4", dict(filt=4), -1),
    ("unknown-filter-before-zero-size", dict(filt=4, w=0), -1), ("unknown-format-before-missing-file", dict(fmt=0, path="missing"), -1),
    ("target-0x480", dict(w=0), -4), ("target-640x0", dict(h=0), -4), ("target-above-2^28", dict(w=1 << 14, h=(1 << 14) + 1), -4),
    ("target-width-2^32", dict(w=1 << 32, h=1), -4),
    ("zero-size-before-missing-file", dict(w=0, path="missing"), -4),
    ("missing-file", dict(path="missing"), -2),                                                    # FILE_NOT_FOUND_ERR, as AGMV_DecodeFramesFmtDev
    ("missing-file-before-area-upscale", dict(path="missing", filt=U.AREA), -2),
    ("area-upscale-in-x", dict(filt=U.AREA, w=321, h=240), -4), ("area-upscale-in-y", dict(filt=U.AREA, w=320, h=241), -4),
    ("area-upscale", dict(filt=U.AREA), -4),
]


@pytest.mark.parametrize("name,change,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_undeliverable_arguments_are_refused_before_a_device_is_opened(name, change, code, tmp_path):
    """(the pointer is never written and no device is opened: every one of these returns first, in the header's order)"""
    L = host()
    a = dict(dict(fmt=2, w=640, h=480, filt=U.BILINEAR, path=SPLASH), **change)
    path = (str(tmp_path / "missing.agmv") if a["path"] == "missing" else a["path"]).encode()
    for fmt in ([a["fmt"]] if "fmt" in change else SC.LAYOUTS + SC.YUV_709F):
        assert L.AGMV_DecodeFramesScaledDev(path, C.c_void_p(4096), fmt, a["w"], a["h"], a["filt"], 4, None) == code, fmt
    assert L.AGMV_DecodeFramesScaledDev(None, C.c_void_p(4096), a["fmt"], a["w"], a["h"], a["filt"], 4, None) == -1      # NULL filename, whatever else


def test_without_frames_only_the_info_is_filled():
    """d_frames NULL returns 0 with the file's own size in *info, for every filter -- also for an AREA target the file cannot be
    scaled to, whose refusal comes behind it"""
    from libagmv_amd.seq import AGMV_INFO
    L = host()
    for filt, w, h in ((U.BILINEAR, 640, 480), (U.NEAREST, 7, 5), (U.AREA, 160, 120), (U.AREA, 640, 480)):
        info = AGMV_INFO()
        assert L.AGMV_DecodeFramesScaledDev(SPLASH.encode(), None, 16, w, h, filt, 0, C.byref(info)) == 0
        assert (info.width, info.height, info.number_of_frames) == (320, 240, 119)
    assert L.AGMV_DecodeFramesScaledDev(SPLASH.encode(), None, 16, 0, 480, U.BILINEAR, 0, None) == -4      # the size is looked at first


def test_seq_refuses_a_misuse_of_size_and_scale_before_the_library_is_loaded(tmp_path, monkeypatch):
    import libagmv_amd
    from libagmv_amd import seq

    def reached():
        raise AssertionError("the library was called")
    monkeypatch.setattr(seq, "load_library", reached)
    for scale in ("nearest", "area"):
        with pytest.raises(ValueError, match="size="):
            libagmv_amd.decode_frames(SPLASH, scale=scale)                                         # a filter without a target
    for name in ("bicubic", "BILINEAR", None, 3, ["bilinear"]):
        with pytest.raises(ValueError, match="scale"):
            libagmv_amd.decode_frames(SPLASH, size=(480, 640), scale=name)
        with pytest.raises(ValueError, match="scale"):
            libagmv_amd.decode_frames(SPLASH, scale=name)
    for size in ((480,), (480, 640, 3), (0, 640), (480, -4), (480.0, 640), "480x640", 480, (True, 640)):
        with pytest.raises(ValueError, match="size"):
            libagmv_amd.decode_frames(SPLASH, size=size)
    with pytest.raises(ValueError, match="yuv="):
        libagmv_amd.decode_frames(SPLASH, fmt="rgb24", yuv="bt709", size=(480, 640))               # the older refusal still comes
    with pytest.raises(AssertionError, match="the library was called"):
        libagmv_amd.decode_frames(SPLASH)                                                          # the default scale without a size is today's call
    with pytest.raises(ValueError, match="scale"):
        libagmv_amd.encode_frames(str(tmp_path / "x.agmv"), None, size=(16, 24), scale="bilinear")  # the encoder's filters stay two
    assert not os.listdir(tmp_path)


def test_seq_refuses_an_impossible_target_after_the_header_is_read(monkeypatch):
    """a YUV layout with an odd target and "area" with a target larger than the file: ValueError behind the header call, before
    anything is allocated (torch.empty is patched to fail; only the info call reaches the library)"""
    import torch
    import libagmv_amd
    from libagmv_amd import seq
    L = seq.load_library()
    calls = []

    class Watch:
        def __getattr__(self, name):
            f = getattr(L, name)

            def call(*a):
                calls.append((name, a[1]))
                return f(*a)
            return call
    monkeypatch.setattr(seq, "load_library", lambda: Watch())
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a tensor was allocated")))
    for kw in (dict(fmt="nv12", size=(481, 640)), dict(fmt="i420", size=(480, 641), scale="nearest"), dict(fmt="nv12", size=(119, 160), scale="area")):
        with pytest.raises(ValueError, match="even"):
            libagmv_amd.decode_frames(SPLASH, **kw)
    for size in ((241, 320), (240, 321), (480, 640)):
        with pytest.raises(ValueError, match="area"):
            libagmv_amd.decode_frames(SPLASH, fmt="rgb24", size=size, scale="area")
    assert calls and all(c == ("AGMV_DecodeFramesFmtDev", None) for c in calls)                    # header reads only
