"""Normalised float tensor clips before they touch the GPU (include/agmv.h, "normalised float tensors"): the headers hold the
definition and the libraries the symbols; agmv_hip_tensor_table (host only) equals the numpy statement of tests/tensor_cases.py bit
for bit and refuses what lies outside the bounds; reading what was written returns every byte; flushing subnormals changes no
byte inside the bounds; AGMV_DecodeFramesTensorDev / AGMV_EncodeFramesTensorDev refuse what they cannot deliver in the header's
order before a device is opened (a fake pointer, no file created); libagmv_amd.seq refuses a misuse before it loads the library."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import hostlib as H
import tensor_cases as TC

ROOT = H.ROOT
SPLASH = os.path.join(ROOT, "tests", "golden", "agmv_splash.agmv")         # 119 frames of 320 x 240
F3 = C.c_float * 3
NEAREST, AREA, BILINEAR = 1, 2, 3


def hiplib():
    import torch  # noqa: F401  (torch's HIP runtime first, as in libagmv_amd.hip.load_library: the GPU tests may share this process)
    from libagmv_amd import hip
    H.lib()
    return hip.load_library()


def host():
    import torch  # noqa: F401
    from libagmv_amd.seq import AGMV_INFO
    L = H.lib()
    return L


def lib_table(t, mean, std):
    out = np.zeros((3, 256), TC.BITS[t])
    rc = hiplib().agmv_hip_tensor_table(t, F3(*mean), F3(*std), out.ctypes.data_as(C.c_void_p))
    return rc, out


def test_headers_and_libraries_hold_the_definition_and_the_functions():
    hdr = open(os.path.join(ROOT, "include", "agmv.h")).read()
    values = dict((k, int(v, 0)) for k, v in re.findall(r"\b(AGMV_TENSOR_\w+)\s*=\s*(\w+)", hdr))
    assert values == {"AGMV_TENSOR_F32": 1, "AGMV_TENSOR_F16": 2, "AGMV_TENSOR_BF16": 3}
    flat = re.sub(r"\s+", " ", hdr)
    for words in ("(v / 255 - mean[c]) / std[c]", "2^-32 <= |std[c]| <= 2^32", "|mean[c]| <= 2^32", "flushes subnormals",
                  "((double)v / 255.0 - (double)mean[c]) / (double)std[c]", "out[k][c][y][x] = T[c][channel c of D(x, y)]",
                  "a[c] = (float)(255.0 * (double)std[c])", "b[c] = (float)(255.0 * (double)mean[c])", "t = fl32(fl32(x * a[c]) + b[c])",
                  "(int)rintf(fminf(fmaxf(t, 0), 255))", "never a fused one", "byte for byte"):
        assert words in flat, words
    for f in ("AGMV_DecodeFramesTensorDev", "AGMV_EncodeFramesTensorDev"):
        assert re.search(r"\bint\s+%s\(" % f, hdr) and hasattr(host(), f), f
    hip_hdr = open(os.path.join(ROOT, "include", "agmv_hip.h")).read()
    hiplib()
    G = C.CDLL(os.path.join(ROOT, "libagmv_amd", "libagmv_hip.so"))
    for f in ("agmv_hip_tensor_frame_bytes", "agmv_hip_tensor_table", "agmv_hip_tensor_from_xrgb_async", "agmv_hip_tensor_to_xrgb_async"):
        assert re.search(r"\b%s\(" % f, hip_hdr) and hasattr(G, f), f
    import libagmv_amd
    from libagmv_amd import hip
    assert libagmv_amd.TENSORFMT == {"f32": 1, "f16": 2, "bf16": 3} and "TENSORFMT" in libagmv_amd.__all__
    assert callable(libagmv_amd.AgmvHip.tensor_from_xrgb_async) and callable(libagmv_amd.AgmvHip.tensor_to_xrgb_async)
    assert libagmv_amd.PIXFMT == {"xrgb32": 1, "rgb24": 2, "bgr24": 3, "rgba32": 4, "rgb8p": 5} and hip.YUVFMT == {"nv12": 16, "i420": 17}


def test_frame_bytes_needs_no_device():
    L = hiplib()
    for n in (1, 16, 320 * 240, 1 << 28):
        assert [L.agmv_hip_tensor_frame_bytes(t, n) for t in TC.TYPES] == [12 * n, 6 * n, 6 * n]
    for t in (0, 4, 5, 16, -1, 255):
        assert L.agmv_hip_tensor_frame_bytes(t, 100) == 0
    assert L.agmv_hip_pixfmt_frame_bytes(0, 100) == 0 and L.agmv_hip_pixfmt_frame_bytes(6, 100) == 0      # the byte layouts stay what they were


TABLE_NORMS = dict(TC.NORMS, **{
    "negative-std": ((0.5, 0.25, 0.0), (-0.5, 0.25, -1.0)),
    "std-2^-32": ((0.0, 0.5, 1.0), (2.0 ** -32, -2.0 ** -32, 2.0 ** -32)),
    "std-2^32": ((0.0, 0.5, -1.0), (2.0 ** 32, -2.0 ** 32, 2.0 ** 32)),
    "mean-2^32": ((2.0 ** 32, -2.0 ** 32, 1e-30), (1.0, 2.0 ** -32, 3.0)),
    "per-channel": ((0.1, 0.2, 0.3), (0.7, 1.3, 255.0))})


@pytest.mark.parametrize("t", TC.TYPES, ids=[TC.NAMES[t] for t in TC.TYPES])
@pytest.mark.parametrize("norm", sorted(TABLE_NORMS))
def test_the_table_equals_numpy_bit_for_bit(norm, t):
    mean, std = TABLE_NORMS[norm]
    rc, got = lib_table(t, mean, std)
    assert rc == 0
    exp = TC.table(t, mean, std)
    assert got.dtype == exp.dtype and (got == exp).all(), (norm, np.argwhere(got != exp)[:4])
    if norm == "std-2^-32" and t == TC.F16:                        # 2^24 and beyond: binary16's overflow is an infinity of the sign
        assert (got[0, 1:] == 0x7C00).all() and (got[1, :127] == 0x7C00).all() and (got[1, 128:] == 0xFC00).all()
    from libagmv_amd import hip
    assert (hip.tensor_table(TC.NAMES[t], mean, std) == exp).all()  # the binding's view of the same call


def test_the_narrow_conversions_at_their_edges():
    """the table's integer code on values chosen for it: ties, the subnormal range of binary16, its overflow.  A std of 1 / x puts
    x itself into T[c][255] when mean is 0 (255 / 255 = 1 exactly, and 1 / (1 / x) for the powers of two used here)"""
    for x in (2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 2.0 ** -26, 65504.0, 65520.0, 2.0 ** 16, 2.0 ** 31):
        for t in TC.TYPES:
            rc, got = lib_table(t, (0, 0, 0), (1 / x, -1 / x, 1 / x))
            assert rc == 0 and (got == TC.table(t, (0, 0, 0), (1 / x, -1 / x, 1 / x))).all(), (x, t)
    f = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24 * 1.5, 2.0 ** -24 * 2.5, 65519.99, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32)
    assert TC.narrow(TC.F16, f).tolist() == [0x3C00, 0x3C02, 0x0002, 0x0002, 0x7BFF, 0x3C04, 0x3C0C]      # half to even, both ways; the last two are exact
    assert TC.narrow(TC.BF16, f)[-2:].tolist() == [0x3F80, 0x3F82]


BAD_NORMS = [((0, 0, 0), (0, 1, 1)), ((0, 0, 0), (1, 1, 2.0 ** -33)), ((0, 0, 0), (1, 2.0 ** 33, 1)), ((0, 0, 0), (1, -2.0 ** 33, 1)),
             ((2.0 ** 33, 0, 0), (1, 1, 1)), ((0, -2.0 ** 33, 0), (1, 1, 1)), ((0, 0, math.nan), (1, 1, 1)), ((0, 0, 0), (math.nan, 1, 1)),
             ((math.inf, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, math.inf)), ((0, 0, 0), (1, -math.inf, 1)), ((0, 0, 0), (1e-45, 1, 1))]


def test_the_table_refuses_what_lies_outside_the_bounds():
    for mean, std in BAD_NORMS:
        for t in TC.TYPES:
            rc, got = lib_table(t, mean, std)
            assert rc != 0 and not got.any(), (mean, std)
    for t in (0, 4, 16):
        out = np.zeros(768, np.uint32)
        assert hiplib().agmv_hip_tensor_table(t, F3(0, 0, 0), F3(1, 1, 1), out.ctypes.data_as(C.c_void_p)) != 0 and not out.any()
    from libagmv_amd import hip
    with pytest.raises(ValueError, match="bounds"):
        hip.tensor_table("f16", 0.0, 0.0)
    with pytest.raises(ValueError, match="fmt"):
        hip.tensor_table("f64")


@pytest.mark.parametrize("t", TC.TYPES, ids=[TC.NAMES[t] for t in TC.TYPES])
@pytest.mark.parametrize("norm", sorted(TC.NORMS))
def test_reading_what_was_written_returns_every_byte(norm, t):
    mean, std = TC.NORMS[norm]
    rc, tab = lib_table(t, mean, std)
    assert rc == 0
    v = np.arange(256, dtype=np.uint32)
    clip = TC.from_packed(tab, (v << 16 | v << 8 | v).reshape(1, 16, 16))
    assert clip.shape == (1, 3, 16, 16)
    back = TC.to_packed(t, clip, mean, std)
    assert (back == (v << 16 | v << 8 | v).reshape(1, 16, 16)).all()
    assert all(len(np.unique(tab[c])) == 256 for c in range(3))    # 256 distinct elements per channel, in BF16 too


def test_flushing_subnormals_changes_no_byte():
    """the reading rule with every input and intermediate result flushed against the rule as it stands: float32 subnormals and the
    smallest normals, the 65 536 binary16 patterns and a sweep of ordinary values, with std and mean at and inside their bounds"""
    rng = np.random.default_rng(7)
    sub = np.concatenate([np.arange(0, 64, dtype=np.uint32), rng.integers(0, 0x01000000, 4096, dtype=np.uint32), np.array([0x007FFFFF, 0x00800000, 0x00800001], np.uint32)])
    sub = np.concatenate([sub, sub | 0x80000000])
    ordinary = np.concatenate([np.linspace(-2, 3, 4001).astype(np.float32).view(np.uint32), rng.integers(0, 1 << 32, 8192, dtype=np.uint32)])
    x32 = np.concatenate([sub, ordinary]).view(np.float32)
    x16 = TC.widen(TC.F16, np.arange(65536, dtype=np.uint16))
    norms = list(TC.NORMS.values()) + [((0, 0, 0), (2.0 ** -32,) * 3), ((0, 0, 0), (2.0 ** 32,) * 3), ((1e-44, -1e-44, 1e-39), (2.0 ** -32, 1.0, -2.0 ** 32)),
                                       ((2.0 ** 32, -2.0 ** 32, 0.5), (2.0 ** 32, 2.0 ** -32, -0.5))]
    for mean, std in norms:
        a, b = TC.coefficients(mean, std)
        for c in range(3):
            for x in (x32, x16):
                assert (TC.read_channel(x, a[c], b[c]) == TC.read_channel(x, a[c], b[c], ftz=True)).all(), (mean, std, c)


def test_known_answers_of_the_reading_rule():
    one = np.float32(1)
    x = np.array([0.0, -0.0, 1.0, 1.1, -3.0, np.inf, -np.inf, np.nan, 3e38, -3e38], np.float32)
    assert TC.read_channel(x, np.float32(255), np.float32(0)).tolist() == [0, 0, 255, 255, 0, 255, 0, 0, 255, 0]
    assert TC.read_channel(x, np.float32(-255), np.float32(255)).tolist() == [255, 255, 0, 0, 255, 0, 255, 0, 0, 255]      # a negative std
    ties = (np.arange(255, dtype=np.float32) + np.float32(0.5))    # k + 0.5 exactly, in the "bytes" normalisation: a = 1
    assert TC.read_channel(ties, one, np.float32(0)).tolist() == [k + (k & 1) for k in range(255)]


# ---- the two public calls: refusals before a device is opened -------------------------------------------------------
ID = (F3(0, 0, 0), F3(1, 1, 1))
DEC_REFUSALS = [
    ("type-0", dict(t=0), -1), ("type-4", dict(t=4), -1), ("type-16", dict(t=16), -1),
    ("std-0", dict(std=F3(1, 0, 1)), -1), ("std-nan", dict(std=F3(1, 1, math.nan)), -1), ("mean-inf", dict(mean=F3(math.inf, 0, 0)), -1),
    ("std-2^33", dict(std=F3(2.0 ** 33, 1, 1)), -1), ("std-2^-33", dict(std=F3(1, 1, 2.0 ** -33)), -1), ("mean-2^33", dict(mean=F3(0, -2.0 ** 33, 0)), -1),
    ("mean-null", dict(mean=None), -1), ("std-null", dict(std=None), -1),
    ("filter-0-with-a-size", dict(filt=0), -1), ("filter-4", dict(filt=4), -1),
    ("unknown-filter-before-zero-size", dict(filt=4, w=0), -1), ("unknown-type-before-missing-file", dict(t=0, path="missing"), -1),
    ("bad-normalisation-before-zero-size", dict(std=F3(0, 0, 0), w=0), -1),
    ("target-0x480", dict(w=0), -4), ("target-640x0", dict(h=0), -4), ("target-above-2^28", dict(w=1 << 14, h=(1 << 14) + 1), -4),
    ("target-width-2^32", dict(w=1 << 32, h=1), -4), ("zero-size-before-missing-file", dict(w=0, path="missing"), -4),
    ("missing-file", dict(path="missing"), -2), ("missing-file-at-the-file's-size", dict(path="missing", w=0, h=0, filt=99), -2),
    ("missing-file-before-area-upscale", dict(path="missing", filt=AREA), -2),
    ("area-upscale-in-x", dict(filt=AREA, w=321, h=240), -4), ("area-upscale-in-y", dict(filt=AREA, w=320, h=241), -4),
]


@pytest.mark.parametrize("name,change,code", DEC_REFUSALS, ids=[r[0] for r in DEC_REFUSALS])
def test_decode_refuses_before_a_device_is_opened(name, change, code, tmp_path):
    """(the pointer is never written and no device is opened: every one of these returns first, in the header's order)"""
    L = host()
    a = dict(dict(t=TC.F16, mean=ID[0], std=ID[1], w=640, h=480, filt=BILINEAR, path=SPLASH), **change)
    path = (str(tmp_path / "missing.agmv") if a["path"] == "missing" else a["path"]).encode()
    for t in ([a["t"]] if "t" in change else TC.TYPES):
        assert L.AGMV_DecodeFramesTensorDev(path, C.c_void_p(4096), t, a["mean"], a["std"], a["w"], a["h"], a["filt"], 4, None) == code, t
    assert L.AGMV_DecodeFramesTensorDev(None, C.c_void_p(4096), a["t"], a["mean"], a["std"], a["w"], a["h"], a["filt"], 4, None) == -1


def test_decode_without_a_tensor_only_fills_the_info():
    from libagmv_amd.seq import AGMV_INFO
    L = host()
    for filt, w, h in ((BILINEAR, 640, 480), (NEAREST, 7, 5), (AREA, 160, 120), (AREA, 640, 480), (99, 0, 0), (0, 0, 0)):
        info = AGMV_INFO()
        assert L.AGMV_DecodeFramesTensorDev(SPLASH.encode(), None, TC.BF16, F3(0.5, 0.5, 0.5), F3(0.5, 0.5, 0.5), w, h, filt, 0, C.byref(info)) == 0
        assert (info.width, info.height, info.number_of_frames) == (320, 240, 119)
    assert L.AGMV_DecodeFramesTensorDev(SPLASH.encode(), None, TC.BF16, ID[0], ID[1], 0, 480, BILINEAR, 0, None) == -4


ENC_OK = dict(t=TC.F16, mean=ID[0], std=ID[1], n=8, w=64, h=48, opt=3, quality=3, compression=1, schedule=2)
ENC_REFUSALS = [
    ("type-0", dict(t=0), -1), ("type-4", dict(t=4), -1), ("std-0", dict(std=F3(0, 1, 1)), -1), ("mean-nan", dict(mean=F3(0, math.nan, 0)), -1),
    ("std-2^33", dict(std=F3(1, 2.0 ** 33, 1)), -1), ("mean-null", dict(mean=None), -1), ("std-null", dict(std=None), -1),
    ("opt-0", dict(opt=0), -1), ("opt-9", dict(opt=9), -1), ("quality-0", dict(quality=0), -1), ("compression-3", dict(compression=3), -1),
    ("schedule-0", dict(schedule=0), -1), ("schedule-4", dict(schedule=4), -1),
    ("bad-type-before-too-few-frames", dict(t=0, n=1), -1), ("bad-normalisation-before-a-bad-size", dict(std=F3(0, 0, 0), w=6), -1),
    ("too-few-frames-pdifs", dict(n=3), -2), ("too-few-frames-heavy", dict(n=1, opt=1), -2), ("no-frames-full", dict(n=0, schedule=1), -2),
    ("width-6", dict(w=6), -3), ("height-0", dict(h=0), -3), ("above-2^28", dict(w=1 << 14, h=(1 << 14) + 4), -3),
    ("too-few-frames-and-a-bad-width", dict(n=3, w=6), None),
]


@pytest.mark.parametrize("name,change,code", ENC_REFUSALS, ids=[r[0] for r in ENC_REFUSALS])
def test_encode_refuses_before_a_device_is_opened(name, change, code, tmp_path):
    """a fake pointer that is never read; no file is created; and where the type and the normalisation are good the value is the
    one AGMV_EncodeFramesDev returns for the same clip geometry"""
    L = host()
    a = dict(ENC_OK, **change)
    out = str(tmp_path / "x.agmv").encode()
    rc = L.AGMV_EncodeFramesTensorDev(out, C.c_void_p(4096), a["t"], a["mean"], a["std"], a["n"], a["w"], a["h"], 24, a["opt"], a["quality"], a["compression"], a["schedule"])
    assert rc < 0 and (code is None or rc == code)
    if not ({"t", "mean", "std"} & set(change)):
        assert rc == L.AGMV_EncodeFramesDev(out, C.c_void_p(4096), a["n"], a["w"], a["h"], 24, a["opt"], a["quality"], a["compression"], a["schedule"])
    assert L.AGMV_EncodeFramesTensorDev(None, C.c_void_p(4096), a["t"], a["mean"], a["std"], a["n"], a["w"], a["h"], 24, a["opt"], a["quality"], a["compression"], a["schedule"]) < 0
    assert L.AGMV_EncodeFramesTensorDev(out, None, TC.F32, ID[0], ID[1], 8, 64, 48, 24, 3, 3, 1, 2) == -1
    assert not os.listdir(tmp_path)


def test_seq_refuses_a_misuse_before_the_library_is_loaded(tmp_path, monkeypatch):
    import torch
    import libagmv_amd
    from libagmv_amd import seq

    def reached():
        raise AssertionError("the library was called")
    monkeypatch.setattr(seq, "load_library", reached)
    out = str(tmp_path / "x.agmv")
    f16 = torch.zeros((4, 3, 16, 16), dtype=torch.float16)
    for fmt in ("xrgb32", "rgb8p", "nv12", 5):
        with pytest.raises(ValueError, match="mean="):
            libagmv_amd.decode_frames(SPLASH, fmt=fmt, mean=0.5)
        with pytest.raises(ValueError, match="mean="):
            libagmv_amd.decode_frames(SPLASH, fmt=fmt, std=(0.5, 0.5, 0.5))
    with pytest.raises(ValueError, match="mean="):
        libagmv_amd.encode_frames(out, torch.zeros((4, 3, 16, 16), dtype=torch.uint8), mean=0.5)
    with pytest.raises(ValueError, match="mean="):
        libagmv_amd.encode_frames(out, torch.zeros((4, 16, 16), dtype=torch.int32), fmt="xrgb32", std=2.0)
    for kw in (dict(yuv="bt709"), dict(full_range=True), dict(size=(8, 8)), dict(size=(8, 8), scale="nearest")):
        with pytest.raises(ValueError, match="tensor clip"):
            libagmv_amd.encode_frames(out, f16, **kw)
        with pytest.raises(ValueError, match="tensor clip"):
            libagmv_amd.encode_frames(out, f16, fmt="f16", **kw)
    for kw in (dict(yuv="bt601"), dict(full_range=True)):
        with pytest.raises(ValueError, match="yuv="):
            libagmv_amd.decode_frames(SPLASH, fmt="bf16", **kw)
    for bad in ("half", (1, 2), (1, 2, 3, 4), object(), [0.5, "x", 1], True):
        with pytest.raises(ValueError, match="std"):
            libagmv_amd.decode_frames(SPLASH, fmt="f32", std=bad)
        with pytest.raises(ValueError, match="mean"):
            libagmv_amd.encode_frames(out, f16, mean=bad)
    with pytest.raises(ValueError, match="fmt"):
        libagmv_amd.encode_frames(out, f16, fmt="f32")                                            # the named type is not the tensor's
    with pytest.raises(ValueError, match="fmt"):
        libagmv_amd.encode_frames(out, torch.zeros((4, 3, 16, 16), dtype=torch.float64))           # no tensor type
    with pytest.raises(ValueError, match="fmt"):
        libagmv_amd.encode_frames(out, torch.zeros((4, 16, 16, 3), dtype=torch.float32), fmt="f32")   # channels last
    with pytest.raises(ValueError, match="fmt"):
        libagmv_amd.encode_frames(out, torch.zeros((2, 16, 16), dtype=torch.float32))              # a 3-d float tensor is no tensor clip
    with pytest.raises(ValueError, match="contiguous"):
        libagmv_amd.encode_frames(out, torch.zeros((4, 3, 16, 32), dtype=torch.float32)[:, :, :, ::2])
    with pytest.raises(ValueError, match="size="):
        libagmv_amd.decode_frames(SPLASH, fmt="f16", scale="nearest")                              # the older refusals still come
    with pytest.raises(ValueError, match="must be on"):
        libagmv_amd.encode_frames(out, f16)                                                        # a good tensor clip gets as far as the device check
    with pytest.raises(AssertionError, match="the library was called"):
        libagmv_amd.decode_frames(SPLASH, fmt="f16", mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), size=(224, 224))
    assert not os.listdir(tmp_path)
