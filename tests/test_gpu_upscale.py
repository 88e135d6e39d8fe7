"""agmv_hip_scale_frames_async, the decoder's scaling sink (AGMV_SCALE_NEAREST / AGMV_SCALE_BILINEAR of include/agmv.h): a packed
XRGB32 clip written at a target size in any of the seven layouts, against the numpy statement of the two rules and of the
layouts' writing rules (tests/upscale_cases.py, tests/scale_cases.py).  Everything is exact.  A lane forms 16 target pixels of a
row (YUV: 16 x 2) and stores them with 16-byte stores where the target's width is a multiple of 16 and its frames lie on 16-byte
boundaries, walking a band of 8 rows; every other target, and a YUV frame with an odd last row, is written pixel by pixel.  The shapes hold both paths and
their edges; a target base off a 16-byte boundary takes an aligned shape to the per-pixel path, which must give the same bytes.
Where a term of the taps leaves 32 bits on either axis the kernels divide in 64: shapes on either side of that (U.up_small).
Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import pixfmt_cases as P
import scale_cases as SC
import upscale_cases as U
import yuv_cases as Y

pytestmark = pytest.mark.gpu

GUARD = 64                                       # bytes on either side of the target
N = 3
NV12_709F = Y.NV12 | Y.BT709 | Y.FULL_RANGE
FORMATS = SC.LAYOUTS + (NV12_709F,)
FILTERS = (U.NEAREST, U.BILINEAR)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    return torch


@pytest.fixture(scope="module")
def hip(torch):
    from libagmv_amd import AgmvHip
    h = AgmvHip(0)
    yield h
    h.close()


def source(sw, sh, seed, n=N):
    """random pixels with bits >= 24 set: they are no pixels"""
    return np.random.default_rng(seed).integers(0, 1 << 32, (n, sh, sw), dtype=np.uint32) | np.uint32(0x80000000)


def run(torch, hip, filt, pix, fmt, dw, dh, off=0):
    """-> (the target's bytes, uint8 [n, frame bytes]; whether the guard bytes on either side of it kept their value)"""
    n, sh, sw = pix.shape
    fb = SC.frame_bytes(fmt, dw, dh)
    buf = torch.full((GUARD + off + n * fb + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    src = torch.from_numpy(pix.view(np.int32)).cuda()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = hip.L.agmv_hip_scale_frames_async(hip.ctx, filt, src.data_ptr(), sw, sh, n, fmt, dw, dh, buf.data_ptr() + GUARD + off, s)
    assert rc == 0, hip.L.agmv_hip_last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    lo, hi = GUARD + off, GUARD + off + n * fb
    return host[lo:hi].reshape(n, fb), bool((host[:lo] == 0x5A).all() and (host[hi:] == 0x5A).all())


@pytest.mark.parametrize("shape", U.SHAPES, ids=[U.shape_id(s) for s in U.SHAPES])
@pytest.mark.parametrize("fmt", FORMATS, ids=[SC.fmt_name(f) for f in FORMATS])
@pytest.mark.parametrize("filt", FILTERS, ids=[U.FILTER_NAMES[f] for f in FILTERS])
def test_every_layout_equals_numpy(torch, hip, filt, fmt, shape):
    """3 frames; once on a 16-byte boundary and once off it (4 bytes for XRGB32, 1 byte for the others): the same bytes"""
    sw, sh, dw, dh = shape
    pix = source(sw, sh, fmt * 1000 + dw)
    exp = np.asarray(SC.from_packed(fmt, U.scale(filt, pix, dw, dh))).view(np.uint8).reshape(N, -1)
    for off in (0, 4 if fmt == P.XRGB32 else 1):
        got, guards = run(torch, hip, filt, pix, fmt, dw, dh, off)
        assert got.shape == exp.shape
        assert (got == exp).all(), (shape, off, np.argwhere(got != exp)[:4], got[got != exp][:4], exp[got != exp][:4])
        assert guards, (shape, off, "guard bytes written")


# a lane of the aligned path walks a band of 8 target rows and keeps its horizontal pass while the two source rows stay the same
BANDS = [(7, 5, 32, 13),             # one band and 5 rows of the next; an odd height: the YUV layouts go pixel by pixel
         (3, 9, 16, 26),             # three bands and a row pair; up in both axes
         (6, 20, 32, 9)]             # down in y: every target row has source rows of its own


@pytest.mark.parametrize("shape", BANDS, ids=[U.shape_id(s) for s in BANDS])
@pytest.mark.parametrize("fmt", FORMATS, ids=[SC.fmt_name(f) for f in FORMATS])
@pytest.mark.parametrize("filt", FILTERS, ids=[U.FILTER_NAMES[f] for f in FILTERS])
def test_bands_of_rows_equal_numpy(torch, hip, filt, fmt, shape):
    sw, sh, dw, dh = shape
    pix = source(sw, sh, fmt * 1000 + dh)
    exp = np.asarray(SC.from_packed(fmt, U.scale(filt, pix, dw, dh))).view(np.uint8).reshape(N, -1)
    got, guards = run(torch, hip, filt, pix, fmt, dw, dh)
    assert (got == exp).all(), (shape, np.argwhere(got != exp)[:4], got[got != exp][:4], exp[got != exp][:4])
    assert guards, (shape, "guard bytes written")


# ---- the 64-bit form of the taps, the column stepper on a downscale, degenerate targets (tests/upscale_cases.py) ----
_scaled = {}


def scaled(filt, shape, n):
    """(the source, its scaled XRGB32 clip by the numpy statement), made once per filter and shape and left unchanged: every layout
    of a shape is written from the same pixels"""
    key = (filt, shape, n)
    if key not in _scaled:
        sw, sh, dw, dh = shape
        pix = source(sw, sh, sw + 7 * dw + 13 * dh, n=n)
        exp = U.scale(filt, pix, dw, dh)
        exp.setflags(write=False)                                 # (the source stays writable: torch.from_numpy warns otherwise)
        _scaled[key] = pix, exp
    return _scaled[key]


def check_shape(torch, hip, filt, fmt, shape, small, n=N):
    assert U.axes_small(shape) == small, (shape, "the shape is on the wrong side of up_small")
    sw, sh, dw, dh = shape
    pix, xrgb = scaled(filt, shape, n)
    exp = np.asarray(SC.from_packed(fmt, xrgb)).view(np.uint8).reshape(n, -1)
    got, guards = run(torch, hip, filt, pix, fmt, dw, dh)
    assert got.shape == exp.shape
    assert (got == exp).all(), (shape, np.argwhere(got != exp)[:4], got[got != exp][:4], exp[got != exp][:4])
    assert guards, (shape, "guard bytes written")


@pytest.mark.parametrize("shape,small", U.WIDE_INDEX, ids=[U.shape_id(s) for s, _ in U.WIDE_INDEX])
@pytest.mark.parametrize("fmt", FORMATS, ids=[SC.fmt_name(f) for f in FORMATS])
@pytest.mark.parametrize("filt", FILTERS, ids=[U.FILTER_NAMES[f] for f in FILTERS])
def test_taps_divided_in_64_bits_equal_numpy(torch, hip, filt, fmt, shape, small):
    """(2X + 1) * s + d leaves 32 bits on one axis, so both axes divide in 64: through x and through y, on the band kernel and pixel by pixel"""
    assert small != (True, True)
    check_shape(torch, hip, filt, fmt, shape, small)


@pytest.mark.parametrize("shape,small", U.BOUNDARY_P, ids=[U.shape_id(s) for s, _ in U.BOUNDARY_P])
@pytest.mark.parametrize("fmt", (P.XRGB32, P.RGB24), ids=("xrgb32", "rgb24"))
@pytest.mark.parametrize("filt", FILTERS, ids=[U.FILTER_NAMES[f] for f in FILTERS])
def test_either_side_of_the_largest_32_bit_numerator(torch, hip, filt, fmt, shape, small):
    sw, sh, dw, dh = shape
    assert ((2 * dw - 1) * sw + dw < 1 << 32) == small[0] and abs((2 * dw - 1) * sw + dw - (1 << 32)) <= 32768
    check_shape(torch, hip, filt, fmt, shape, small)


@pytest.mark.parametrize("shape,small", U.BOUNDARY_F, ids=[U.shape_id(s) for s, _ in U.BOUNDARY_F])
@pytest.mark.parametrize("fmt", (P.XRGB32, P.RGB24), ids=("xrgb32", "rgb24"))
def test_either_side_of_the_largest_32_bit_weight_numerator(torch, hip, fmt, shape, small):
    """one frame of 3 x 1 -> 8.4 million columns, bilinear: 513 * d on either side of 2^32"""
    sw, sh, dw, dh = shape
    assert (513 * dw < 1 << 32) == small[0] and abs(513 * dw - (1 << 32)) < 16 * 513 and (2 * dw - 1) * sw + dw < 1 << 32
    check_shape(torch, hip, U.BILINEAR, fmt, shape, small, n=1)


@pytest.mark.parametrize("shape,small", U.DOWN_X, ids=[U.shape_id(s) for s, _ in U.DOWN_X])
@pytest.mark.parametrize("fmt", FORMATS, ids=[SC.fmt_name(f) for f in FORMATS])
@pytest.mark.parametrize("filt", FILTERS, ids=[U.FILTER_NAMES[f] for f in FILTERS])
def test_down_in_x_with_a_remainder_and_targets_of_one_pixel(torch, hip, filt, fmt, shape, small):
    sw, sh, dw, dh = shape
    assert sw > dw and (sw % dw or (dw, dh) == (1, 1))                             # the column stepper moves by q >= 1 and a remainder
    check_shape(torch, hip, filt, fmt, shape, small)


def test_the_flags_reach_the_writer(torch, hip):
    pix = source(5, 3, 77)
    a, _ = run(torch, hip, U.BILINEAR, pix, Y.NV12, 48, 34)
    b, _ = run(torch, hip, U.BILINEAR, pix, NV12_709F, 48, 34)
    assert (a != b).any()


def test_the_wrapper_and_a_wide_target(torch, hip):
    """AgmvHip.scale_frames_async on 2 frames of 320 x 240 -> 1920 x 1080 NV12 and 640 x 360 RGB24: the flagship ratio, many blocks per frame"""
    pix = source(320, 240, 5, n=2)
    src = torch.from_numpy(pix.view(np.int32)).cuda()
    for fmt, name, (dw, dh) in ((Y.NV12, "nv12", (1920, 1080)), (P.RGB24, "rgb24", (640, 360))):
        got = hip.scale_frames_async(U.BILINEAR, src, 320, 240, 2, name, dw, dh)
        torch.cuda.synchronize()
        exp = np.asarray(SC.from_packed(fmt, U.scale_bilinear(pix, dw, dh))).reshape(2, -1)
        assert tuple(got.shape) == exp.shape and (got.cpu().numpy() == exp).all()


def test_no_frames_and_refusals_launch_nothing(torch, hip):
    src = torch.zeros(64 * 64, dtype=torch.int32, device="cuda")
    dst = torch.full((4 * 64 * 64,), 0x5A, dtype=torch.uint8, device="cuda")
    call = hip.L.agmv_hip_scale_frames_async
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = dict(filt=U.BILINEAR, sw=16, sh=16, n=1, fmt=2, dw=32, dh=32)
    bad = [dict(filt=U.AREA), dict(filt=U.AREA, dw=8, dh=8), dict(filt=0), dict(filt=4),                                  # AREA is another call's; unknown filters
           dict(fmt=0), dict(fmt=6), dict(fmt=15), dict(fmt=18), dict(fmt=2 | 0x100), dict(fmt=16 | 0x400),                 # unknown formats
           dict(sw=0), dict(sh=0), dict(dw=0), dict(dh=0),                                                                 # zero sizes
           dict(dw=1 << 15, dh=(1 << 13) + 1), dict(sw=1 << 15, sh=(1 << 13) + 1)]                                         # more than 2^28 pixels
    for change in bad:
        a = dict(ok, **change)
        assert call(hip.ctx, a["filt"], src.data_ptr(), a["sw"], a["sh"], a["n"], a["fmt"], a["dw"], a["dh"], dst.data_ptr(), s) != 0, change
        assert hip.L.agmv_hip_last_error()
    a = ok
    assert call(hip.ctx, a["filt"], None, a["sw"], a["sh"], 1, a["fmt"], a["dw"], a["dh"], dst.data_ptr(), s) != 0         # NULL pointers
    assert call(hip.ctx, a["filt"], src.data_ptr(), a["sw"], a["sh"], 1, a["fmt"], a["dw"], a["dh"], None, s) != 0
    assert call(None, a["filt"], src.data_ptr(), a["sw"], a["sh"], 1, a["fmt"], a["dw"], a["dh"], dst.data_ptr(), s) != 0  # no context
    assert b"NULL context" in hip.L.agmv_hip_last_error()
    for filt in FILTERS:
        assert call(hip.ctx, filt, src.data_ptr(), a["sw"], a["sh"], 0, a["fmt"], a["dw"], a["dh"], dst.data_ptr(), s) == 0    # no frames: nothing to do
    torch.cuda.synchronize()
    assert bool((dst == 0x5A).all())
    with pytest.raises(RuntimeError, match="area"):
        hip.scale_frames_async(U.AREA, src, 16, 16, 1, "rgb24", 8, 8)
    with pytest.raises(ValueError):
        hip.scale_frames_async(U.BILINEAR, src, 16, 16, 1, "rgb24", 32, 32, yuv="bt709")
