"""The two scale rules of include/agmv.h (AGMV_SCALE_NEAREST, AGMV_SCALE_AREA) stated in numpy on XRGB32 clips, uint32 [n, h, w] of
0x00RRGGBB, with int64 sums; and the cases tests/test_scale_cpu.py, tests/test_gpu_scale.py and tests/test_gpu_scale_files.py share.
A clip in another layout is scaled by reading it to XRGB32 first (tests/pixfmt_cases.py, tests/yuv_cases.py)."""
import functools

import numpy as np

import pixfmt_cases as P
import yuv_cases as Y

NEAREST, AREA = 1, 2
FILTER_NAMES = {NEAREST: "nearest", AREA: "area"}
AREA_MAX_SOURCE = 1 << 24                       # sw * sh of AGMV_SCALE_AREA: 255 * sw * sh + sw * sh / 2 < 2^32

# the seven layouts as the fmt argument; the YUV ones once plain (BT.601 limited) and once with both flags
BYTE_LAYOUTS = (P.XRGB32, P.RGB24, P.BGR24, P.RGBA32, P.RGB8P)
YUV_PLAIN = (Y.NV12, Y.I420)
YUV_709F = (Y.NV12 | Y.BT709 | Y.FULL_RANGE, Y.I420 | Y.BT709 | Y.FULL_RANGE)
LAYOUTS = BYTE_LAYOUTS + YUV_PLAIN


def fmt_name(fmt):
    if fmt & 0xFF in Y.LAYOUTS:
        return "%s-%s" % (Y.NAMES[fmt & 0xFF], Y.FLAG_NAMES[fmt & 0x300])
    return P.NAMES[fmt]


def frame_bytes(fmt, w, h):
    return Y.frame_bytes(fmt, w, h) if fmt & 0xFF in Y.LAYOUTS else P.frame_bytes(fmt, w * h)


def to_packed(fmt, raw, w, h):
    """a clip in fmt, uint8 [n, frame bytes] -> the XRGB32 clip it stands for, uint32 [n, h, w]"""
    raw = np.asarray(raw, np.uint8)
    if fmt & 0xFF in Y.LAYOUTS:
        return Y.to_packed(fmt, raw, w, h)
    return P.to_packed(fmt, raw, w * h)[0].reshape(raw.shape[0], h, w)


def from_packed(fmt, pix):
    """uint32 [n, h, w] -> the clip in fmt, uint8 [n, frame bytes] (for YUV a lossy writing: read it back for the clip it stands for)"""
    n, h, w = pix.shape
    if fmt & 0xFF in Y.LAYOUTS:
        return Y.from_packed(fmt, pix, w, h)
    return P.from_packed(fmt, pix.reshape(n, h * w))


@functools.lru_cache(maxsize=8)
def weights(s, d):
    """int64 [d, s]: the overlap of target pixel X = [X * s, (X + 1) * s) with source pixel i = [i * d, (i + 1) * d)"""
    X = np.arange(d, dtype=np.int64)[:, None]
    i = np.arange(s, dtype=np.int64)[None, :]
    w = np.clip(np.minimum((X + 1) * s, (i + 1) * d) - np.maximum(X * s, i * d), 0, None)
    w.setflags(write=False)
    return w


def scale_area(pix, dw, dh):
    """uint32 [n, sh, sw] -> uint32 [n, dh, dw]: per channel (sum of wy * wx * S + (sw * sh) div 2) div (sw * sh)"""
    pix = np.asarray(pix, np.uint32)
    n, sh, sw = pix.shape
    assert 0 < dw <= sw and 0 < dh <= sh and sw * sh <= AREA_MAX_SOURCE
    wx, wy = weights(sw, dw), weights(sh, dh)
    assert (wx.sum(axis=1) == sw).all() and (wy.sum(axis=1) == sh).all() and wx.max() <= dw and wy.max() <= dh
    out = np.zeros((n, dh, dw), np.uint32)
    for s in (16, 8, 0):
        c = ((pix >> s) & 255).astype(np.int64)
        acc = np.matmul(np.matmul(wy, c), wx.T)                   # int64 [n, dh, dw]
        out |= ((acc + (sw * sh) // 2) // (sw * sh)).astype(np.uint32) << s
    return out


def scale_nearest(pix, dw, dh):
    """uint32 [n, sh, sw] -> uint32 [n, dh, dw]: D(X, Y) = S(((2X + 1) * sw) div (2 * dw), ((2Y + 1) * sh) div (2 * dh))"""
    pix = np.asarray(pix, np.uint32)
    n, sh, sw = pix.shape
    assert dw > 0 and dh > 0
    xs = ((2 * np.arange(dw, dtype=np.int64) + 1) * sw) // (2 * dw)
    ys = ((2 * np.arange(dh, dtype=np.int64) + 1) * sh) // (2 * dh)
    return np.ascontiguousarray(pix[:, ys][:, :, xs] & 0xFFFFFF)


def scale(filt, pix, dw, dh):
    return scale_area(pix, dw, dh) if filt == AREA else scale_nearest(pix, dw, dh)


def doubled(pix):
    """every pixel twice in both directions"""
    return np.repeat(np.repeat(pix, 2, axis=1), 2, axis=2)


# agmv_hip_scale_area_dev: (sw, sh, dw, dh).  SC_TILE target columns share one LDS accumulator row in the kernel (1024).
STARRED = [(8, 8, 4, 4),             # an integer factor
           (7, 5, 3, 2),             # odd sizes, odd YUV edges; the second frame of a byte layout starts unaligned
           (1920, 18, 320, 4)]       # the real ratios 6 and 4.5: one source row feeds two target rows; 16-byte loads
MORE = [(5, 7, 5, 3),                # one axis identity
        (1, 1, 1, 1),
        (259, 3, 37, 1),             # runs across lane and wave edges
        (1000, 16, 999, 15),         # weights 1 and dw - 1
        (5000, 2, 2499, 1),          # a target wider than one accumulator tile: three tiles, their edges inside source pixels
        (2064, 4, 1040, 2)]          # tiles again, with 16-byte loads (2064 = 16 * 129) and a tile edge inside a source pixel's reach


def shape_id(s):
    return "%dx%d-to-%dx%d" % s
