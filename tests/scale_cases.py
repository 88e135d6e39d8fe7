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


def _area_axis(c, d):
    """int64 [..., s] -> int64 [..., d]: target X = F((X + 1) * s) - F(X * s), where every source pixel is d units long and
    F(t) = d * (the sum of the pixels before pixel t div d) + (t mod d) * pixel t div d is the integral of the row up to unit t"""
    s = c.shape[-1]
    cum = np.zeros(c.shape[:-1] + (s + 1,), np.int64)
    np.cumsum(c, axis=-1, out=cum[..., 1:])
    t = np.arange(d + 1, dtype=np.int64) * s
    i, r = t // d, t % d
    assert i[-1] == s and r[-1] == 0                              # F(s * d) takes nothing of a pixel behind the row
    F = d * cum[..., i] + r * c[..., np.minimum(i, s - 1)]
    return F[..., 1:] - F[..., :-1]


def scale_area_streamed(pix, dw, dh):
    """scale_area without the weight matrices, for shapes whose [dw, sw] matrix cannot be held: prefix sums along x, then along y,
    in int64, then the same rounding.  tests/test_scale_cpu.py proves it equal to scale_area on every shape of STARRED and MORE"""
    pix = np.asarray(pix, np.uint32)
    n, sh, sw = pix.shape
    assert 0 < dw <= sw and 0 < dh <= sh and sw * sh <= AREA_MAX_SOURCE
    out = np.zeros((n, dh, dw), np.uint32)
    for s in (16, 8, 0):
        c = ((pix >> s) & 255).astype(np.int64)
        acc = _area_axis(_area_axis(c, dw).swapaxes(1, 2), dh).swapaxes(1, 2)     # int64 [n, dh, dw]
        assert acc.shape == (n, dh, dw) and int(acc.max()) <= 255 * sw * sh
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


def area_small(shape):
    """whether a lane's position u = (source column) * dw, at most (sw - 1) * dw, is formed in 32 bits: the library asks sw * dw < 2^32"""
    return shape[0] * shape[2] < 1 << 32


# (shape, area_small): scale_area_streamed states these, the weight matrices of scale_area would hold up to 2^32 elements
WIDE_U = [((65536, 2, 65536, 1), False),      # sw * dw = 2^32 exactly: the identity in x, 64 tiles
          ((65536, 2, 65535, 1), True)]       # the largest 32-bit u, weights 1 and dw - 1
WIDE_TILES = ((131072, 1, 40000, 1), False)   # 40 accumulator tiles
WIDE_BOUND = ((1 << 22, 4, 4099, 3), False)   # sw * sh = 2^24, the accumulator bound, with the 64-bit u: five tiles, target rows astride source rows


def shape_id(s):
    return "%dx%d-to-%dx%d" % s
