"""AGMV_SCALE_BILINEAR of include/agmv.h stated in numpy on XRGB32 clips, uint32 [n, h, w] of 0x00RRGGBB, with int64 sums, and
the shapes tests/test_upscale_cpu.py, tests/test_gpu_upscale.py and tests/test_gpu_upscale_files.py share.  The other two filters
of the decoder's scaling sink and the layouts are those of tests/scale_cases.py."""
import numpy as np

import scale_cases as SC
from scale_cases import from_packed, scale_area, scale_nearest  # noqa: F401  (the sink's other filters and its writing rules)

NEAREST, AREA, BILINEAR = SC.NEAREST, SC.AREA, 3
FILTER_NAMES = {NEAREST: "nearest", AREA: "area", BILINEAR: "bilinear"}
COLUMNS = 1 << 16                                # target columns scale_bilinear forms at a time

# agmv_hip_scale_frames_async: (sw, sh, dw, dh).  A lane owns 16 target pixels of a row (YUV: 16 x 2).
SHAPES = [(8, 8, 8, 8),              # identity
          (8, 4, 16, 8),             # exactly one 16-group, factor 2
          (5, 3, 48, 34),            # non-integer, three groups, even rows for YUV
          (4, 4, 37, 23),            # odd target: the per-pixel path, and the chroma edges with cnt 2 and 1
          (12, 12, 32, 8),           # up in x, down in y
          (1, 1, 16, 2),             # every tap clamped
          (5, 3, 512, 4)]            # f = 256 occurs


def shape_id(s):
    return "%dx%d-to-%dx%d" % s


def up_small(s, d):
    """whether the kernels divide an axis of source length s and target length d in 32 bits: (2X + 1) * s + d for every X < d and
    256 * r + d for every r < 2d fit 32 bits.  The first is largest at X = d - 1; the second stays below 513 * d, which is the
    bound the library takes"""
    return (2 * d - 1) * s + d < 1 << 32 and 513 * d < 1 << 32


def axes_small(shape):
    """(x, y): a launch takes the 64-bit form on both axes where either is False"""
    sw, sh, dw, dh = shape
    return up_small(sw, dw), up_small(sh, dh)


# Shapes whose products leave 32 bits, each with the side of up_small its axes must fall on (x, y); extreme aspect ratios keep
# them small: 3 frames of the largest are 0.5 MB.
WIDE_INDEX = [((70001, 1, 40000, 2), (False, True)),     # through x; dw a multiple of 16 and dh even: every layout stores 16 bytes at a time
              ((70001, 1, 40001, 3), (False, True)),     # through x, pixel by pixel, with odd YUV edges
              ((1, 70001, 16, 40000), (True, False)),    # through y only: 5000 bands of 8 rows, each dividing on y
              ((2, 70001, 17, 40001), (True, False))]    # through y only, pixel by pixel
# either side of the first term: (2d - 1) * s + d = 2^32 - 32768, the largest a 32-bit p + 2d takes, and 2^32 + 32767
BOUNDARY_P = [((65536, 1, 32768, 2), (True, True)), ((65537, 1, 32768, 2), (False, True))]
# either side of the second term: 513 * d = 2^32 - 8176, where 256 * r + d is the largest 32 bits hold, and 2^32 + 32
BOUNDARY_F = [((3, 1, 8372240, 1), (True, True)), ((3, 1, 8372256, 1), (False, True))]
# down in x with a remainder (the column stepper's q >= 1 and m2 > 0), and targets of one row and of one pixel
DOWN_X = [((37, 5, 16, 8), (True, True)),                # q = 2, 16-byte stores
          ((100, 7, 48, 10), (True, True)),              # q = 2, three groups, bands of 8 and 2 rows
          ((50, 3, 17, 1), (True, True)),                # a single odd YUV row
          ((33, 33, 1, 1), (True, True))]
NEW_SHAPES = WIDE_INDEX + BOUNDARY_P + BOUNDARY_F + DOWN_X


def taps(s, d):
    """(i0, i1, f), int64 [d] each: the taps of every target index on an axis of source length s and target length d"""
    p = (2 * np.arange(d, dtype=np.int64) + 1) * s - d
    neg = p < 0
    q = np.where(neg, 0, p)
    i0 = q // (2 * d)
    f = np.where(neg, 0, (256 * (q % (2 * d)) + d) // (2 * d))
    return i0, np.minimum(i0 + 1, s - 1), f


def scale_bilinear(pix, dw, dh, sums=None):
    """uint32 [n, sh, sw] -> uint32 [n, dh, dw].  sums: a list that receives the largest value any channel's sum took before the shift"""
    pix = np.asarray(pix, np.uint32)
    n, sh, sw = pix.shape
    assert dw > 0 and dh > 0
    x0, x1, fx = taps(sw, dw)
    y0, y1, fy = taps(sh, dh)
    fy = fy[None, :, None]
    out = np.zeros((n, dh, dw), np.uint32)
    for s in (16, 8, 0):
        c = ((pix >> s) & 255).astype(np.int64)
        r0, r1 = c[:, y0], c[:, y1]
        most = 0
        for a in range(0, dw, COLUMNS):                           # (slices that stay in cache: a target of 8 million columns in half the time)
            b = min(a + COLUMNS, dw)
            f, xa, xb = fx[None, None, a:b], x0[a:b], x1[a:b]
            top = (256 - f) * r0[:, :, xa] + f * r0[:, :, xb]
            bot = (256 - f) * r1[:, :, xa] + f * r1[:, :, xb]
            acc = (256 - fy) * top + fy * bot + 32768
            if sums is not None:
                most = max(most, int(acc.max()))
            out[:, :, a:b] |= (acc >> 16).astype(np.uint32) << s
        if sums is not None:
            sums.append(most)
    return out


def scale(filt, pix, dw, dh):
    if filt == BILINEAR:
        return scale_bilinear(pix, dw, dh)
    return SC.scale(filt, pix, dw, dh)


def tap_bounds(pix, dw, dh):
    """(lo, hi), uint32 [n, dh, dw] per channel packed like pix: the smallest and the largest of each target pixel's four taps"""
    pix = np.asarray(pix, np.uint32)
    n, sh, sw = pix.shape
    x0, x1, _ = taps(sw, dw)
    y0, y1, _ = taps(sh, dh)
    lo, hi = np.zeros((n, dh, dw), np.uint32), np.zeros((n, dh, dw), np.uint32)
    for s in (16, 8, 0):
        c = (pix >> s) & 255
        four = np.stack([c[:, ya][:, :, xa] for ya in (y0, y1) for xa in (x0, x1)])
        lo |= four.min(axis=0) << s
        hi |= four.max(axis=0) << s
    return lo, hi
