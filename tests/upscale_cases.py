"""AGMV_SCALE_BILINEAR of include/agmv.h stated in numpy on XRGB32 clips, uint32 [n, h, w] of 0x00RRGGBB, with int64 sums, and
the shapes tests/test_upscale_cpu.py, tests/test_gpu_upscale.py and tests/test_gpu_upscale_files.py share.  The other two filters
of the decoder's scaling sink and the layouts are those of tests/scale_cases.py."""
import numpy as np

import scale_cases as SC
from scale_cases import from_packed, scale_area, scale_nearest  # noqa: F401  (the sink's other filters and its writing rules)

NEAREST, AREA, BILINEAR = SC.NEAREST, SC.AREA, 3
FILTER_NAMES = {NEAREST: "nearest", AREA: "area", BILINEAR: "bilinear"}

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
    fx, fy = fx[None, None, :], fy[None, :, None]
    out = np.zeros((n, dh, dw), np.uint32)
    for s in (16, 8, 0):
        c = ((pix >> s) & 255).astype(np.int64)
        top = (256 - fx) * c[:, y0][:, :, x0] + fx * c[:, y0][:, :, x1]
        bot = (256 - fx) * c[:, y1][:, :, x0] + fx * c[:, y1][:, :, x1]
        acc = (256 - fy) * top + fy * bot + 32768
        if sums is not None:
            sums.append(int(acc.max()))
        out |= (acc >> 16).astype(np.uint32) << s
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
