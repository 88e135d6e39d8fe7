"""A view of a clip at another frame rate (AGMV_RATE of include/agmv.h, agmv_hip_time_frames_async of include/agmv_hip_time.h)
stated in numpy: the clip is read to XRGB32 by its layout's reading rule and its frames and window are taken (tests/view_source_cases.py,
which stands on tests/pixfmt_cases.py and tests/yuv_cases.py), then the frames of the result are formed per channel in uint64 with
integer division.  And the clips the tests of the time axis share.  Nothing here calls the code under test."""
import math

import numpy as np

import scale_cases as SC
import view_source_cases as VS

NEAREST, AREA = 1, 2                            # AGMV_TIME
FILTER_NAMES = {NEAREST: "nearest", AREA: "area"}
MAX_RATE = 65535


def reduced(src, dst):
    g = math.gcd(src, dst)
    return src // g, dst // g


def length(nv, src, dst):
    """m: the frames of the result of a view of nv frames"""
    sn, dn = reduced(src, dst)
    return nv * dn // sn


def weights(sn, dn, j):
    """[(k, wt)]: the frames of V with a weight above 0 in frame j of R under AREA, sn : dn reduced: the overlaps of
    [k dn, (k + 1) dn) with [j sn, (j + 1) sn)"""
    lo, hi = j * sn, (j + 1) * sn
    out = []
    for k in range(lo // dn, (hi - 1) // dn + 1):
        wt = min((k + 1) * dn, hi) - max(k * dn, lo)
        assert 0 < wt <= dn
        out.append((k, wt))
    return out


def nearest_index(sn, dn, j):
    return (2 * j + 1) * sn // (2 * dn)


def nearest_by_search(sn, dn, j):
    """the same frame without a division: the last k whose interval starts at or before the centre of the target interval,
    k * 2 dn <= (2j + 1) sn"""
    k = 0
    while (k + 1) * 2 * dn <= (2 * j + 1) * sn:
        k += 1
    return k


def taps(sn, dn, filt, j):
    return [(nearest_index(sn, dn, j), sn)] if filt == NEAREST else weights(sn, dn, j)


def frame_reads(nv, src, dst, filt):
    sn, dn = reduced(src, dst)
    return sum(len(taps(sn, dn, filt, j)) for j in range(nv * dn // sn))


def resample(V, src, dst, filt, j0=0, count=None):
    """frames j0 .. j0 + count - 1 (count None: to the last) of R for the XRGB32 clip V, uint32 [nv, h, w]: bits 24 .. 31 are 0"""
    sn, dn = reduced(src, dst)
    assert filt in (NEAREST, AREA) and (filt == NEAREST or dn <= sn)
    m = V.shape[0] * dn // sn
    count = m - j0 if count is None else count
    assert 0 <= j0 and j0 + count <= m
    out = np.zeros((count,) + V.shape[1:], np.uint32)
    for jj in range(count):
        acc = [np.zeros(V.shape[1:], np.uint64) for _ in range(3)]
        for k, wt in taps(sn, dn, filt, j0 + jj):
            for c, sh in enumerate((16, 8, 0)):
                acc[c] += np.uint64(wt) * ((V[k] >> np.uint32(sh)) & np.uint32(0xFF)).astype(np.uint64)
        r, g, b = [((a + np.uint64(sn // 2)) // np.uint64(sn)).astype(np.uint32) for a in acc]
        out[jj] = r << np.uint32(16) | g << np.uint32(8) | b
    return out


def resample_source(fmt, raw, w, h, first, step, x, y, width, height, src, dst, filt, j0=0, count=None):
    """the same of a clip in fmt, uint8 [n, frame bytes]: V is the view to the end of the clip"""
    return resample(VS.view(fmt, raw, w, h, first, 0, step, x, y, width, height), src, dst, filt, j0, count)


FLAT = (slice(2, 6), slice(4, 10))               # rows, columns of the region that is flat in time: whole 2 x 2 cells


def moving_packed(n, h, w, seed):
    """an XRGB32 clip, uint32 [n, h, w], whose pixels change from frame to frame by a different amount per channel (red by 1 .. 7,
    green by 8 .. 40, blue by 41 .. 120, modulo 256, from a random first frame) -- outside FLAT, where every frame has the first one's pixels"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (3, h, w), dtype=np.int64)
    step = np.stack([rng.integers(1, 8, (h, w)), rng.integers(8, 41, (h, w)), rng.integers(41, 121, (h, w))])
    step[(slice(None),) + FLAT] = 0
    t = np.arange(n, dtype=np.int64).reshape(n, 1, 1, 1)
    c = ((base[None] + t * step[None]) % 256).astype(np.uint32)
    return c[:, 0] << np.uint32(16) | c[:, 1] << np.uint32(8) | c[:, 2]


def moving_clip(fmt, n, h, w, seed):
    """(raw, packed): the moving clip written in fmt, uint8 [n, frame bytes], and the XRGB32 clip that stands for (for the YUV
    layouts the writing is lossy: packed is what is read back, and FLAT is still flat in time, cell by cell, for even bounds)"""
    raw = SC.from_packed(fmt, moving_packed(n, h, w, seed))
    return raw, VS.packed(fmt, raw, w, h)


def white_clip(n, h, w):
    """n frames of 0x00FFFFFF, uint32 [n, h, w]"""
    return np.full((n, h, w), 0x00FFFFFF, np.uint32)


def reduced_pairs(limit):
    return [(s, d) for s in range(1, limit + 1) for d in range(1, limit + 1) if math.gcd(s, d) == 1]
