"""A view of a source clip in any of the seven layouts (agmv_hip_view_source_async of include/agmv_hip_view_source.h, AGMV_EncodeViewDev
of include/agmv.h) stated in numpy: the clip is read to XRGB32 by its layout's reading rule (tests/scale_cases.py), then the frames
and the window are taken from that (tests/view_cases.py).  And the window arithmetic of encode_frames(fit="crop").  Nothing here
calls the code under test."""
import numpy as np

import scale_cases as SC
import view_cases as V
import yuv_cases as Y

YUV_FLAGS = (0, Y.BT709, Y.FULL_RANGE, Y.BT709 | Y.FULL_RANGE)


def raw_clip(fmt, n, h, w, seed):
    """n frames of h x w in fmt, uint8 [n, frame bytes], every byte random -- but the fourth of an XRGB32 word, which the reading
    rule of tests/scale_cases.py masks and the copy keeps"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (n, SC.frame_bytes(fmt, w, h)), dtype=np.uint8)
    if fmt == SC.P.XRGB32:
        raw[:, 3::4] = 0
    return raw


def packed(fmt, raw, w, h):
    """the XRGB32 clip S a source stands for, uint32 [n, h, w], frame by frame"""
    return np.concatenate([SC.to_packed(fmt, raw[k:k + 1], w, h) for k in range(raw.shape[0])]) if raw.shape[0] else np.zeros((0, h, w), np.uint32)


def view(fmt, raw, w, h, first=0, count=0, step=1, x=0, y=0, width=0, height=0):
    """V of include/agmv.h: the selected windows of S"""
    return V.view(packed(fmt, raw, w, h), first, count, step, x, y, width, height)


def fit_window(src_h, src_w, h, w):
    """(top, left, height, width): the largest centred window of the target's aspect, as encode_frames(fit="crop") defines it"""
    if src_w * h >= src_h * w:
        ch, cw = src_h, (src_h * w) // h
    else:
        cw, ch = src_w, (src_w * h) // w
    return (src_h - ch) // 2, (src_w - cw) // 2, ch, cw


def fit_by_search(src_h, src_w, h, w):
    """(height, width) of the same window without a division: the full frame on the axis where the source has room to spare for the
    target's aspect, and on the other the largest length, found by counting down, at which the window is not yet wider (taller)
    than the target"""
    if src_w * h >= src_h * w:
        cw = src_w
        while cw * h > src_h * w:
            cw -= 1
        return src_h, cw
    ch = src_h
    while ch * w > src_w * h:
        ch -= 1
    return ch, src_w
