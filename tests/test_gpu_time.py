"""agmv_hip_time_frames_async (k_time) against the numpy statement of tests/time_cases.py, word for word: a view of a clip in each of
the seven layouts resampled in time, between guard words.  13 frames of 40 x 24: the full frame, a window with no aligned group, a
5-pixel tail, odd YUV offsets and an odd last row, and one whole group plus a 4-pixel tail at x = 16; 40 is no multiple of 16, so
only the 4-byte layouts, the YUV layouts (patches of 8 x 2, 8-byte loads) and every other row of the 1- and 3-byte ones take their wide
loads there, and the same windows are cut from 48 x 24 frames, where every layout does.  The rates are an integer factor, ratios whose taps straddle outputs, one output from
all frames, nearly 1 : 1, and under NEAREST a duplication.  A strided view, batches (j0 > 0), clips off their 16-byte boundaries,
the accumulators' bound at 65535 taps of 255, and refusals that write nothing.  Needs an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import scale_cases as SC
import time_cases as TC
import view_source_cases as VS
import yuv_cases as Y

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0x5A5A5A5A                     # words on either side of the target (256 bytes: the alignment stays), and what they hold
N, SH = 13, 24
WIDTHS = (40, 48)
WINDOWS = [(0, 0, 0, 0), (3, 1, 21, 7), (16, 0, 20, 24)]                        # (x, y, w, h); zeros: the full frame
RATES = [(4, 1, TC.AREA), (5, 2, TC.AREA), (3, 2, TC.AREA), (7, 3, TC.AREA), (13, 1, TC.AREA), (13, 12, TC.AREA),
         (4, 1, TC.NEAREST), (5, 2, TC.NEAREST), (2, 5, TC.NEAREST)]
FORMATS = SC.LAYOUTS
RGB24 = SC.P.RGB24


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


@functools.lru_cache(maxsize=None)
def source(fmt, sw):
    """(raw, packed) of the 13-frame clip of sw x 24 in fmt, made once and left unchanged"""
    raw, packed = TC.moving_clip(fmt, N, SH, sw, 400 + sw)
    raw.setflags(write=False)
    packed.setflags(write=False)
    return raw, packed


class Clip:
    """a source clip on the device `src_off` bytes behind a 16-byte boundary, and the XRGB32 clip it stands for on the host"""

    def __init__(self, torch, fmt, raw, packed, src_off=0):
        self.fmt, self.n, (self.sh, self.sw), self.packed = fmt, raw.shape[0], packed.shape[1:], packed
        self.dev = torch.zeros(raw.size + 32, dtype=torch.uint8, device="cuda")
        assert self.dev.data_ptr() % 16 == 0
        self.dev[src_off:src_off + raw.size] = torch.from_numpy(raw.reshape(-1).copy()).cuda()
        self.ptr = self.dev.data_ptr() + src_off

    def run(self, torch, hip, first, step, view_len, win, rate, j0, count, dst_off=0, n_frames=None, fmt=None, src=True, dst=True):
        """-> (return value, the target's words [count, h, w], whether every word around it kept the fill)"""
        x, y, w, h = win
        buf = torch.full((GUARD + dst_off + count * w * h + GUARD,), FILL, dtype=torch.int32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = hip.L.agmv_hip_time_frames_async(hip.ctx, self.fmt if fmt is None else fmt, self.ptr if src else None, self.sw, self.sh, self.n if n_frames is None else n_frames,
                                              first, step, view_len, x, y, w, h, rate[0], rate[1], rate[2], j0, count,
                                              buf.data_ptr() + 4 * (GUARD + dst_off) if dst else None, s)
        torch.cuda.synchronize()
        host = buf.cpu().numpy().view(np.uint32)
        lo, hi = GUARD + dst_off, GUARD + dst_off + count * w * h
        return rc, host[lo:hi].reshape(count, h, w), bool((host[:lo] == FILL).all() and (host[hi:] == FILL).all())

    def check(self, torch, hip, first, step, win, rate, j0=0, count=None, dst_off=0):
        x, y, w, h = win = win if win[2] else (0, 0, self.sw, self.sh)
        v = self.packed[first::step, y:y + h, x:x + w]
        m = TC.length(v.shape[0], rate[0], rate[1])
        count = m - j0 if count is None else count
        exp = TC.resample(v, rate[0], rate[1], rate[2], j0, count)
        rc, got, guards = self.run(torch, hip, first, step, v.shape[0], win, rate, j0, count, dst_off)
        what = (SC.fmt_name(self.fmt), (self.sw, self.sh), (first, step), win, rate, (j0, count), dst_off)
        assert rc == 0, (what, hip.L.agmv_hip_last_error())
        assert (got == exp).all(), (what, np.argwhere(got != exp)[:4])
        assert guards, (what, "guard words written")
        return count


@pytest.mark.parametrize("sw", WIDTHS)
@pytest.mark.parametrize("fmt", FORMATS, ids=[SC.fmt_name(f) for f in FORMATS])
def test_every_window_and_rate_equals_numpy(torch, hip, fmt, sw):
    clip = Clip(torch, fmt, *source(fmt, sw))
    frames = 0
    for win in WINDOWS:
        for rate in RATES:
            frames += clip.check(torch, hip, 0, 1, win, rate)
    assert frames == 3 * (3 + 5 + 8 + 5 + 1 + 12 + 3 + 5 + 32)


@pytest.mark.parametrize("fmt", FORMATS, ids=[SC.fmt_name(f) for f in FORMATS])
def test_a_strided_view_and_batches(torch, hip, fmt):
    """first = 1, step = 2: V's frame index is not the source's (6 frames); then parts of a result against the same frames of the whole"""
    clip = Clip(torch, fmt, *source(fmt, 40))
    for win in WINDOWS[:2]:
        for rate in ((3, 2, TC.AREA), (5, 2, TC.AREA), (6, 1, TC.AREA), (7, 1, TC.AREA), (2, 1, TC.NEAREST), (2, 5, TC.NEAREST)):
            clip.check(torch, hip, 1, 2, win, rate)
        clip.check(torch, hip, 2, 3, win, (3, 2, TC.AREA))
    for rate, j0, count in (((13, 12, TC.AREA), 5, 4), ((13, 12, TC.AREA), 11, 1), ((3, 2, TC.AREA), 3, 5), ((5, 2, TC.AREA), 4, 1), ((2, 5, TC.NEAREST), 7, 20),
                            ((4, 1, TC.NEAREST), 2, 1), ((3, 2, TC.AREA), 8, 0)):
        clip.check(torch, hip, 0, 1, WINDOWS[1], rate, j0, count)
        clip.check(torch, hip, 0, 1, WINDOWS[2], rate, j0, count)


FLAGGED = [f | flags for f in SC.YUV_PLAIN for flags in VS.YUV_FLAGS if flags]


@pytest.mark.parametrize("fmt", FLAGGED, ids=[SC.fmt_name(f) for f in FLAGGED])
def test_both_matrices_and_both_ranges(torch, hip, fmt):
    clip = Clip(torch, fmt, *TC.moving_clip(fmt, N, SH, 48, 460))
    for win in WINDOWS:
        clip.check(torch, hip, 0, 1, win, (5, 2, TC.AREA))
        clip.check(torch, hip, 1, 2, win, (2, 1, TC.NEAREST))


@pytest.mark.parametrize("src_off,dst_off", [(0, 1), (1, 0), (1, 1)], ids=["target-off", "source-off", "both-off"])
@pytest.mark.parametrize("fmt", FORMATS, ids=[SC.fmt_name(f) for f in FORMATS])
def test_clips_off_their_16_byte_boundary_give_the_same_words(torch, hip, fmt, src_off, dst_off):
    """the source 1 byte off (XRGB32: one word), the target one word off: the windows that take 16-byte accesses when aligned"""
    clip = Clip(torch, fmt, *source(fmt, 48), src_off=src_off * (4 if fmt == SC.P.XRGB32 else 1))
    for win in WINDOWS:
        clip.check(torch, hip, 0, 1, win, (5, 2, TC.AREA), dst_off=dst_off)
        clip.check(torch, hip, 0, 1, win, (4, 1, TC.NEAREST), 1, 2, dst_off=dst_off)


def test_bits_24_to_31_are_not_read_and_come_out_zero(torch, hip):
    raw, packed = source(SC.P.XRGB32, 48)
    high = (raw.view(np.uint32) | np.uint32(0x7E000000)).view(np.uint8)
    for rate in ((1, 1, TC.AREA), (1, 1, TC.NEAREST), (3, 2, TC.AREA), (2, 5, TC.NEAREST)):
        Clip(torch, SC.P.XRGB32, high, packed).check(torch, hip, 0, 1, WINDOWS[0], rate)
    Clip(torch, SC.P.RGBA32, *source(SC.P.RGBA32, 48)).check(torch, hip, 0, 1, WINDOWS[1], (1, 1, TC.AREA))


def test_a_flat_region_keeps_its_pixels(torch, hip):
    for fmt in (RGB24, Y.NV12):
        clip = Clip(torch, fmt, *source(fmt, 48))
        rows, cols = TC.FLAT
        win = (cols.start, rows.start, cols.stop - cols.start, rows.stop - rows.start)
        for rate in ((7, 3, TC.AREA), (13, 1, TC.AREA)):
            rc, got, guards = clip.run(torch, hip, 0, 1, N, win, rate, 0, TC.length(N, *rate[:2]))
            assert rc == 0 and guards and (got == clip.packed[0][TC.FLAT]).all()


def test_the_accumulators_hold_65535_taps_of_255(torch, hip):
    """65 535 frames of 16 x 4 XRGB32, all 0x00FFFFFF (4.2 MB): at 65535 : 1 the one output frame sums 65535 * 255 per channel and comes out
    white; at 65535 : 65534 the first and the last output frame against numpy"""
    n = 65535
    white = TC.white_clip(n, 4, 16)
    clip = Clip(torch, SC.P.XRGB32, white.view(np.uint8).reshape(n, -1), white)
    rc, got, guards = clip.run(torch, hip, 0, 1, n, (0, 0, 16, 4), (65535, 1, TC.AREA), 0, 1)
    assert rc == 0 and guards and got.shape == (1, 4, 16) and (got == 0x00FFFFFF).all()
    for j in (0, 65533):
        rc, got, guards = clip.run(torch, hip, 0, 1, n, (0, 0, 16, 4), (65535, 65534, TC.AREA), j, 1)
        assert rc == 0 and guards and (got == TC.resample(white, 65535, 65534, TC.AREA, j, 1)).all() and (got == 0x00FFFFFF).all()


def test_long_sums_of_moving_pixels(torch, hip):
    """600 frames of 24 x 2 RGB24 at 600 : 1 and 599 : 2: sums of many different taps, and a tap range per output frame that is long"""
    raw, packed = TC.moving_clip(RGB24, 600, 2, 24, 470)
    clip = Clip(torch, RGB24, raw, packed)
    for rate in ((600, 1, TC.AREA), (599, 2, TC.AREA), (300, 1, TC.NEAREST)):
        clip.check(torch, hip, 0, 1, (0, 0, 0, 0), rate)
        clip.check(torch, hip, 0, 1, (1, 0, 17, 2), rate)


def test_more_output_frames_than_the_grid_holds(torch, hip):
    """7 frames of 4 x 2 RGB24 at 1 : 10001 NEAREST: 70 007 output frames, more than the 65535 a launch spreads over its grid, so the
    last are reached on the second trip round the kernel's frame loop only"""
    raw, packed = TC.moving_clip(RGB24, 7, 2, 4, 480)
    clip = Clip(torch, RGB24, raw, packed)
    rc, got, guards = clip.run(torch, hip, 0, 1, 7, (1, 0, 3, 2), (1, 10001, TC.NEAREST), 0, 70007)
    assert rc == 0 and guards
    assert (got == np.repeat(packed[:, :, 1:4], 10001, axis=0)).all()


def test_many_blocks_per_frame(torch, hip):
    """9 frames of 1024 x 64 NV12 at stride 2, a 1001 x 61 window at an even and at an odd offset: several workgroups a frame, the last
    of them part empty"""
    raw = VS.raw_clip(Y.NV12, 9, 64, 1024, 490)
    clip = Clip(torch, Y.NV12, raw, VS.packed(Y.NV12, raw, 1024, 64))
    for x, y in ((16, 2), (3, 1)):
        clip.check(torch, hip, 1, 2, (x, y, 1001, 61), (3, 2, TC.AREA))


A52 = (5, 2, TC.AREA)
REFUSED = {"a-tap-behind-the-clip": dict(n_frames=12), "a-strided-view-behind-the-clip": dict(first=1, step=2, view_len=7), "rate-src-0": dict(rate=(0, 2, TC.AREA)),
           "rate-dst-0": dict(rate=(5, 0, TC.NEAREST)), "area-raises-the-rate": dict(rate=(2, 5, TC.AREA)), "rate-not-reduced": dict(rate=(10, 4, TC.AREA)),
           "rate-above-65535": dict(rate=(65537, 2, TC.AREA)), "filter-0": dict(rate=(5, 2, 0)), "filter-3": dict(rate=(5, 2, 3)),
           "frames-behind-the-result": dict(j0=4, count=2), "j0-that-wraps": dict(j0=0xFFFFFFFF, count=2), "null-source": dict(src=False), "null-target": dict(dst=False),
           "step-0": dict(step=0), "window-past-the-right-edge": dict(win=(41, 0, 8, 2)), "window-height-0": dict(win=(0, 0, 8, 0)), "x-that-wraps": dict(win=(0xFFFFFFFC, 0, 8, 2)),
           "format-0": dict(fmt=0), "format-6": dict(fmt=6), "unknown-yuv-flag": dict(fmt=Y.NV12 | 0x400)}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_every_refusal_touches_nothing(torch, hip, name):
    clip = Clip(torch, RGB24, *source(RGB24, 48))
    a = dict(dict(first=0, step=1, view_len=N, win=(8, 0, 8, 2), rate=A52, j0=0, count=2), **REFUSED[name])
    rc, got, guards = clip.run(torch, hip, a.pop("first"), a.pop("step"), a.pop("view_len"), a.pop("win"), a.pop("rate"), a.pop("j0"), a.pop("count"), **a)
    assert rc != 0 and hip.L.agmv_hip_last_error()
    assert guards and (got == FILL).all()
    hip.check()


def test_an_odd_yuv_frame_is_refused_and_count_zero_launches_nothing(torch, hip):
    clip = Clip(torch, RGB24, *source(RGB24, 48))
    buf = torch.full((256,), FILL, dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fmt, sw, sh in ((Y.NV12, 47, 24), (Y.I420, 48, 23)):
        assert hip.L.agmv_hip_time_frames_async(hip.ctx, fmt, clip.ptr, sw, sh, 4, 0, 1, 4, 0, 0, 8, 2, 2, 1, TC.AREA, 0, 2, buf.data_ptr(), s) != 0
        assert b"even" in hip.L.agmv_hip_last_error()
    rc, got, guards = clip.run(torch, hip, 0, 1, N, (8, 0, 8, 2), A52, 3, 0)
    assert rc == 0 and guards and got.size == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint32) == FILL).all()
    hip.check()


def test_the_wrapper_returns_the_frames(torch, hip):
    raw, packed = source(RGB24, 48)
    rgb = Clip(torch, RGB24, raw, packed)
    got = hip.time_frames("rgb24", rgb.dev, 48, SH, N, 1, 2, 6, 1, 1, 33, 5, (3, 2))
    assert tuple(got.shape) == (4, 5, 33) and (got.cpu().numpy().view(np.uint32) == TC.resample(packed[1::2, 1:6, 1:34], 3, 2, TC.AREA)).all()
    got = hip.time_frames("rgb24", rgb.dev, 48, SH, N, 0, 1, N, 0, 0, 48, SH, (2, 5), time="nearest", j0=30, count=2)
    assert (got.cpu().numpy().view(np.uint32) == TC.resample(packed, 2, 5, TC.NEAREST, 30, 2)).all()
    fmt = Y.NV12 | Y.BT709
    nraw, npacked = TC.moving_clip(fmt, N, SH, 48, 461)
    nv = Clip(torch, fmt, nraw, npacked)
    got = hip.time_frames("nv12", nv.dev, 48, SH, N, 0, 1, N, 17, 1, 15, 5, (13, 1), yuv="bt709")
    assert tuple(got.shape) == (1, 5, 15) and (got.cpu().numpy().view(np.uint32) == TC.resample(npacked[:, 1:6, 17:32], 13, 1, TC.AREA)).all()
    with pytest.raises(ValueError, match="src"):
        hip.time_frames("rgb24", rgb.dev[:12 * 48 * SH * 3], 48, SH, N, 0, 1, N, 0, 0, 8, 8, (2, 1))
    with pytest.raises(ValueError, match="time"):
        hip.time_frames("rgb24", rgb.dev, 48, SH, N, 0, 1, N, 0, 0, 8, 8, (2, 1), time="box")
    with pytest.raises(ValueError, match="rate"):
        hip.time_frames("rgb24", rgb.dev, 48, SH, N, 0, 1, N, 0, 0, 8, 8, (0, 1))
    with pytest.raises(RuntimeError, match="reduced"):
        hip.time_frames("rgb24", rgb.dev, 48, SH, N, 0, 1, N, 0, 0, 8, 8, (4, 2), count=1)
    with pytest.raises(RuntimeError, match="outside the clip"):
        hip.time_frames("rgb24", rgb.dev, 48, SH, N, 4, 3, 5, 0, 0, 8, 8, (2, 1))
