"""agmv_hip_view_source_async (k_view_src; XRGB32: k_view) against the numpy statement of tests/view_source_cases.py, word for word:
every step-th frame of a clip in each of the seven layouts and a window of each, as the packed XRGB32 words the whole-clip
converters give, between guard words.  The windows start and end on, one before and one behind the 16-pixel groups of a lane, at
even and odd rows, so every layout takes its 16-byte loads (48 pixels wide: all; 36 and 68: RGBA32 alone), its 16-byte stores and
its element-by-element forms, and NV12 / I420 are cut at odd offsets and sizes.  Source and target are also put off their 16-byte
boundaries.  A view of more frames than one launch spreads over its grid takes a second trip.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import scale_cases as SC
import view_cases as V
import view_source_cases as VS
import yuv_cases as Y

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0x5A5A5A5A                     # words on either side of the target (256 bytes: the alignment stays), and what they hold
N = 7
SOURCES = [(36, 10), (48, 6), (68, 12)]          # (w, h)
XS, WIDTHS, YS, HEIGHTS = (0, 1, 15, 16, 17), (1, 4, 15, 16, 17, 33), (0, 1, 3), (1, 2, 5)
SELECTIONS = [(0, 1, 0), (2, 1, 3), (1, 2, 0), (0, 3, 2), (6, 5, 0), (3, 4, 9)]     # (first, step, count) of an AGMV_VIEW: count 0 is "to the end"
FORMATS = SC.LAYOUTS
FLAGGED = [f | flags for f in SC.YUV_PLAIN for flags in VS.YUV_FLAGS if flags]      # both matrices and both ranges, on one shape
GRID_FRAMES = 65535                              # the frames one launch spreads over its grid


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


def call(torch, hip, fmt, d_src, sw, sh, first, step, count, x, y, w, h, d_dst):
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return hip.L.agmv_hip_view_source_async(hip.ctx, fmt, d_src, sw, sh, first, step, count, x, y, w, h, d_dst, s)


class Clip:
    """a source clip on the device `src_off` bytes behind a 16-byte boundary, and the XRGB32 clip it stands for on the host"""

    def __init__(self, torch, fmt, n, sw, sh, seed, src_off=0, raw=None):
        self.fmt, self.n, self.sw, self.sh = fmt, n, sw, sh
        raw = VS.raw_clip(fmt, n, sh, sw, seed) if raw is None else raw
        self.packed = SC.to_packed(fmt, raw, sw, sh)
        self.dev = torch.zeros(raw.size + 32, dtype=torch.uint8, device="cuda")
        assert self.dev.data_ptr() % 16 == 0
        self.dev[src_off:src_off + raw.size] = torch.from_numpy(raw.reshape(-1)).cuda()
        self.ptr = self.dev.data_ptr() + src_off

    def run(self, torch, hip, first, step, count, x, y, w, h, dst_off=0):
        """-> (return value, the target's words [count, h, w], whether every word around it kept the fill)"""
        buf = torch.full((GUARD + dst_off + count * w * h + GUARD,), FILL, dtype=torch.int32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        rc = call(torch, hip, self.fmt, self.ptr, self.sw, self.sh, first, step, count, x, y, w, h, buf.data_ptr() + 4 * (GUARD + dst_off))
        torch.cuda.synchronize()
        host = buf.cpu().numpy().view(np.uint32)
        lo, hi = GUARD + dst_off, GUARD + dst_off + count * w * h
        return rc, host[lo:hi].reshape(count, h, w), bool((host[:lo] == FILL).all() and (host[hi:] == FILL).all())

    def check(self, torch, hip, sel, x, y, w, h, dst_off=0):
        first, step, count = sel
        length = V.length(first, step, count, self.n)
        rc, got, guards = self.run(torch, hip, first, step, length, x, y, w, h, dst_off)
        exp = V.view(self.packed, first, count, step, x, y, w, h)
        what = (SC.fmt_name(self.fmt), (self.sw, self.sh), sel, (x, y, w, h), dst_off)
        assert rc == 0, (what, hip.L.agmv_hip_last_error())
        assert exp.shape == (length, h, w) and length >= 1
        assert (got == exp).all(), (what, np.argwhere(got != exp)[:4])
        assert guards, (what, "guard words written")


def windows(sw, sh):
    return [(x, y, w, h) for x in XS for w in WIDTHS if x + w <= sw for y in YS for h in HEIGHTS if y + h <= sh]


@pytest.mark.parametrize("size", SOURCES, ids=["%dx%d" % s for s in SOURCES])
@pytest.mark.parametrize("fmt", FORMATS, ids=[SC.fmt_name(f) for f in FORMATS])
def test_every_window_equals_numpy(torch, hip, fmt, size):
    """every window of the lists that fits the source, the six selections taken in turn (each meets every x, width, y and height)"""
    sw, sh = size
    clip = Clip(torch, fmt, N, sw, sh, 100 + sw)
    wins = windows(sw, sh)
    assert len(wins) >= 200 and any(x & 1 and y & 1 and w & 1 and h & 1 for x, y, w, h in wins)
    for k, win in enumerate(wins):
        clip.check(torch, hip, SELECTIONS[(k + k // len(SELECTIONS)) % len(SELECTIONS)], *win)


@pytest.mark.parametrize("sel", SELECTIONS, ids=["%d-%d-%d" % s for s in SELECTIONS])
def test_every_selection_on_every_layout(torch, hip, sel):
    for fmt in FORMATS:
        clip = Clip(torch, fmt, N, 48, 6, 150)
        for win in ((0, 0, 48, 6), (16, 0, 32, 6), (16, 0, 16, 2), (1, 1, 33, 5), (17, 3, 15, 1)):
            clip.check(torch, hip, sel, *win)


@pytest.mark.parametrize("fmt", FLAGGED, ids=[SC.fmt_name(f) for f in FLAGGED])
def test_both_matrices_and_both_ranges(torch, hip, fmt):
    clip = Clip(torch, fmt, N, 48, 6, 160)
    for k, win in enumerate(windows(48, 6)):
        clip.check(torch, hip, SELECTIONS[k % len(SELECTIONS)], *win)


@pytest.mark.parametrize("src_off,dst_off", [(0, 1), (1, 0), (1, 1)], ids=["target-off", "source-off", "both-off"])
@pytest.mark.parametrize("fmt", FORMATS, ids=[SC.fmt_name(f) for f in FORMATS])
def test_clips_off_their_16_byte_boundary_give_the_same_words(torch, hip, fmt, src_off, dst_off):
    """the source 1 byte off (XRGB32: one word), the target one word off: the windows that take 16-byte accesses when aligned"""
    clip = Clip(torch, fmt, N, 48, 6, 170, src_off * (4 if fmt == SC.P.XRGB32 else 1))
    for k, win in enumerate([(x, y, w, h) for x in (0, 16, 17) for w in (4, 16, 17, 32) if x + w <= 48 for y in (0, 1) for h in (2, 5)]):
        clip.check(torch, hip, SELECTIONS[k % len(SELECTIONS)], *win, dst_off=dst_off)


def test_xrgb32_words_are_copied_as_they_are(torch, hip):
    pix = V.clip(N, 6, 48, 21)                                              # bits 24 .. 31 set
    clip = Clip(torch, SC.P.XRGB32, N, 48, 6, 0, raw=pix.view(np.uint8).reshape(N, -1))
    rc, got, guards = clip.run(torch, hip, 1, 2, 3, 16, 1, 17, 5)
    assert rc == 0 and guards and (got == V.view(pix, 1, 3, 2, 16, 1, 17, 5)).all() and (got >> 24 == 0x7E).all()


def test_alpha_is_not_copied(torch, hip):
    clip = Clip(torch, SC.P.RGBA32, N, 48, 6, 180)
    rc, got, guards = clip.run(torch, hip, 0, 1, N, 0, 0, 48, 6)
    assert rc == 0 and guards and (got == clip.packed).all() and (got >> 24 == 0).all()


def test_count_zero_launches_nothing(torch, hip):
    for fmt in (SC.P.RGB24, Y.NV12, SC.P.XRGB32):
        clip = Clip(torch, fmt, N, 48, 6, 190)
        rc, got, guards = clip.run(torch, hip, 0, 1, 0, 16, 0, 16, 2)
        assert rc == 0 and guards and got.size == 0


RGB24 = SC.P.RGB24
REFUSED = {"null-source": dict(src=None), "null-target": dict(dst=None), "source-width-0": dict(sw=0), "source-height-0": dict(sh=0),
           "window-width-0": dict(w=0), "window-height-0": dict(h=0), "step-0": dict(step=0), "window-past-the-right-edge": dict(x=41),
           "window-past-the-bottom": dict(y=5), "x-that-wraps": dict(x=0xFFFFFFFC), "y-that-wraps": dict(y=0xFFFFFFFF), "window-wider-than-the-frame": dict(x=0, w=49),
           "format-0": dict(fmt=0), "format-6": dict(fmt=6), "flags-on-a-byte-layout": dict(fmt=RGB24 | Y.BT709), "unknown-yuv-flag": dict(fmt=Y.NV12 | 0x400),
           "nv12-of-odd-width": dict(fmt=Y.NV12, sw=47), "i420-of-odd-height": dict(fmt=Y.I420, sh=5, h=1, y=0)}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_every_refusal_touches_nothing(torch, hip, name):
    clip = Clip(torch, RGB24, N, 48, 6, 200)
    buf = torch.full((N * 48 * 6 + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda")
    a = dict(dict(fmt=RGB24, src=clip.ptr, sw=48, sh=6, first=0, step=1, count=2, x=8, y=0, w=8, h=2, dst=buf.data_ptr() + 4 * GUARD), **REFUSED[name])
    assert call(torch, hip, a["fmt"], a["src"], a["sw"], a["sh"], a["first"], a["step"], a["count"], a["x"], a["y"], a["w"], a["h"], a["dst"]) != 0
    assert hip.L.agmv_hip_last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint32) == FILL).all()
    hip.check()


def test_the_wrapper_returns_the_view(torch, hip):
    rgb = Clip(torch, RGB24, N, 48, 6, 210)
    got = hip.view_source("rgb24", rgb.dev, 48, 6, 2, 3, 2, 1, 1, 33, 5)
    assert tuple(got.shape) == (2, 5, 33) and (got.cpu().numpy().view(np.uint32) == V.view(rgb.packed, 2, 2, 3, 1, 1, 33, 5)).all()
    nv = Clip(torch, Y.NV12 | Y.BT709, N, 48, 6, 211)
    got = hip.view_source("nv12", nv.dev, 48, 6, 0, 2, 4, 17, 1, 15, 5, yuv="bt709")
    assert (got.cpu().numpy().view(np.uint32) == V.view(nv.packed, 0, 4, 2, 17, 1, 15, 5)).all()
    x32 = torch.from_numpy(V.clip(N, 6, 48, 22).view(np.int32)).cuda()
    got = hip.view_source("xrgb32", x32, 48, 6, 1, 1, 2, 4, 0, 8, 6)
    assert (got.cpu().numpy() == x32.cpu().numpy()[1:3, :, 4:12]).all()
    with pytest.raises(ValueError, match="src"):
        hip.view_source("rgb24", rgb.dev[:N * 48 * 6 * 3], 48, 6, 2, 3, 3, 1, 1, 33, 5)      # frame 8 of 7
    with pytest.raises(ValueError, match="step"):
        hip.view_source("rgb24", rgb.dev, 48, 6, 0, 0, 1, 1, 1, 5, 5)
    with pytest.raises(ValueError, match="yuv="):
        hip.view_source("rgb24", rgb.dev, 48, 6, 0, 1, 1, 1, 1, 5, 5, yuv="bt709")
    with pytest.raises(RuntimeError, match="window"):
        hip.view_source("rgb24", rgb.dev, 48, 6, 0, 1, 1, 44, 1, 5, 5)


def test_more_frames_than_the_grid_holds(torch, hip):
    """70 000 frames of 4 x 2 RGB24, a 3 x 2 window of each: a launch spreads at most 65535 frames over its grid, so the last 4465 are
    reached on the second trip round the kernel's frame loop only"""
    n = 70000
    assert n > GRID_FRAMES
    clip = Clip(torch, RGB24, n, 4, 2, 220)
    rc, got, guards = clip.run(torch, hip, 0, 1, n, 1, 0, 3, 2)
    assert rc == 0 and guards
    assert (got == clip.packed[:, :, 1:4]).all()


def test_many_blocks_per_frame(torch, hip):
    """24 frames of 1024 x 64 NV12 at stride 3, a 1001 x 61 window at an even and at an odd offset: several workgroups a frame, the
    last of them part empty"""
    clip = Clip(torch, Y.NV12, 24, 1024, 64, 230)
    for x, y in ((16, 2), (3, 1)):
        rc, got, guards = clip.run(torch, hip, 1, 3, 8, x, y, 1001, 61)
        assert rc == 0 and guards
        assert (got == V.view(clip.packed, 1, 8, 3, x, y, 1001, 61)).all()
