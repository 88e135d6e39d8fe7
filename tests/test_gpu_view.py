"""agmv_hip_view_frames_async (k_view) against the numpy statement of tests/view_cases.py, word for word: every step-th frame of a
packed XRGB32 clip and a window of each, copied with bits 24 .. 31 as they are, between guard words.  The windows take each of the
kernel's four forms (16-byte loads and stores, either alone, neither), the source and the destination are also put one element off
their 16-byte boundary, and the sizes the index arithmetic can get wrong are here: a source offset past 2^32 bytes and a view of
more frames than one launch spreads over its grid.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import view_cases as V

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0x5A5A5A5A                     # words on either side of the destination (256 bytes: the alignment stays), and what they hold
N, SH, SW = 9, 12, 20
# (x, y, w, h) in the 20 x 12 source, and the form the kernel takes for it with both clips on a 16-byte boundary
WINDOWS = {"full-frame": (0, 0, 20, 12), "wide": (4, 0, 8, 12), "odd": (1, 3, 5, 7), "aligned-start-narrow": (4, 2, 6, 3), "last-pixel": (19, 11, 1, 1)}
GRID_FRAMES = 65535                              # VIEW_GRID_FRAMES of agmv_clip_hip.hip: the frames one launch spreads over its grid


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


@pytest.fixture(scope="module")
def clip():
    return V.clip(N, SH, SW, 7)


def call(torch, hip, d_src, sw, sh, first, step, count, x, y, w, h, d_dst):
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return hip.L.agmv_hip_view_frames_async(hip.ctx, d_src, sw, sh, first, step, count, x, y, w, h, d_dst, s)


def run(torch, hip, pix, first, step, count, x, y, w, h, src_off=0, dst_off=0):
    """-> (return value, the destination's words [count, h, w], whether every word around it kept the fill)"""
    n, sh, sw = pix.shape
    src = torch.zeros(pix.size + 4, dtype=torch.int32, device="cuda")
    src[src_off:src_off + pix.size] = torch.from_numpy(pix.view(np.int32).reshape(-1)).cuda()
    buf = torch.full((GUARD + dst_off + count * w * h + GUARD,), FILL, dtype=torch.int32, device="cuda")
    assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    rc = call(torch, hip, src.data_ptr() + 4 * src_off, sw, sh, first, step, count, x, y, w, h, buf.data_ptr() + 4 * (GUARD + dst_off))
    torch.cuda.synchronize()
    host = buf.cpu().numpy().view(np.uint32)
    lo, hi = GUARD + dst_off, GUARD + dst_off + count * w * h
    return rc, host[lo:hi].reshape(count, h, w), bool((host[:lo] == FILL).all() and (host[hi:] == FILL).all())


@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_every_window_step_and_start_equals_numpy(torch, hip, clip, window):
    x, y, w, h = WINDOWS[window]
    for first in (0, 8):
        for step in (1, 2, 3, 8):
            for count in sorted({1, (N - 1 - first) // step + 1}):
                rc, got, guards = run(torch, hip, clip, first, step, count, x, y, w, h)
                exp = V.view(clip, first, count, step, x, y, w, h)
                assert rc == 0, hip.L.agmv_hip_last_error()
                assert got.shape == exp.shape and (got == exp).all(), (window, first, step, count, np.argwhere(got != exp)[:4])
                assert guards, (window, first, step, count, "guard words written")
                assert (got >> 24 == 0x7E).all()


@pytest.mark.parametrize("src_off,dst_off", [(1, 0), (0, 1), (1, 1), (3, 2)])
@pytest.mark.parametrize("window", ["wide", "full-frame"])
def test_a_clip_off_its_16_byte_boundary_gives_the_same_words(torch, hip, clip, window, src_off, dst_off):
    x, y, w, h = WINDOWS[window]
    rc, got, guards = run(torch, hip, clip, 1, 2, 4, x, y, w, h, src_off, dst_off)
    assert rc == 0 and guards
    assert (got == V.view(clip, 1, 4, 2, x, y, w, h)).all()


def test_count_zero_launches_nothing(torch, hip, clip):
    rc, got, guards = run(torch, hip, clip, 0, 1, 0, 4, 0, 8, 12)
    assert rc == 0 and guards and got.size == 0
    buf = torch.full((256,), FILL, dtype=torch.int32, device="cuda")
    src = torch.from_numpy(clip.view(np.int32)).cuda()
    assert call(torch, hip, src.data_ptr(), SW, SH, 0, 1, 0, 4, 0, 8, 12, buf.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint32) == FILL).all()


REFUSED = {"null-source": dict(src=None), "null-destination": dict(dst=None), "source-width-0": dict(sw=0), "source-height-0": dict(sh=0),
           "window-width-0": dict(w=0), "window-height-0": dict(h=0), "step-0": dict(step=0), "window-past-the-right-edge": dict(x=13),
           "window-past-the-bottom": dict(y=1), "x-that-wraps": dict(x=0xFFFFFFFC), "y-that-wraps": dict(y=0xFFFFFFFF), "window-wider-than-the-frame": dict(x=0, w=21)}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_every_refusal_touches_nothing(torch, hip, clip, name):
    src = torch.from_numpy(clip.view(np.int32)).cuda()
    buf = torch.full((N * SH * SW + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda")
    a = dict(dict(src=src.data_ptr(), sw=SW, sh=SH, first=0, step=1, count=2, x=4, y=0, w=8, h=12, dst=buf.data_ptr() + 4 * GUARD), **REFUSED[name])
    assert call(torch, hip, a["src"], a["sw"], a["sh"], a["first"], a["step"], a["count"], a["x"], a["y"], a["w"], a["h"], a["dst"]) != 0
    assert hip.L.agmv_hip_last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint32) == FILL).all()
    hip.check()


def test_the_wrapper_returns_the_view(torch, hip, clip):
    src = torch.from_numpy(clip.view(np.int32)).cuda()
    got = hip.view_frames_async(src, SW, SH, 2, 3, 3, 1, 3, 5, 7)
    assert tuple(got.shape) == (3, 7, 5) and (got.cpu().numpy().view(np.uint32) == V.view(clip, 2, 3, 3, 1, 3, 5, 7)).all()
    with pytest.raises(ValueError, match="src"):
        hip.view_frames_async(src, SW, SH, 2, 3, 4, 1, 3, 5, 7)                    # frame 11 of 9
    with pytest.raises(ValueError, match="step"):
        hip.view_frames_async(src, SW, SH, 0, 0, 1, 1, 3, 5, 7)
    with pytest.raises(RuntimeError, match="window"):
        hip.view_frames_async(src, SW, SH, 0, 1, 1, 16, 3, 5, 7)


def test_source_offset_past_2_to_32_bytes(torch, hip):
    """5 frames of 16384 x 16384 that are never filled but for the window's rows of frame 4: a product of the source index held in
    32 bits reads elsewhere"""
    sw = sh = 16384
    first, x, y, w, h = 4, 8, 16378, 24, 5
    assert first * sw * sh * 4 >= 1 << 32 and (first * sw * sh + y * sw + x) * 4 > 1 << 32      # the frame alone starts 2^32 bytes in
    src = torch.empty((5, sh, sw), dtype=torch.int32, device="cuda")
    rows = V.clip(1, h, sw, 11)[0]
    src[first, y:y + h] = torch.from_numpy(rows.view(np.int32)).cuda()
    buf = torch.full((GUARD + w * h + GUARD,), FILL, dtype=torch.int32, device="cuda")
    assert call(torch, hip, src.data_ptr(), sw, sh, first, 1, 1, x, y, w, h, buf.data_ptr() + 4 * GUARD) == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy().view(np.uint32)
    assert (host[GUARD:-GUARD].reshape(h, w) == rows[:, x:x + w]).all()
    assert (host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all()


def test_more_frames_than_the_grid_holds(torch, hip):
    """65541 frames of 4 x 2, every second one, a 3 x 1 window: a launch spreads at most 65535 frames over its grid, so six of them are
    reached on the second trip round the kernel's frame loop only"""
    n, count = 2 * (GRID_FRAMES + 6), GRID_FRAMES + 6
    assert count > GRID_FRAMES
    pix = V.clip(n, 2, 4, 13)
    rc, got, guards = run(torch, hip, pix, 1, 2, count, 1, 1, 3, 1)
    assert rc == 0 and guards
    assert (got == V.view(pix, 1, count, 2, 1, 1, 3, 1)).all()


def test_many_blocks_per_frame(torch, hip):
    """64 frames of 512 x 512 at stride 3, a 500 x 509 window: 250 workgroups a frame, the last of them part empty"""
    pix = V.clip(64, 512, 512, 17)
    rc, got, guards = run(torch, hip, pix, 1, 3, 21, 8, 2, 500, 509)
    assert rc == 0 and guards
    assert (got == V.view(pix, 1, 21, 3, 8, 2, 500, 509)).all()
