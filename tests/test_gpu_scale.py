"""agmv_hip_scale_area_dev, the exact box-filter downscale of a clip in any of the seven layouts (AGMV_SCALE_AREA of include/agmv.h),
through AgmvHip against the numpy statement of the rule (tests/scale_cases.py).  Everything is exact: the kernel sums integers.
A lane takes 16 consecutive pixels of a source row, with 16-byte loads where the clip's frames lie on 16-byte boundaries (YUV:
and the width is a multiple of 16) and byte by byte otherwise and at a row's head and tail; 1024 target columns share one
accumulator tile; the work items are walked with a grid stride.  The shapes hold each of these paths and their edges, the byte
offset 1 takes an aligned clip to the byte-wise path.  Where sw * dw leaves 32 bits a lane forms its position in 64: shapes on either
side of that, stated by prefix sums (SC.scale_area_streamed).  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import pixfmt_cases as P
import scale_cases as SC
import yuv_cases as Y

pytestmark = pytest.mark.gpu

GUARD = 64
ALL_FORMATS = SC.LAYOUTS + SC.YUV_709F
IDS = [SC.fmt_name(f) for f in ALL_FORMATS]


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


def source(torch, fmt, raw, off=0):
    """the clip `raw` (uint8 [n, frame bytes]) on the device, `off` bytes behind a 16-byte boundary, as the tensor scale_area_dev takes"""
    raw = np.ascontiguousarray(raw, np.uint8).reshape(-1)
    if fmt == P.XRGB32:
        assert off == 0
        return torch.from_numpy(raw.view(np.int32)).cuda()
    buf = torch.empty(off + raw.size + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + raw.size]
    view.copy_(torch.from_numpy(raw))
    return view


def run(torch, hip, fmt, raw, sw, sh, dw, dh, off=0):
    """-> (uint32 [n, dh, dw] from the device, whether the guard words on either side of the destination kept their value)"""
    n = raw.shape[0]
    buf = torch.full((GUARD + n * dw * dh + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out = buf[GUARD:GUARD + n * dw * dh]
    got = hip.scale_area_dev(fmt, source(torch, fmt, raw, off), sw, sh, n, dw, dh, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    return host[GUARD:-GUARD].view(np.uint32).reshape(n, dh, dw), bool((host[:GUARD] == 0x5A5A5A5A).all() and (host[-GUARD:] == 0x5A5A5A5A).all())


def check(torch, hip, fmt, raw, sw, sh, dw, dh, offsets=(0,), statement=SC.scale_area):
    exp = statement(SC.to_packed(fmt, raw, sw, sh), dw, dh)
    for off in offsets:
        got, guards = run(torch, hip, fmt, raw, sw, sh, dw, dh, off)
        assert (got >> 24 == 0).all(), (sw, sh, dw, dh, off, "top byte")
        assert (got == exp).all(), (sw, sh, dw, dh, off, np.argwhere(got != exp)[:4], got[got != exp][:4], exp[got != exp][:4])
        assert guards, (sw, sh, dw, dh, off, "guard words written")


def contents(fmt, n, sw, sh, seed):
    fb = SC.frame_bytes(fmt, sw, sh)
    return [np.random.default_rng(seed).integers(0, 256, (n, fb), dtype=np.uint8), np.full((n, fb), 0xFF, np.uint8)]


@pytest.mark.parametrize("shape", SC.STARRED, ids=[SC.shape_id(s) for s in SC.STARRED])
@pytest.mark.parametrize("fmt", ALL_FORMATS, ids=IDS)
def test_every_layout_equals_numpy(torch, hip, fmt, shape):
    """3 frames, random and all-0xFF bytes; at byte offset 1 the 16-byte loads are off"""
    sw, sh, dw, dh = shape
    for raw in contents(fmt, 3, sw, sh, fmt * 1000 + sw):
        check(torch, hip, fmt, raw, sw, sh, dw, dh, offsets=(0,) if fmt == P.XRGB32 else (0, 1))


@pytest.mark.parametrize("shape", SC.MORE, ids=[SC.shape_id(s) for s in SC.MORE])
@pytest.mark.parametrize("fmt", SC.LAYOUTS, ids=[SC.fmt_name(f) for f in SC.LAYOUTS])
def test_edges_of_the_walk_equal_numpy(torch, hip, fmt, shape):
    sw, sh, dw, dh = shape
    for raw in contents(fmt, 2, sw, sh, fmt * 1000 + dw):
        check(torch, hip, fmt, raw, sw, sh, dw, dh)


@pytest.mark.parametrize("fmt", SC.YUV_709F, ids=[SC.fmt_name(f) for f in SC.YUV_709F])
@pytest.mark.parametrize("shape", [(7, 5, 3, 2), (64, 48, 32, 24)], ids=SC.shape_id)
def test_yuv_bt709_full_range(torch, hip, fmt, shape):
    sw, sh, dw, dh = shape
    raw = np.random.default_rng(9).integers(0, 256, (3, SC.frame_bytes(fmt, sw, sh)), dtype=np.uint8)
    check(torch, hip, fmt, raw, sw, sh, dw, dh, offsets=(0, 1, 16))
    plain = SC.scale_area(SC.to_packed(fmt & 0xFF, raw, sw, sh), dw, dh)
    assert (plain != SC.scale_area(SC.to_packed(fmt, raw, sw, sh), dw, dh)).any()               # the flags reach the reader


def test_the_accumulator_bound(torch, hip):
    """sw * sh = 2^24: one all-0xFFFFFF XRGB32 frame sums to 255 * 2^22 * 4 per target pixel and channel, a random RGB8P frame to the block means"""
    white = np.full((1, 4096 * 4096), 0xFFFFFF, np.uint32).view(np.uint8).reshape(1, -1)
    got, guards = run(torch, hip, P.XRGB32, white, 4096, 4096, 4, 4)
    assert (got == 0xFFFFFF).all() and guards
    white[:] = 0xFF                                                                             # bits >= 24 set: they are no pixels
    got, _ = run(torch, hip, P.XRGB32, white, 4096, 4096, 4, 4)
    assert (got == 0xFFFFFF).all()
    raw = np.random.default_rng(5).integers(0, 256, (1, 3 * 4096 * 4096), dtype=np.uint8)
    got, guards = run(torch, hip, P.RGB8P, raw, 4096, 4096, 4, 4)
    # an integer factor: the mean of each 1024 x 1024 block, rounded half up (numpy's int64 matrix product takes seconds at this size)
    sums = raw.reshape(3, 4, 1024, 4, 1024).sum(axis=(2, 4), dtype=np.int64)
    mean = ((sums + (1 << 19)) >> 20).astype(np.uint32)
    assert (got[0] == (mean[0] << 16 | mean[1] << 8 | mean[2])).all() and guards


# ---- a lane's position u = column * dw past 32 bits (SC.scale_area_streamed states these shapes; tests/test_scale_cpu.py proves it) ----
@pytest.mark.parametrize("shape,small", SC.WIDE_U, ids=[SC.shape_id(s) for s, _ in SC.WIDE_U])
@pytest.mark.parametrize("fmt", ALL_FORMATS, ids=IDS)
def test_either_side_of_the_largest_32_bit_position(torch, hip, fmt, shape, small):
    """2 frames of 65536 x 2 -> 65536 x 1 (sw * dw = 2^32, the 64-bit form) and -> 65535 x 1 (the largest 32-bit u); the byte
    layouts also at byte offset 1, so that the 16-byte loads and the byte reader both walk each form"""
    sw, sh, dw, dh = shape
    assert SC.area_small(shape) == small and abs(sw * dw - (1 << 32)) <= 65536
    raw = np.random.default_rng(fmt * 1000 + dw).integers(0, 256, (2, SC.frame_bytes(fmt, sw, sh)), dtype=np.uint8)
    offsets = (0, 1) if fmt in SC.BYTE_LAYOUTS and fmt != P.XRGB32 else (0,)
    check(torch, hip, fmt, raw, sw, sh, dw, dh, offsets=offsets, statement=SC.scale_area_streamed)


@pytest.mark.parametrize("fmt", SC.LAYOUTS, ids=[SC.fmt_name(f) for f in SC.LAYOUTS])
def test_forty_tiles_with_the_64_bit_position(torch, hip, fmt):
    (sw, sh, dw, dh), small = SC.WIDE_TILES
    assert SC.area_small((sw, sh, dw, dh)) == small and not small and (dw + 1023) // 1024 == 40
    raw = np.random.default_rng(fmt * 1000 + dw).integers(0, 256, (2, SC.frame_bytes(fmt, sw, sh)), dtype=np.uint8)
    check(torch, hip, fmt, raw, sw, sh, dw, dh, statement=SC.scale_area_streamed)


def test_the_accumulator_bound_with_the_64_bit_position(torch, hip):
    """sw * sh = 2^24 and sw * dw >= 2^32 in one frame of 4194304 x 4 -> 4099 x 3: five tiles, target rows astride source rows"""
    (sw, sh, dw, dh), small = SC.WIDE_BOUND
    assert SC.area_small((sw, sh, dw, dh)) == small and not small and sw * sh == SC.AREA_MAX_SOURCE and (dw + 1023) // 1024 == 5 and sh % dh
    white = np.full((1, 4 * sw * sh), 0xFF, np.uint8)                                           # bits >= 24 set: they are no pixels
    got, guards = run(torch, hip, P.XRGB32, white, sw, sh, dw, dh)
    assert (got == 0xFFFFFF).all() and guards
    raw = np.random.default_rng(17).integers(0, 256, (1, 3 * sw * sh), dtype=np.uint8)
    check(torch, hip, P.RGB24, raw, sw, sh, dw, dh, statement=SC.scale_area_streamed)


def test_more_frames_than_a_grid_holds(torch, hip):
    """70 000 frames of 8 x 8 RGB24 -> 4 x 4: 280 000 work items, every frame its own content"""
    raw = np.random.default_rng(11).integers(0, 256, (70000, 3 * 64), dtype=np.uint8)
    check(torch, hip, P.RGB24, raw, 8, 8, 4, 4)


def test_the_same_call_twice_gives_the_same_bytes(torch, hip):
    for fmt, (sw, sh, dw, dh) in ((P.RGB24, (1920, 18, 320, 4)), (Y.NV12, (1920, 18, 320, 4)), (P.RGBA32, (259, 3, 37, 1))):
        raw = np.random.default_rng(13).integers(0, 256, (4, SC.frame_bytes(fmt, sw, sh)), dtype=np.uint8)
        a, _ = run(torch, hip, fmt, raw, sw, sh, dw, dh)
        b, _ = run(torch, hip, fmt, raw, sw, sh, dw, dh)
        assert a.tobytes() == b.tobytes()


def test_error_returns_launch_nothing(torch, hip):
    src = torch.zeros(4 * 64 * 64, dtype=torch.uint8, device="cuda")
    dst = torch.full((64 * 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    call = hip.L.agmv_hip_scale_area_dev
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = [(0, 16, 16, 8, 8), (6, 16, 16, 8, 8), (15, 16, 16, 8, 8), (18, 16, 16, 8, 8), (2 | 0x100, 16, 16, 8, 8), (16 | 0x400, 16, 16, 8, 8),   # unknown formats
           (2, 0, 16, 8, 8), (2, 16, 0, 8, 8), (2, 16, 16, 0, 8), (2, 16, 16, 8, 0),                                                        # zero sizes
           (2, 16, 16, 17, 8), (2, 16, 16, 8, 17), (16, 16, 16, 32, 16),                                                                    # an upscale
           (2, 4097, 4096, 8, 8), (1, 1 << 24, 2, 8, 2)]                                                                                    # more than 2^24 source pixels
    for fmt, sw, sh, dw, dh in bad:
        assert call(hip.ctx, fmt, src.data_ptr(), sw, sh, 1, dw, dh, dst.data_ptr(), s) != 0, (fmt, sw, sh, dw, dh)
        assert hip.L.agmv_hip_last_error()
    assert call(None, 2, src.data_ptr(), 16, 16, 1, 8, 8, dst.data_ptr(), s) != 0                # no context
    assert call(hip.ctx, 2, src.data_ptr(), 16, 16, 0, 8, 8, dst.data_ptr(), s) == 0             # no frames: nothing to do
    torch.cuda.synchronize()
    assert bool((dst == 0x5A5A5A5A).all())
    with pytest.raises(ValueError):
        hip.scale_area_dev("rgb24", src, 16, 16, 1, 8, 8, yuv="bt709")
    with pytest.raises(RuntimeError, match="area scale"):
        hip.scale_area_dev("rgb24", src, 16, 16, 1, 32, 8)
