"""The kernels that read and write a clip in 8-bit YUV 4:2:0 (AGMV_PIXFMT_NV12 / AGMV_PIXFMT_I420 with the BT.709 and full-range
flags), through AgmvHip, against the numpy statement of the definition (tests/yuv_cases.py): agmv_hip_yuv_to_xrgb_dev /
_from_xrgb_dev, agmv_hip_yuv_gather_dev, agmv_hip_yuv_histogram_dev and agmv_hip_yuv_similarity_dev (the last two against the
packed kernels on the converted clip).  Everything is exact.  A lane owns a patch of 16 x 2 pixels where w is a multiple of 16
and the clip is 16-byte aligned, and goes byte by byte otherwise: the geometries hold nothing, one and several patches, an odd
last row, widths that miss the wide path, and an I420 V plane on and off the 16-byte grid; the byte offsets 1 and 16 take a
wide geometry to the byte-wise path and back.  Needs an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import hostlib as H
import yuv_cases as Y

pytestmark = pytest.mark.gpu

GEOMETRIES = [(1, 1), (2, 2), (3, 3), (5, 2), (16, 2), (16, 3), (32, 4), (34, 6), (48, 5), (64, 48), (160, 128), (321, 243)]
OFFSETS = [0, 1, 16]
FORMATS = [layout | flags for layout in Y.LAYOUTS for flags in Y.FLAGS]
IDS = ["%s-%s" % (Y.NAMES[f & 0xFF], Y.FLAG_NAMES[f & 0x300]) for f in FORMATS]
SRC_W, SRC_H = 321, 243
GUARD = 64


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


def dev_u32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def host_u32(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def guarded(torch, n_bytes, off=0, raw=None):
    """n_bytes (holding `raw`, else 0xA5) `off` bytes behind a 16-byte boundary, between GUARD bytes of 0xA5 on either side;
    returns (allocation, view)"""
    buf = torch.full((GUARD + off + n_bytes + GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and GUARD % 16 == 0
    view = buf[GUARD + off:GUARD + off + n_bytes]
    if raw is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(raw, np.uint8).reshape(-1)))
    return buf, view


def guards_untouched(torch, buf, off, n_bytes):
    torch.cuda.synchronize()
    return bool((buf[:GUARD + off] == 0xA5).all() and (buf[GUARD + off + n_bytes:] == 0xA5).all())


def packed_out(torch, n, npx):
    """an int32 [n, npx] destination between guard bytes"""
    buf, view = guarded(torch, 4 * n * npx)
    return buf, view.view(torch.int32).view(n, npx)


# ------------------------------------------------------------------ to / from XRGB
@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_yuv_to_xrgb(torch, hip, fmt):
    rng = np.random.default_rng(fmt)
    for w, h in GEOMETRIES:
        for n in (1, 3):
            raw = rng.integers(0, 256, (n, Y.frame_bytes(fmt, w, h)), dtype=np.uint8)
            exp = Y.to_packed(fmt, raw, w, h).reshape(n, w * h)
            for off in OFFSETS:
                _, view = guarded(torch, raw.size, off, raw)
                buf, out = packed_out(torch, n, w * h)
                hip.yuv_to_xrgb_dev(fmt, view, w, h, n, out=out)
                got = host_u32(torch, out)
                assert (got >> 24 == 0).all(), (w, h, n, off, "top byte")
                assert (got == exp).all(), (w, h, n, off, np.argwhere(got != exp)[:4])
                assert guards_untouched(torch, buf, 0, 4 * n * w * h), (w, h, n, off, "guard bytes written")


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_yuv_from_xrgb(torch, hip, fmt):
    """random bits >= 24 in the packed input; the 64 bytes on either side of the frames keep their 0xA5"""
    rng = np.random.default_rng(100 + fmt)
    for w, h in GEOMETRIES:
        fb = Y.frame_bytes(fmt, w, h)
        for n in (1, 3):
            pix = rng.integers(0, 1 << 32, (n, h, w), dtype=np.uint32)
            exp = Y.from_packed(fmt, pix, w, h)
            src = dev_u32(torch, pix.reshape(n, w * h))
            for off in OFFSETS:
                buf, view = guarded(torch, n * fb, off)
                hip.yuv_from_xrgb_dev(fmt, src, w, h, out=view)
                torch.cuda.synchronize()
                got = buf.cpu().numpy()[GUARD + off:GUARD + off + n * fb].reshape(n, fb)
                assert (got == exp).all(), (w, h, n, off, np.argwhere(got != exp)[:4])
                assert guards_untouched(torch, buf, off, n * fb), (w, h, n, off, "guard bytes written")


@pytest.mark.parametrize("w,h,npx", [(64, 80, 4100), (321, 243, 9600)])
@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_first_pixels_of_larger_frames(torch, hip, fmt, w, h, npx):
    """a count that ends inside a row (and inside a patch): rows of npx words in the destination, nothing behind them"""
    rng = np.random.default_rng(200 + fmt + w)
    n = 3
    raw = rng.integers(0, 256, (n, Y.frame_bytes(fmt, w, h)), dtype=np.uint8)
    exp = Y.to_packed(fmt, raw, w, h).reshape(n, w * h)[:, :npx]
    _, view = guarded(torch, raw.size, 0, raw)
    buf, out = packed_out(torch, n, npx)
    hip.yuv_to_xrgb_dev(fmt, view, w, h, n, npx, out=out)
    assert (host_u32(torch, out) == exp).all()
    assert guards_untouched(torch, buf, 0, 4 * n * npx)


@functools.lru_cache(maxsize=None)
def every_triple():
    """64 frames of 512 x 512: the chroma planes enumerate all (U, V), the luma of frame f holds 4 f + (x & 1) + 2 (y & 1)"""
    f, y, x = np.meshgrid(np.arange(64), np.arange(512), np.arange(512), indexing="ij")
    luma = (4 * f + (x & 1) + 2 * (y & 1)).astype(np.uint8)
    v, u = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")                  # sample (cx, cy) = (U, V)
    u, v = u.astype(np.uint8), v.astype(np.uint8)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[None]
    return luma, u, v, up(u), up(v)


@pytest.mark.parametrize("flags", Y.FLAGS, ids=[Y.FLAG_NAMES[f] for f in Y.FLAGS])
def test_every_triple_is_read_as_the_definition_says(torch, hip, flags):
    luma, u, v, uu, vv = every_triple()
    exp = Y.yuv_to_rgb(flags, luma, uu, vv).reshape(64, -1)
    assert np.unique(luma.astype(np.uint32).reshape(64, 256, 2, 256, 2)[:, 3, :, 5, :]).size == 256       # one chroma sample meets all 256 Y
    for layout in Y.LAYOUTS:
        chroma = np.stack([u, v], axis=2).reshape(-1) if layout == Y.NV12 else np.concatenate([u.reshape(-1), v.reshape(-1)])
        raw = np.concatenate([luma.reshape(64, -1), np.broadcast_to(chroma, (64, chroma.size))], axis=1)
        assert (Y.to_packed(layout | flags, raw[:1], 512, 512).reshape(1, -1) == exp[:1]).all()
        buf, out = packed_out(torch, 64, 512 * 512)
        got = host_u32(torch, hip.yuv_to_xrgb_dev(layout | flags, torch.from_numpy(np.ascontiguousarray(raw)).cuda(), 512, 512, 64, out=out))
        assert (got == exp).all(), (layout, np.argwhere(got != exp)[:4])
        assert guards_untouched(torch, buf, 0, 4 * 64 * 512 * 512), (layout, "guard bytes written")


@pytest.mark.parametrize("flags", Y.FLAGS, ids=[Y.FLAG_NAMES[f] for f in Y.FLAGS])
def test_every_colour_is_written_as_the_definition_says(torch, hip, flags):
    """one 4096 x 4096 frame holding all 2^24 colours: R and G from the row, B and the low bits from the column, so the 2 x 2 means
    mix neighbouring colours in every channel"""
    yy, xx = np.meshgrid(np.arange(4096, dtype=np.uint32), np.arange(4096, dtype=np.uint32), indexing="ij")
    pix = ((yy >> 4) << 16 | ((yy & 15) << 4 | xx >> 8) << 8 | (xx & 255))[None]
    assert np.unique(pix).size == 1 << 24
    src = dev_u32(torch, pix.reshape(1, -1) | 0x5A000000)
    exp = Y.planes(Y.I420, Y.from_packed(Y.I420 | flags, pix, 4096, 4096), 4096, 4096)
    for layout in Y.LAYOUTS:
        fb = Y.frame_bytes(layout, 4096, 4096)
        buf, view = guarded(torch, fb)
        hip.yuv_from_xrgb_dev(layout | flags, src, 4096, 4096, out=view.view(1, fb))
        torch.cuda.synchronize()
        got = Y.planes(layout, view.cpu().numpy().reshape(1, fb), 4096, 4096)
        for name, g, e in zip("YUV", got, exp):
            assert (g == e).all(), (layout, name, np.argwhere(g != e)[:4])
        assert guards_untouched(torch, buf, 0, fb), (layout, "guard bytes written")


# ------------------------------------------------------------------ gather
def source_index(sw, sh, tw, th):
    L = H.lib()
    p = L.agmv_source_index(sw, sh, tw, th, tw, th)
    out = np.ctypeslib.as_array(p, (tw * th,)).copy()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(p)
    return out


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_yuv_gather_through_the_gba_and_nds_tables(torch, hip, fmt):
    rng = np.random.default_rng(300 + fmt)
    n = 2
    raw = rng.integers(0, 256, (n, Y.frame_bytes(fmt, SRC_W, SRC_H)), dtype=np.uint8)
    pix = Y.to_packed(fmt, raw, SRC_W, SRC_H).reshape(n, -1)
    for off in (0, 1):
        _, view = guarded(torch, raw.size, off, raw)
        for tw, th in ((120, 80), (128, 96)):
            idx = source_index(SRC_W, SRC_H, tw, th)
            assert (idx < SRC_W * SRC_H).sum() > tw * th // 2
            idx[[3, 77]] = 0xFFFFFFFF                                   # "no source pixel", and indices outside the frame
            idx[[5, 4097]] = [SRC_W * SRC_H, 0xFFFFFFFE]
            idx[[6, 7]] = [0, SRC_W * SRC_H - 1]
            live = idx < SRC_W * SRC_H
            exp = np.where(live[None, :], pix[:, np.where(live, idx, 0)], 0)
            buf, out = packed_out(torch, n, idx.size)
            hip.yuv_gather_dev(fmt, view, SRC_W, SRC_H, n, dev_u32(torch, idx), out=out)
            assert (host_u32(torch, out) == exp).all(), (off, tw, th)
            assert guards_untouched(torch, buf, 0, 4 * n * idx.size)


# ------------------------------------------------------------------ histogram
@functools.lru_cache(maxsize=None)
def runs_clip(n, w, h):
    """packed pixels [n, h, w] whose colours come in runs of 1 .. 40 pixels (flat areas and noise), so the run-length atomics see
    runs that cross lanes, slices, rows and frames; a YUV clip written from them in numpy has flat chroma where the colours are"""
    rng = np.random.default_rng(400 + 7 * n + w + 1000 * h)
    out = np.empty(n * w * h, np.uint32)
    i = 0
    while i < out.size:
        k = int(rng.integers(1, 41))
        out[i:i + k] = rng.integers(0, 1 << 24)
        i += k
    out = out.reshape(n, h, w)
    out.setflags(write=False)
    return out


# the frame sizes of the other kernels, the two counts that end inside a row, and one that ends inside a patch of a wide frame
HIST_SHAPES = [(w, h, w * h) for w, h in GEOMETRIES] + [(64, 80, 4100), (SRC_W, SRC_H, 9600), (64, 48, 64 * 47 + 16)]
HIST_BYTES = 4 << 19


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_yuv_histogram_equals_the_packed_histogram_of_the_converted_clip(torch, hip, fmt):
    """both add to what the table holds; the table lies between guard bytes"""
    start = np.random.default_rng(400 + fmt).integers(0, 1000, 1 << 19, dtype=np.uint32)
    start_d = dev_u32(torch, start).view(torch.uint8)
    for w, h, npx in HIST_SHAPES:
        for n in (1, 3):
            raw = Y.from_packed(fmt, runs_clip(n, w, h), w, h)
            packed = dev_u32(torch, Y.to_packed(fmt, raw, w, h).reshape(n, -1)[:, :npx])
            for quality in (1, 2, 3):
                exp = host_u32(torch, hip.histogram_dev(packed, quality, start_d.clone().view(torch.int32)))
                assert int(exp.sum(dtype=np.uint64) - start.sum(dtype=np.uint64)) == n * npx
                for off in OFFSETS:
                    _, view = guarded(torch, raw.size, off, raw)
                    buf, table = guarded(torch, HIST_BYTES)
                    table.copy_(start_d)
                    hip.yuv_histogram_dev(fmt, view, w, h, n, npx, quality, table.view(torch.int32))
                    got = host_u32(torch, table.view(torch.int32))
                    assert (got == exp).all(), (w, h, npx, n, quality, off, np.argwhere(got != exp)[:4])
                    assert guards_untouched(torch, buf, 0, HIST_BYTES), (w, h, npx, n, quality, off, "guard bytes written")


# ------------------------------------------------------------------ similarity
def pairs_clip(rng, fmt, n, w, h):
    """frames that keep about half of the bytes of the frame before (equal and different pixels), one pair of equal frames and one
    pair that differs by one luma step in a quarter of the pixels (nearly equal: most greys move, some do not)"""
    fb = Y.frame_bytes(fmt, w, h)
    fr = np.empty((n, fb), np.uint8)
    fr[0] = rng.integers(0, 256, fb, dtype=np.uint8)
    for f in range(1, n):
        fr[f] = np.where(rng.random(fb) < 0.5, fr[f - 1], rng.integers(0, 256, fb, dtype=np.uint8))
    if n > 3:
        fr[2] = fr[1]
        fr[3] = fr[2]
        step = rng.random(w * h) < 0.25
        fr[3, :w * h] = np.where(step, fr[2, :w * h] ^ 1, fr[2, :w * h])
    return fr


def grey(p):
    p = p.astype(np.uint32)
    return (((p >> 16) & 255) + ((p >> 8) & 255) + (p & 255)) // 3


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_yuv_similarity_equals_the_packed_kernel_on_the_converted_clip(torch, hip, fmt):
    rng = np.random.default_rng(500 + fmt)
    for w, h in GEOMETRIES:
        for n in (2, 6):
            raw = pairs_clip(rng, fmt, n, w, h)
            pix = Y.to_packed(fmt, raw, w, h).reshape(n, -1)
            g = grey(pix)
            by_hand = (g[:-1] == g[1:]).sum(1).astype(np.uint32)
            exp = host_u32(torch, hip.similarity_dev(dev_u32(torch, pix)))[:n - 1]
            assert (exp == by_hand).all()
            if n == 6 and w * h >= 64:
                assert by_hand[1] == w * h and 0 < by_hand[2] < w * h and 0 < by_hand[0] < w * h
            for off in OFFSETS:
                _, view = guarded(torch, raw.size, off, raw)
                buf, counts = guarded(torch, 4 * (n - 1))                         # 0xA5A5A5A5 each: overwritten, not added to
                got = host_u32(torch, hip.yuv_similarity_dev(fmt, view, w, h, n, counts.view(torch.int32)))
                assert (got == exp).all(), (w, h, n, off, got, exp)
                assert guards_untouched(torch, buf, 0, 4 * (n - 1)), (w, h, n, off, "guard bytes written")


def test_yuv_similarity_more_pairs_than_one_flush_segment(torch, hip):
    rng = np.random.default_rng(600)
    fmt, w, h, n = Y.I420 | Y.BT709, 16, 6, 1030
    raw = pairs_clip(rng, fmt, n, w, h)
    g = grey(Y.to_packed(fmt, raw, w, h).reshape(n, -1))
    buf, counts = guarded(torch, 4 * (n - 1))
    got = host_u32(torch, hip.yuv_similarity_dev(fmt, torch.from_numpy(raw).cuda(), w, h, n, counts.view(torch.int32)))
    assert (got == (g[:-1] == g[1:]).sum(1)).all()
    assert guards_untouched(torch, buf, 0, 4 * (n - 1)), "guard bytes written"


def test_unknown_format_or_flag_is_an_error(torch, hip):
    src = torch.zeros(256, dtype=torch.uint8, device="cuda")
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    for fmt in (0, 2, 6, 18, 16 | 0x400, 17 | 0x800, 2 | 0x100, 0x100):
        assert hip.L.agmv_hip_yuv_to_xrgb_dev(hip.ctx, fmt, src.data_ptr(), 4, 4, 1, 16, out.data_ptr(), None) != 0
        assert hip.L.agmv_hip_yuv_from_xrgb_dev(hip.ctx, fmt, out.data_ptr(), 4, 4, 1, src.data_ptr(), None) != 0
        assert hip.L.agmv_hip_yuv_gather_dev(hip.ctx, fmt, src.data_ptr(), 4, 4, 1, out.data_ptr(), 1, out.data_ptr(), None) != 0
        assert hip.L.agmv_hip_yuv_histogram_dev(hip.ctx, fmt, src.data_ptr(), 4, 4, 1, 16, 1, out.data_ptr(), None) != 0
        assert hip.L.agmv_hip_yuv_similarity_dev(hip.ctx, fmt, src.data_ptr(), 4, 4, 2, out.data_ptr(), None) != 0
        assert b"pixel format" in hip.L.agmv_hip_last_error()
        with pytest.raises(ValueError):
            hip.yuv_to_xrgb_dev(fmt, src, 4, 4, 1)
    for fmt in (16, 17 | 0x300):
        assert hip.L.agmv_hip_pixels_to_xrgb_dev(hip.ctx, fmt, src.data_ptr(), 16, 1, 16, out.data_ptr(), None) != 0      # the pixel-count functions
    with pytest.raises(ValueError):
        hip.yuv_to_xrgb_dev("nv12", src, 4, 4, 1, yuv="bt2020")
