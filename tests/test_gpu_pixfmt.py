"""The kernels that read and write a clip in the caller's pixel layout (AGMV_PIXFMT: RGB24, BGR24, RGBA32, planar RGB8),
through AgmvHip, against numpy statements of the layouts (tests/pixfmt_cases.py): agmv_hip_pixels_to_xrgb_dev /
_from_xrgb_dev, agmv_hip_gather_fmt_dev, agmv_hip_histogram_fmt_dev (against the packed kernel it generalises) and
agmv_hip_similarity_fmt_dev.  Everything is exact.  The sizes are the smallest that reach every path: a lane owns 16 pixels
(1, 15, 16, 17: nothing, a partial, one, one and a partial group), a wave 1024, a block 4096; a clip at a byte offset or with
frames of an odd size takes the byte-wise path of the same kernels.  Needs an MI355X."""
import numpy as np
import pytest

import pixfmt_cases as P

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 16, 17, 63, 64, 65, 1000, 160 * 128]
OFFSETS = [0, 1, 2, 3, 4, 12]
SRC_W, SRC_H = 321, 243
SRC_PX = SRC_W * SRC_H


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


def dev_clip(torch, raw, off=0, guard=0):
    """the bytes of `raw` `off` bytes behind a 512-byte boundary of an allocation filled with 0xA5; returns (allocation, view)"""
    raw = np.ascontiguousarray(raw, np.uint8).reshape(-1)
    buf = torch.full((guard + off + raw.size + guard + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[guard + off:guard + off + raw.size]
    view.copy_(torch.from_numpy(raw))
    assert view.data_ptr() % 16 == (guard + off) % 16
    return buf, view


def random_packed(rng, n, npx):
    return rng.integers(0, 1 << 32, (n, npx), dtype=np.uint32)


# ------------------------------------------------------------------ to / from XRGB
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("fmt", P.NEW)
def test_pixels_to_xrgb(torch, hip, fmt, n, off):
    rng = np.random.default_rng(1000 * fmt + 10 * n + off)
    for npx in SIZES:
        raw = rng.integers(0, 256, (n, P.frame_bytes(fmt, npx)), dtype=np.uint8)          # (random alpha too)
        exp, _ = P.to_packed(fmt, raw, npx)
        _, view = dev_clip(torch, raw, off)
        got = host_u32(torch, hip.pixels_to_xrgb_dev(fmt, view, npx, n))
        assert got.shape == (n, npx)
        assert (got >> 24 == 0).all(), (npx, "top byte")
        assert (got == exp).all(), (npx, np.argwhere(got != exp)[:4])


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("fmt", P.NEW)
def test_pixels_from_xrgb(torch, hip, fmt, n, off):
    """random bits >= 24 in the packed input; alpha 0xFF on output; the 64 bytes on either side of the frames keep their 0xA5"""
    rng = np.random.default_rng(2000 * fmt + 10 * n + off)
    for npx in SIZES:
        pix = random_packed(rng, n, npx)
        fb = P.frame_bytes(fmt, npx)
        buf, view = dev_clip(torch, np.full(n * fb, 0xA5, np.uint8), off, guard=64)
        hip.pixels_from_xrgb_dev(fmt, dev_u32(torch, pix), out=view)
        torch.cuda.synchronize()
        whole = buf.cpu().numpy()
        got = whole[64 + off:64 + off + n * fb].reshape(n, fb)
        assert (got == P.from_packed(fmt, pix)).all(), npx
        if fmt == P.RGBA32:
            assert (got.reshape(n, npx, 4)[..., 3] == 0xFF).all(), npx
        assert (whole[:64 + off] == 0xA5).all() and (whole[64 + off + n * fb:] == 0xA5).all(), (npx, "guard bytes written")
        back, _ = P.to_packed(fmt, got, npx)
        assert (back == pix & 0xFFFFFF).all()


@pytest.mark.parametrize("fmt", P.NEW)
def test_first_pixels_of_larger_frames(torch, hip, fmt):
    """9 600 of 321 x 243 pixels per frame: the frame stride is 3 * 78003 bytes (odd), the plane stride 78003, not 9 600"""
    rng = np.random.default_rng(30 + fmt)
    n, npx = 3, 9600
    raw = rng.integers(0, 256, (n, P.frame_bytes(fmt, SRC_PX)), dtype=np.uint8)
    exp, _ = P.to_packed(fmt, raw, SRC_PX)
    _, view = dev_clip(torch, raw)
    got = host_u32(torch, hip.pixels_to_xrgb_dev(fmt, view, SRC_PX, n, npx))
    assert (got == exp[:, :npx]).all()
    # and with frames that ARE aligned (4112 = 257 * 16), a count that ends inside a group of 16
    raw = rng.integers(0, 256, (n, P.frame_bytes(fmt, 4112)), dtype=np.uint8)
    exp, _ = P.to_packed(fmt, raw, 4112)
    _, view = dev_clip(torch, raw)
    got = host_u32(torch, hip.pixels_to_xrgb_dev(fmt, view, 4112, n, 4100))
    assert (got == exp[:, :4100]).all()


@pytest.mark.parametrize("npx", [1, 48])
@pytest.mark.parametrize("fmt", [P.XRGB32] + list(P.NEW))
def test_one_pixel_written_out_by_hand(torch, hip, fmt, npx):
    """0x00112233 in all five layouts, as bytes typed in tests/pixfmt_cases.py: a channel swap cannot hide behind a symmetric helper"""
    one = np.frombuffer(P.ONE_PIXEL[fmt], np.uint8)
    raw = np.tile(one, npx) if fmt != P.RGB8P else np.repeat(one, npx)
    src = dev_u32(torch, raw.view(np.uint32)) if fmt == P.XRGB32 else dev_clip(torch, raw)[1]
    got = host_u32(torch, hip.pixels_to_xrgb_dev(fmt, src, npx, 1))
    assert (got == 0x00112233).all()
    packed = np.full((1, npx), 0x00112233 if fmt == P.XRGB32 else 0x5A112233, np.uint32)
    out = hip.pixels_from_xrgb_dev(fmt, dev_u32(torch, packed))
    torch.cuda.synchronize()
    assert out.cpu().numpy().reshape(-1).view(np.uint8).tobytes() == raw.tobytes()


# ------------------------------------------------------------------ gather
@pytest.mark.parametrize("fmt", [P.XRGB32] + list(P.NEW))
def test_gather_fmt(torch, hip, fmt):
    rng = np.random.default_rng(40 + fmt)
    n = 2
    pix = random_packed(rng, n, SRC_PX) & 0xFFFFFF
    raw = P.from_packed(fmt, pix, alpha=rng.integers(0, 256, (n, SRC_PX), dtype=np.uint8))
    src = dev_u32(torch, pix) if fmt == P.XRGB32 else dev_clip(torch, raw)[1]
    for n_out in (1, 9600, 12288):
        idx = rng.integers(0, SRC_PX, n_out, dtype=np.uint32)
        if n_out > 1:
            idx[[3, 77, n_out - 1]] = 0xFFFFFFFF
            idx[[5, 4097]] = [SRC_PX, 0xFFFFFFFE]                   # outside the source frame: reads as "no source pixel"
            idx[[6, 7]] = [0, SRC_PX - 1]
        live = idx < SRC_PX
        exp = np.where(live[None, :], pix[:, np.where(live, idx, 0)], 0)
        got = host_u32(torch, hip.gather_fmt_dev(fmt, src, SRC_PX, n, dev_u32(torch, idx)))
        assert got.shape == (n, n_out) and (got == exp).all(), n_out
    idx = np.array([0xFFFFFFFF], np.uint32)
    assert (host_u32(torch, hip.gather_fmt_dev(fmt, src, SRC_PX, n, dev_u32(torch, idx))) == 0).all()


# ------------------------------------------------------------------ histogram
def runs_clip(rng, n, npx):
    """colours in runs of 1 .. 40 pixels (flat areas and noise), so the run-length atomics see runs that cross lanes and slices"""
    out = np.empty(n * npx, np.uint32)
    i = 0
    while i < out.size:
        k = int(rng.integers(1, 41))
        out[i:i + k] = rng.integers(0, 1 << 24)
        i += k
    return out.reshape(n, npx)


@pytest.mark.parametrize("fpx,npx,off", [(160 * 128, 160 * 128, 0), (4112, 4100, 0), (SRC_PX, 9600, 0), (160 * 128, 160 * 128, 1), (17, 17, 0)])
@pytest.mark.parametrize("fmt", P.NEW)
def test_histogram_fmt_equals_the_packed_histogram(torch, hip, fmt, fpx, npx, off):
    rng = np.random.default_rng(50 + fmt + fpx)
    n = 3
    pix = runs_clip(rng, n, fpx)
    _, view = dev_clip(torch, P.from_packed(fmt, pix), off)
    packed = dev_u32(torch, pix[:, :npx])
    start = rng.integers(0, 1000, 1 << 19, dtype=np.uint32)                      # both add to what is there
    for quality in (1, 2, 3):
        exp = host_u32(torch, hip.histogram_dev(packed, quality, dev_u32(torch, start)))
        got = host_u32(torch, hip.histogram_fmt_dev(fmt, view, fpx, n, npx, quality, dev_u32(torch, start)))
        assert int(exp.sum(dtype=np.uint64) - start.sum(dtype=np.uint64)) == n * npx
        assert (got == exp).all(), quality


def test_histogram_fmt_of_a_packed_clip_is_the_packed_histogram(torch, hip):
    rng = np.random.default_rng(59)
    pix = runs_clip(rng, 3, 4112)
    exp = host_u32(torch, hip.histogram_dev(dev_u32(torch, pix[:, :4100]), 3))
    got = host_u32(torch, hip.histogram_fmt_dev(P.XRGB32, dev_u32(torch, pix), 4112, 3, 4100, 3))
    assert (got == exp).all()


# ------------------------------------------------------------------ similarity
def grey(p):
    p = p.astype(np.uint32)
    return (((p >> 16) & 255) + ((p >> 8) & 255) + (p & 255)) // 3


def expected_counts(pix):
    g = grey(pix)
    return (g[:-1] == g[1:]).sum(1).astype(np.uint32)


def random_clip(rng, n, npx):
    """each frame keeps about half of the frame before it, so the counts are neither 0 nor npx"""
    fr = np.empty((n, npx), np.uint32)
    fr[0] = rng.integers(0, 1 << 24, npx, dtype=np.uint32)
    for f in range(1, n):
        keep = rng.random(npx) < 0.5
        fr[f] = np.where(keep, fr[f - 1], rng.integers(0, 1 << 24, npx, dtype=np.uint32))
    return fr


def gpu_counts(torch, hip, fmt, pix, off=0, rng=None):
    n, npx = pix.shape
    alpha = rng.integers(0, 256, (n, npx), dtype=np.uint8) if rng is not None else None
    _, view = dev_clip(torch, P.from_packed(fmt, pix, alpha=alpha), off)
    counts = torch.full((max(n - 1, 1),), 123456, dtype=torch.int32, device="cuda")      # overwritten, not added to
    return host_u32(torch, hip.similarity_fmt_dev(fmt, view, n, npx, counts))[:n - 1]


@pytest.mark.parametrize("n", [2, 3, 9])
@pytest.mark.parametrize("fmt", P.NEW)
def test_similarity_fmt_counts(torch, hip, fmt, n):
    rng = np.random.default_rng(60 + 10 * fmt + n)
    for npx in (1, 7, 16, 17, 1023, 1025, 160 * 128):
        pix = random_clip(rng, n, npx)
        exp = expected_counts(pix)
        assert (gpu_counts(torch, hip, fmt, pix, rng=rng) == exp).all(), npx


@pytest.mark.parametrize("off", [0, 1, 4, 12])
@pytest.mark.parametrize("fmt", P.NEW)
def test_similarity_fmt_grey_edges(torch, hip, fmt, off):
    """equal greys of different colours count, channel sums 2 | 3 and 764 | 765 straddle a grey step; also from a clip at a byte
    offset (the byte-wise loads)"""
    npx = 4096 + 32
    a = np.zeros(npx, np.uint32)
    b = np.zeros(npx, np.uint32)
    a[0::4], b[0::4] = 0x030000, 0x000201            # sums 3 and 3: grey 1 and 1, different colours
    a[1::4], b[1::4] = 0x000002, 0x010101            # sums 2 and 3: grey 0 and 1
    a[2::4], b[2::4] = 0xFFFEFE, 0xFEFFFF            # sums 763 and 764: grey 254 and 254
    a[3::4], b[3::4] = 0xFFFFFE, 0xFFFFFF            # sums 764 and 765: grey 254 and 255
    c = (b & 0xFF) << 16 | (b & 0xFF00) | b >> 16    # b with R and B exchanged: other colours, the same greys
    pix = np.stack([a, b, c, a])
    exp = expected_counts(pix)
    assert list(exp) == [npx // 2, npx, npx // 2] and (b != c).any()
    assert (gpu_counts(torch, hip, fmt, pix, off) == exp).all()


@pytest.mark.parametrize("fmt", P.NEW)
def test_similarity_fmt_more_pairs_than_one_flush_segment(torch, hip, fmt):
    rng = np.random.default_rng(70 + fmt)
    pix = random_clip(rng, 1030, 64)
    assert (gpu_counts(torch, hip, fmt, pix) == expected_counts(pix)).all()


def test_similarity_fmt_of_a_packed_clip_is_the_packed_kernel(torch, hip):
    rng = np.random.default_rng(79)
    pix = random_clip(rng, 5, 1025)
    got = host_u32(torch, hip.similarity_fmt_dev(P.XRGB32, dev_u32(torch, pix), 5, 1025))
    assert (got == expected_counts(pix)).all()


def test_unknown_format_is_an_error(torch, hip):
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(16, dtype=torch.int32, device="cuda")
    for fmt in (0, 6):
        assert hip.L.agmv_hip_pixels_to_xrgb_dev(hip.ctx, fmt, src.data_ptr(), 16, 1, 16, out.data_ptr(), None) != 0
        assert hip.L.agmv_hip_pixels_from_xrgb_dev(hip.ctx, fmt, out.data_ptr(), 1, 16, src.data_ptr(), None) != 0
        assert hip.L.agmv_hip_gather_fmt_dev(hip.ctx, fmt, src.data_ptr(), 16, 1, out.data_ptr(), 1, out.data_ptr(), None) != 0
        assert hip.L.agmv_hip_similarity_fmt_dev(hip.ctx, fmt, src.data_ptr(), 2, 8, out.data_ptr(), None) != 0
        assert b"pixel format" in hip.L.agmv_hip_last_error()
        with pytest.raises(ValueError):
            hip.pixels_to_xrgb_dev(fmt, src, 16, 1)
