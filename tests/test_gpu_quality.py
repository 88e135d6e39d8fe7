"""agmv_hip_measure_frames_async (k_measure) against the numpy statement of tests/quality_cases.py, word for word, for every layout
of the reference clip.  The shapes are the smallest at which the kernel can go wrong: blocks without a window, one window, two
overlapping ones, a width that is no multiple of 16, whole 16-pixel groups, one block past the kernel's tile in either direction,
clips no frame of which is 16-byte aligned, many frames, more items than a launch has workgroups (so that a workgroup walks
several, of different frames and tiles), and one frame whose sums do not fit 32 bits.  Every call is made twice
into result arrays that hold garbage, and both must hold the same bytes.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import pixfmt_cases as P
import quality_cases as Q
import scale_cases as SC
import yuv_cases as Y

pytestmark = pytest.mark.gpu

LAYOUTS = SC.BYTE_LAYOUTS + SC.YUV_PLAIN
TW, TH = Q.kernel_tile()
SHAPES = [(4, 4), (4, 8), (8, 4),                 # (w, h): blocks but no window
          (8, 8), (12, 8),                       # one window, two overlapping ones
          (20, 12),                              # rows that start inside a group of 16: the byte readers
          (32, 8), (48, 16),                     # whole groups of 16 on the 16-byte path
          (4 * TW + 4, 8), (8, 4 * TH + 4)]      # one block past the tile: windows across the tiles' seam


@pytest.fixture(scope="module")
def hip():
    import torch
    from libagmv_amd import AgmvHip
    assert torch.cuda.is_available()
    h = AgmvHip(0)
    yield h
    torch.cuda.synchronize()
    h.close()


def dev(a, offset=0):
    """an ndarray as a device tensor of the same bytes, `offset` elements into its allocation"""
    import torch
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32}[a.dtype]
    t = torch.from_numpy(a.view(signed).reshape(-1).copy())
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
    buf[offset:].copy_(t)
    return buf[offset:]


def run(hip, test, fmt, raw, w, h, offset=0):
    """the kernel's words, uint64 [n, 12]: two calls into arrays that hold different garbage"""
    import torch
    n = test.shape[0]
    d_test = dev(test, offset)
    d_ref = dev(raw.view(np.uint32) if fmt == P.XRGB32 else raw, offset)
    outs = []
    for fill in (0x5A5A5A5A5A5A5A5A, -0x0123456789ABCDEF):
        out = torch.full((n, 12), fill, dtype=torch.int64, device="cuda")
        hip.measure_frames(d_test, fmt, d_ref, w, h, n, out=out)
        outs.append(out.cpu().numpy().view(np.uint64))
    torch.cuda.synchronize()
    assert outs[0].tobytes() == outs[1].tobytes(), "two calls on the same clips gave different bytes"
    return outs[0]


def check(hip, test, fmt, refpix, offset=0, alpha=None):
    n, h, w = test.shape
    raw, ref = Q.reference_clip(fmt, refpix)
    if alpha is not None:
        raw = np.ascontiguousarray(P.from_packed(fmt, refpix.reshape(n, h * w), alpha=alpha))
    got, want = run(hip, test, fmt, raw, w, h, offset), Q.entries(Q.measure(test, ref))
    bad = np.argwhere(got != want)
    assert not len(bad), "frame %d word %d is %d, expected %d (%d of %d words differ)" % (
        bad[0][0], bad[0][1], int(got[tuple(bad[0])].view(np.int64)), int(want[tuple(bad[0])].view(np.int64)), len(bad), want.size)
    return want


@functools.lru_cache(maxsize=None)
def pair(w, h, n=2):
    """noise, and noise plus a small perturbation that grows from frame to frame"""
    test = Q.noise(w * 1000 + h, n, h, w)
    return test, Q.perturbed(test, w + h)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("fmt", LAYOUTS, ids=[SC.fmt_name(f) for f in LAYOUTS])
def test_every_layout_and_shape(hip, fmt, shape):
    test, ref = pair(*shape)
    want = check(hip, test, fmt, ref)
    assert (want[:, :3] > 0).all() and (want[0] != want[1]).any()


@pytest.mark.parametrize("fmt", LAYOUTS, ids=[SC.fmt_name(f) for f in LAYOUTS])
def test_complement_and_constant(hip, fmt):
    """negative windows, and a constant clip against noise"""
    test = Q.noise(11, 2, 16, 48)
    want = check(hip, test, fmt, Q.complement(test))
    if fmt in SC.BYTE_LAYOUTS:
        assert (want[:, 9:].view(np.int64) < 0).all()
    check(hip, np.full((2, 16, 48), 0x336699, np.uint32), fmt, test)
    check(hip, test, fmt, test)


@pytest.mark.parametrize("fmt", LAYOUTS, ids=[SC.fmt_name(f) for f in LAYOUTS])
def test_no_frame_is_16_byte_aligned(hip, fmt):
    """both clips one element into their allocations: every load goes through the byte readers"""
    for shape in ((48, 16), (20, 12)):
        test, ref = pair(*shape, n=3)
        check(hip, test, fmt, ref, offset=1)


@pytest.mark.parametrize("flags", Y.FLAGS, ids=[Y.FLAG_NAMES[f] for f in Y.FLAGS])
@pytest.mark.parametrize("layout", Y.LAYOUTS, ids=[Y.NAMES[f] for f in Y.LAYOUTS])
def test_yuv_matrices_and_an_unaligned_second_frame(hip, layout, flags):
    """12 x 12: 216 bytes per frame, so frame 1 starts 8 bytes off a 16-byte boundary; and 32 x 8 on the 16-byte path"""
    assert Y.frame_bytes(layout, 12, 12) == 216
    for shape in ((12, 12), (32, 8)):
        test, ref = pair(*shape, n=3)
        check(hip, test, layout | flags, ref)


def distinct_errors(seed, n, h, w):
    """noise, and the same with some channels raised by 1 + f % 97 in frame f: no two neighbouring frames have the same error"""
    rng = np.random.default_rng(seed)
    test = Q.noise(seed + 1, n, h, w)
    c = np.clip(Q.D.channels(test) + (rng.integers(0, 2, (n, h, w, 3)) * (1 + np.arange(n).reshape(n, 1, 1, 1) % 97)), 0, 255)
    return test, (c[..., 0] << 16 | c[..., 1] << 8 | c[..., 2]).astype(np.uint32)


GRID = Q.kernel_grid()
MANY = [1, 5, 3000, GRID + 904]                  # the last: more one-tile frames than a launch has workgroups


@pytest.mark.parametrize("n", MANY)
@pytest.mark.parametrize("shape", [(4, 4), (8, 8)], ids=["4x4", "8x8"])
def test_many_frames_each_with_its_own_error(hip, shape, n):
    """frames must not leak into each other; with more frames than the launch has workgroups (one item per frame at these sizes)
    the first 904 workgroups walk two items each with the grid's stride"""
    w, h = shape
    test, ref = distinct_errors(n + w, n, h, w)
    for fmt in (P.XRGB32, P.RGB24, Y.NV12):
        want = check(hip, test, fmt, ref)
        if n > 1 and fmt != Y.NV12:
            assert len(np.unique(want[:, 0])) > n // 2


@pytest.mark.parametrize("fmt", [P.XRGB32, P.RGB8P, Y.I420], ids=["xrgb32", "rgb8p", "i420"])
def test_a_workgroup_walks_tiles_of_different_frames(hip, fmt):
    """three tiles per frame (the third one block wide) and a third of the grid plus 40 frames: more items than workgroups, and since
    the grid is no multiple of 3 a workgroup's second item is another tile of another frame -- full after partial, with windows or
    without a right neighbour -- so what an item leaves in LDS and in the lane's maxima must not reach the next"""
    w, h, n = 4 * (2 * TW + 1), 8, GRID // 3 + 40
    assert GRID % 3 and 3 * n > GRID
    test, ref = distinct_errors(14, n, h, w)
    want = check(hip, test, fmt, ref)
    if fmt != Y.I420:
        assert len(np.unique(want[:, 6])) > 40       # the maxima differ from frame to frame


@pytest.mark.parametrize("fmt", LAYOUTS, ids=[SC.fmt_name(f) for f in LAYOUTS])
def test_sums_past_32_bits(hip, fmt):
    """one 320 x 240 frame of 0 against 255: an SSE of 4 993 920 000 per channel"""
    z = np.zeros((1, 240, 320), np.uint32)
    want = check(hip, z, fmt, Q.complement(z))
    if fmt in SC.BYTE_LAYOUTS:
        assert (want[0, :3] == 4993920000).all()


def test_bits_that_are_not_colour_are_ignored(hip):
    """garbage in bits >= 24 of XRGB32 on both sides, and in RGBA32's alpha"""
    rng = np.random.default_rng(13)
    test, ref = pair(48, 16)
    hi = lambda: (rng.integers(0, 256, test.shape).astype(np.uint32) << 24)
    clean = Q.entries(Q.measure(test, ref))
    got = run(hip, test | hi(), P.XRGB32, np.ascontiguousarray(ref | hi()).view(np.uint8).reshape(2, -1), 48, 16)
    assert (got == clean).all()
    assert (check(hip, test | hi(), P.RGBA32, ref, alpha=rng.integers(0, 256, (2, 48 * 16), dtype=np.uint8)) == clean).all()


def test_refusals_launch_nothing(hip):
    import torch
    test, ref = pair(8, 8)
    d_test, d_ref = dev(test), dev(np.zeros(4096, np.uint8))
    out = torch.full((2, 12), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    call = lambda fmt, w, h, n=2: hip.L.agmv_hip_measure_frames_async(hip.ctx, d_test.data_ptr(), fmt, d_ref.data_ptr(), w, h, n, out.data_ptr(), hip._stream())
    for fmt in (0, 6, 15, 18, 0x101, 16 | 0x400):
        assert call(fmt, 8, 8) != 0 and b"format" in hip.L.agmv_hip_last_error()
    for fmt, w, h in ((1, 6, 8), (2, 8, 10), (1, 0, 8), (16, 6, 6), (17, 8, 2)):
        assert call(fmt, w, h) != 0
    assert call(1, 8, 8, 0) == 0                                    # no frame: success, nothing is touched
    torch.cuda.synchronize()
    assert (out == 0x5A5A5A5A5A5A5A5A).all()
    with pytest.raises(RuntimeError):
        hip.measure_frames(d_test, "rgb24", d_ref, 6, 8, 2)
