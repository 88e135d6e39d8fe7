"""agmv_hip_decode_bitstreams_dev cut into ranges of whole GOPs (agmv_decode_hip.hip): parser, k_decode and k_fixup run once
per range, each range continues from the pixels the range before it left, and the call answers for all of them -- pixels,
nentered, the prior-dependence flag, the count of frames the fast parser gave up on, the event times.
AGMV_DEC_RANGE_FRAMES forces the range length: 4 and 8 cut the builder's 9- and 5-frame batches (tests/test_gpu_decode_pipeline.py)
into up to three ranges: 9 frames from first_fc 0 run as 4 + 4 + 1 and 8 + 1, from first_fc 2 as 6 + 3 -- a short first range and
a short last one -- with either length (the first range keeps the batch's first I-frame, the last frame that can read the
caller's I-frame snapshot: the call's prior dependence is the first range's).

Shapes (a tile is 256 blocks): 64x64 one tile; 68x64 a ragged last tile; 320x240 19 tiles; 1028x4 the last block in another
tile than its left neighbour, so that k_fixup crosses tiles.  Every case is compared with OracleDecoder as check_case does."""
import numpy as np
import pytest

import synth as S
from test_gpu_decode_pipeline import Case, cases_of, check_case, dev_u32, set_grid, to_u32  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (68, 64), (320, 240), (1028, 4)]
BATCHES = [(9, 0), (9, 2), (5, 0), (5, 3)]                             # (frames, first_fc) of the builder's batches
RANGES = [4, 8]
REGION = 59 * 64                                                       # bytes a region of the fast parser owns


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


def ranged_cases(shape):
    return [c for c in cases_of(shape) if (c.n, c.first_fc) in BATCHES]


def the_case(shape, kind, n, fc):
    (c,) = [c for c in cases_of(shape) if c.mode512 and c.name == "%s n=%d fc=%d m512" % (kind, n, fc)]
    return c


def decode(torch, hip, c, bits=None, bpos=None):
    """the bitmap form on the current stream: pixels, nentered"""
    bits = torch.from_numpy(c.bits).cuda() if bits is None else bits
    bpos = torch.from_numpy(c.bpos).cuda() if bpos is None else bpos
    prev = dev_u32(torch, c.prev) if c.prev is not None else None
    previ = dev_u32(torch, c.previ) if c.previ is not None else None
    nent = torch.full((c.n,), -1, dtype=torch.int32, device="cuda")
    out = hip.decode_bitstreams_dev(bits, bpos, c.n, c.w, c.h, c.first_fc, nentered=nent, prev=prev, prev_iframe=previ)
    return out, nent


@pytest.mark.parametrize("grid", [None, 2])
@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_ranges_match_oracle(torch, hip, monkeypatch, shape, rng, grid):
    """both palette modes, the five stream kinds, the 9- and 5-frame batches from first_fc 0, 2 and 3"""
    set_grid(monkeypatch, grid)
    monkeypatch.setenv("AGMV_DEC_RANGE_FRAMES", str(rng))
    cs = ranged_cases(shape)
    assert len(cs) == 2 * len(BATCHES) * 5
    mode = None
    for c in cs:
        if c.mode512 != mode:
            mode = c.mode512
            hip.set_palette(c.pal[0], c.pal[1], mode)
        check_case(torch, hip, c, "range %d grid %s: " % (rng, grid))


def frame_the_fast_parser_gives_up(nblk, stride):
    """Runs of "4E 4E ..." (two-byte FILLs whose index byte is a flag value) on odd bytes across 28 region boundaries, each from
    before the run-in of the region behind the boundary to past the boundary, stray bytes that are no flag in between: every
    one of those regions is entered on the wrong byte parity and has to be walked again -- more than the parser repairs
    before it leaves the frame to the map / stitch / emit kernels (test_parser_proof_repair_and_fallback, frame (c), on a frame of
    4800 blocks).  Returns the row and its bpos; every block is entered."""
    b = np.full(stride, 0x11, np.uint8)
    runs, fills = 28, 170
    assert runs * fills <= nblk and runs * REGION + 64 + (nblk - runs * fills) < stride - 64
    for k in range(1, runs + 1):
        start = k * REGION - 301
        assert start % 2 == 1
        b[start:start + 2 * fills] = 0x4E
    end = runs * REGION - 301 + 2 * fills
    rest = nblk - runs * fills
    b[end:end + rest] = 0x5E                                           # COPY, one block per byte
    return b, end + rest


def test_fallback_frames_are_counted_over_ranges(torch, hip, monkeypatch):
    c = the_case((320, 240), "synth", 9, 0)
    nblk = c.w * c.h // 16
    stride = (29 * REGION + 255) & ~255
    bits = np.zeros((c.n, stride), np.uint8)
    bits[:, :c.bits.shape[1]] = c.bits
    bpos = c.bpos.copy()
    bits[1], bpos[1] = frame_the_fast_parser_gives_up(nblk, stride)  # in the first range
    dbits, dbpos = torch.from_numpy(bits).cuda(), torch.from_numpy(bpos).cuda()
    hip.set_palette(c.pal[0], c.pal[1], True)
    monkeypatch.delenv("AGMV_DEC_GRID", raising=False)
    monkeypatch.setenv("AGMV_DEC_RANGE_FRAMES", "0")
    whole, nent_whole = decode(torch, hip, c, dbits, dbpos)
    n_whole = hip.parse_fallback_frames()
    dep_whole = hip.decode_depends_on_prior(c.w, c.h)
    monkeypatch.setenv("AGMV_DEC_RANGE_FRAMES", "4")
    cut, nent_cut = decode(torch, hip, c, dbits, dbpos)
    n_cut = hip.parse_fallback_frames()
    dep_cut = hip.decode_depends_on_prior(c.w, c.h)
    print("fallback frames: uncut %d, three ranges %d" % (n_whole, n_cut))
    assert n_whole >= 1
    assert n_cut == n_whole
    assert int(nent_whole[1]) == nblk and torch.equal(nent_cut, nent_whole)
    assert torch.equal(cut, whole) and dep_cut == dep_whole


def test_event_times_add_up_over_ranges(torch, monkeypatch):
    """three ranges (4 + 4 + 1 frames): groups 1 and 2 are sums of three disjoint intervals inside the call, so each is more
    than what a call on the last range alone reports for the same frame"""
    from libagmv_amd import AgmvHip
    c = the_case((320, 240), "synth", 9, 0)
    w, h, n = c.w, c.h, c.n
    monkeypatch.delenv("AGMV_DEC_GRID", raising=False)
    t = AgmvHip(0)
    try:
        t.set_palette(c.pal[0], c.pal[1], True)
        t.enable_timing(True)
        bits, bpos = torch.from_numpy(c.bits).cuda(), torch.from_numpy(c.bpos).cuda()
        monkeypatch.setenv("AGMV_DEC_RANGE_FRAMES", "4")
        for _ in range(2):                                             # (the first call allocates)
            out, nent = decode(torch, t, c, bits, bpos)
        three = [t.last_kernel_ms(k) for k in (1, 2, 3)]
        assert (to_u32(out).reshape(n, -1) == c.pix).all() and (nent.cpu().numpy() == c.nent).all()
        # the last range by itself: frame 8 from the state frames 7 (prev) and 4 (the I-frame's snapshot) left
        for _ in range(2):
            last = t.decode_bitstreams_dev(bits[8:], bpos[8:], 1, w, h, 8, prev=out[7], prev_iframe=out[4])
        one = [t.last_kernel_ms(k) for k in (1, 2, 3)]
        assert (to_u32(last).reshape(-1) == c.pix[8]).all()
        print("parser, k_decode + k_fixup, call (ms): three ranges %s, the last range alone %s" % (three, one))
        assert three[0] > 0 and three[1] > 0
        assert three[0] + three[1] <= three[2]
        assert three[0] > one[0] and three[1] > one[1]
        monkeypatch.setenv("AGMV_DEC_RANGE_FRAMES", "0")               # one range again: the sums do not carry over
        decode(torch, t, c, bits, bpos)
        whole = [t.last_kernel_ms(k) for k in (1, 2, 3)]
        assert 0 < whole[0] and 0 < whole[1] and whole[0] + whole[1] <= whole[2]
    finally:
        t.close()


def test_ranges_on_a_busy_side_stream(torch, hip, monkeypatch):
    """a non-blocking torch stream with work queued ahead, the bitstreams arriving on that stream behind it: every range's
    launches must follow the caller's stream, or they read the zeros the buffer held before"""
    c = the_case((320, 240), "cut", 9, 2)
    hip.set_palette(c.pal[0], c.pal[1], True)
    monkeypatch.delenv("AGMV_DEC_GRID", raising=False)
    monkeypatch.setenv("AGMV_DEC_RANGE_FRAMES", "4")
    ref, nent_ref = decode(torch, hip, c)
    dep_ref = hip.decode_depends_on_prior(c.w, c.h)
    real_bits, real_bpos = torch.from_numpy(c.bits).cuda(), torch.from_numpy(c.bpos).cuda()
    bits, bpos = torch.zeros_like(real_bits), torch.zeros_like(real_bpos)
    ballast = torch.zeros(1 << 24, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    # torch hands out the 32 streams of its pool in turn, and the late-input harness (tests/stream_cases.py) is sensitive to
    # which of them it is given: take a whole turn, so that the tests after this one get the streams they got without it
    side = [torch.cuda.Stream() for _ in range(32)][0]
    with torch.cuda.stream(side):
        for _ in range(50):
            ballast.add_(1.0)
        bits.copy_(real_bits, non_blocking=True)
        bpos.copy_(real_bpos, non_blocking=True)
        out, nent = decode(torch, hip, c, bits, bpos)
        dep = hip.decode_depends_on_prior(c.w, c.h)
    side.synchronize()
    assert torch.equal(out, ref) and torch.equal(nent, nent_ref) and dep == dep_ref
    assert (to_u32(out).reshape(c.n, -1) == c.pix).all() and dep == c.dep
