"""agmv_hip_deblock_frames_async, the deblocking of include/agmv.h, through AgmvHip.deblock_frames against the numpy statement
(tests/deblock_cases.py): every pixel, both counters, and guard words round the destination.  The shapes are the smallest that can
go wrong: 4 x 4 has no edge and four corner cells only; 8 x 4 and 4 x 8 have one edge and rim cells only; 8 x 8 has one interior
cell; 12 x 20 has all nine kinds of cell and makes the split of a lane's number into (cx, cy) matter; 260 x 8 and 8 x 260 have a
cell row longer than a wave and more cell rows than a wave has lanes; 1028 x 12 has a cell row longer than a workgroup; 3 frames
of 20 x 12 put frames on the grid's second axis, and 16384 + 5 frames of 8 x 8 go past what that axis holds for them.  Needs an
MI355X."""
import ctypes as C

import numpy as np
import pytest

import deblock_cases as K

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0x5A5A5A5A


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


def upload(torch, frames, shift=0):
    """-> (the whole buffer, the clip's words in it): GUARD words, `shift` more, the clip, GUARD words"""
    buf = torch.full((GUARD + shift + frames.size + GUARD,), FILL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    clip = buf[GUARD + shift:GUARD + shift + frames.size]
    clip.copy_(torch.from_numpy(np.ascontiguousarray(frames).view(np.int32).reshape(-1).copy()))
    return buf, clip


def guarded(buf, shift, shape):
    host = buf.cpu().numpy().view(np.uint32)
    assert (host[:GUARD + shift] == FILL).all() and (host[-GUARD:] == FILL).all(), "words around the clip were written"
    return host[GUARD + shift:-GUARD].reshape(shape).copy()


def run(torch, hip, frames, s, counted=True, shift=(0, 0), start=(0, 0), in_place=False):
    """frames uint32 [n, h, w] -> (the kernel's frames, (weak, strong) or None); asserts that the words round the destination kept
    their value and that the source is what it was.  shift: the words by which source and destination lie off a 16-byte boundary;
    start: what the counters hold before the call"""
    n, h, w = frames.shape
    sbuf, src = upload(torch, frames, shift[0])
    if in_place:
        dbuf, dst = sbuf, src
    else:
        dbuf = torch.full((GUARD + shift[1] + frames.size + GUARD,), FILL, dtype=torch.int32, device="cuda")
        dst = dbuf[GUARD + shift[1]:GUARD + shift[1] + frames.size]
    counts = torch.tensor(start, dtype=torch.int64, device="cuda") if counted else None
    assert hip.deblock_frames(src, w, h, s, dst, counts) is dst
    torch.cuda.synchronize()
    hip.check()
    got = guarded(dbuf, shift[0] if in_place else shift[1], frames.shape)
    if not in_place:
        assert (guarded(sbuf, shift[0], frames.shape) == frames).all(), "the source was written"
    return got, tuple(int(c) - s0 for c, s0 in zip(counts.tolist(), start)) if counted else None


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "%d of %d pixels differ" % (len(bad), got.size), bad[:4].tolist(),
                           [hex(int(got[tuple(i)])) for i in bad[:4]], [hex(int(want[tuple(i)])) for i in bad[:4]])


SHAPES = [(1, 4, 4), (2, 4, 8), (2, 8, 4), (2, 8, 8), (2, 20, 12), (1, 8, 260), (1, 260, 8), (1, 12, 1028), (3, 12, 20)]      # (n, h, w)


@pytest.mark.parametrize("n,h,w", SHAPES, ids=["%dx%dx%d" % (w, h, n) for n, h, w in SHAPES])
def test_every_shape_at_every_strength(torch, hip, n, h, w):
    """low-amplitude noise on a staircase of flat blocks 8 and 4 levels apart, and on a gentle one that the low strengths filter"""
    lines = 0
    for s in K.STRENGTHS:
        for clip in (K.staircase_clip(n, h, w, 7 * s + n), K.staircase_clip(n, h, w, 300 + s, levels=4, noise=9),
                     K.staircase_clip(n, h, w, 500 + s, levels=1, noise=1, gain=6)):
            want, weak, strong = K.deblock(clip, s)
            got, counts = run(torch, hip, clip, s, start=(n, 1000))
            same(got, want, (s, n, h, w))
            assert counts == (weak, strong), (s, counts, weak, strong)
            lines += weak + strong
    assert (lines == 0) == (h == 4 and w == 4)


@pytest.mark.parametrize("s", K.STRENGTHS)
def test_crafted_lines_in_either_stage(torch, hip, s):
    clip = K.crafted_clip(s)
    want, weak, strong = K.deblock(clip, s)
    assert weak and strong
    got, counts = run(torch, hip, clip, s)
    same(got, want, s)
    assert counts == (weak, strong)


def test_flat_blocks_become_ramps_and_a_uniform_clip_stays(torch, hip):
    for a, b in ((0, 64), (255, 191), (96, 104)):
        clip = K.flat_blocks(a, b, 12, 20)
        want, weak, strong = K.deblock(clip, 64)
        got, counts = run(torch, hip, clip, 64)
        same(got, want, (a, b))
        assert counts == (0, strong) == (0, K.lines_examined(1, 12, 20))
    uniform = np.full((3, 12, 20), 0xAB4D4D4D, np.uint32)
    got, counts = run(torch, hip, uniform, 64, start=(5, 6))
    same(got, uniform, "uniform")
    assert counts == (0, 0)


def test_a_source_and_a_destination_off_an_8_byte_boundary(torch, hip):
    """the word path: either pointer 4 bytes off; (2, 2) keeps both 8-byte aligned and takes the 16-byte path off a 16-byte boundary"""
    clip = K.staircase_clip(2, 12, 260, 41)
    want, weak, strong = K.deblock(clip, 16)
    for shift in ((1, 0), (0, 1), (1, 1), (3, 1), (2, 2), (1, 2)):
        got, counts = run(torch, hip, clip, 16, shift=shift)
        same(got, want, shift)
        assert counts == (weak, strong)
    crafted = K.crafted_clip(4)
    same(run(torch, hip, crafted, 4, shift=(1, 3))[0], K.deblock(crafted, 4)[0], "crafted, shifted")
    got, counts = run(torch, hip, clip, 16, shift=(1, 1), in_place=True)
    same(got, want, "in place, shifted")


@pytest.mark.parametrize("n,h,w", [(2, 8, 8), (2, 20, 12), (1, 12, 1028)])
def test_in_place_equals_out_of_place(torch, hip, n, h, w):
    clip = K.staircase_clip(n, h, w, 55)
    out, counts = run(torch, hip, clip, 16)
    same(out, K.deblock(clip, 16)[0], "out of place")
    got, counts2 = run(torch, hip, clip, 16, in_place=True)
    same(got, out, "in place")
    assert counts2 == counts


def test_without_counters_and_without_frames(torch, hip):
    clip = K.staircase_clip(3, 12, 20, 5)
    want, _, _ = K.deblock(clip, 16)
    got, _ = run(torch, hip, clip, 16, counted=False)
    same(got, want, "d_counts NULL")
    buf = torch.full((96,), FILL, dtype=torch.int32, device="cuda")
    counts = torch.tensor([9, 11], dtype=torch.int64, device="cuda")
    assert hip.L.agmv_hip_deblock_frames_async(hip.ctx, 8, buf.data_ptr(), 12, 8, 0, buf.data_ptr(), counts.data_ptr(), hip._stream()) == 0
    torch.cuda.synchronize()
    hip.check()
    assert (buf.cpu().numpy().view(np.uint32) == FILL).all() and counts.tolist() == [9, 11]


def test_more_frames_than_the_grid_has_rows(torch, hip):
    """8 x 8: one workgroup per frame, so the second axis holds 16384 frames and the last 5 are a second trip round the frame loop"""
    n = 16384 + 5
    clip = K.staircase_clip(n, 8, 8, 77)
    want, weak, strong = K.deblock(clip, 16)
    assert weak and strong
    got, counts = run(torch, hip, clip, 16)
    same(got, want, "16389 frames")
    assert counts == (weak, strong)


def test_the_wrapper_allocates_and_checks(torch, hip):
    clip = K.staircase_clip(2, 8, 12, 3)
    want, weak, strong = K.deblock(clip, 16)
    pix = torch.from_numpy(clip.view(np.int32).copy()).cuda()
    counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
    out = hip.deblock_frames(pix, 12, 8, 16, counts=counts)
    torch.cuda.synchronize()
    assert out.shape == pix.shape and out.data_ptr() != pix.data_ptr()
    same(out.cpu().numpy().view(np.uint32), want, "a new tensor")
    assert counts.tolist() == [weak, strong]
    with pytest.raises(ValueError, match="whole frames"):
        hip.deblock_frames(pix.reshape(-1)[:-4], 12, 8, 16)
    with pytest.raises(ValueError, match="out"):
        hip.deblock_frames(pix, 12, 8, 16, out=torch.zeros((8,), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="counts"):
        hip.deblock_frames(pix, 12, 8, 16, counts=torch.zeros((1,), dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError, match="strength"):
        hip.deblock_frames(pix, 12, 8, 65)


REFUSALS = [
    ("a NULL context", dict(ctx=None), b"NULL context"),
    ("a NULL source", dict(src=None), b"d_src"),
    ("a NULL destination", dict(dst=None), b"d_dst"),
    ("a source off a word boundary", dict(src=2), b"d_src"),
    ("a destination off a word boundary", dict(dst=2), b"d_dst"),
    ("width 0", dict(w=0), b"multiples of 4"),
    ("height 0", dict(h=0), b"multiples of 4"),
    ("width 10", dict(w=10), b"multiples of 4"),
    ("height 6", dict(h=6), b"multiples of 4"),
    ("2^31 pixels", dict(w=65536, h=32768), b"too large"),
    ("strength 0", dict(s=0), b"strength"),
    ("strength 65", dict(s=65), b"strength"),
]


@pytest.mark.parametrize("what,change,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(torch, hip, what, change, text):
    """a checkerboard of flat blocks, which a launch would turn into ramps and count"""
    clip = K.flat_blocks(96, 104, 8, 12)
    src = torch.from_numpy(np.concatenate([clip.reshape(-1), clip.reshape(-1)]).view(np.int32).copy()).cuda()
    dst = torch.full((2 * 8 * 12 + 4,), FILL, dtype=torch.int32, device="cuda")
    counts = torch.tensor([9, 11], dtype=torch.int64, device="cuda")
    a = dict(ctx=hip.ctx, s=8, src=0, dst=0, w=12, h=8)
    a.update(change)
    sp = None if a["src"] is None else C.c_void_p(src.data_ptr() + a["src"])
    dp = None if a["dst"] is None else C.c_void_p(dst.data_ptr() + a["dst"])
    rc = hip.L.agmv_hip_deblock_frames_async(a["ctx"], a["s"], sp, a["w"], a["h"], 2, dp, counts.data_ptr(), hip._stream())
    assert rc != 0 and text in hip.L.agmv_hip_last_error(), hip.L.agmv_hip_last_error()
    torch.cuda.synchronize()
    hip.check()
    assert (dst.cpu().numpy().view(np.uint32) == FILL).all() and counts.tolist() == [9, 11]
    assert (src.cpu().numpy().view(np.uint32).reshape(2, 8, 12) == clip).all()
