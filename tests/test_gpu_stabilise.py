"""agmv_hip_stabilise_frames_async, the temporal stabilisation of include/agmv.h, through AgmvHip.stabilise_frames against the numpy
statement (tests/stabilise_cases.py), word for word, and the device counter against the statement's `replaced`.  The shapes are the
smallest that can go wrong: one block; 12 x 8, where the split of a lane's block number into (bx, by) matters; 260 x 4, whose 65
blocks cross a wave; 1028 x 8, whose 514 blocks cross a workgroup.  Batches of 1 .. 9 frames from frame counts 0, 1, 2, 3 and 5 have
a leading part without an anchor and a trailing GOP with one or two P-frames; 4 * 65536 + 4 frames go past the grid's second axis;
4100 frames of 512 x 512 put a frame offset past 2^32 bytes.  The crafted blocks sit on both sides of either threshold.  Needs an
MI355X."""
import ctypes as C

import numpy as np
import pytest

import stabilise_cases as S

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


def run(torch, hip, frames, s, first_fc=0, counted=True, shift=0, start=0):
    """frames uint32 [n, h, w] -> (the kernel's frames, the counter); asserts that the words before and after the clip kept their
    value.  shift: words by which the clip lies off a 16-byte boundary; start: what the counter holds before the call"""
    n, h, w = frames.shape
    buf = torch.full((GUARD + shift + frames.size + GUARD,), FILL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    clip = buf[GUARD + shift:GUARD + shift + frames.size]
    clip.copy_(torch.from_numpy(np.ascontiguousarray(frames).view(np.int32).reshape(-1).copy()))
    count = torch.full((1,), start, dtype=torch.int64, device="cuda") if counted else None
    assert hip.stabilise_frames(clip, w, h, s, first_fc, count) is clip
    torch.cuda.synchronize()
    hip.check()
    host = buf.cpu().numpy().view(np.uint32)
    assert (host[:GUARD + shift] == FILL).all() and (host[-GUARD:] == FILL).all(), "words around the clip were written"
    return host[GUARD + shift:-GUARD].reshape(n, h, w).copy(), int(count.item()) - start if counted else None


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "%d of %d pixels differ" % (len(bad), got.size), bad[:4].tolist(),
                           [hex(int(got[tuple(i)])) for i in bad[:4]], [hex(int(want[tuple(i)])) for i in bad[:4]])


SHAPES = [(4, 4), (8, 12), (4, 260), (8, 1028)]                 # (h, w)


@pytest.mark.parametrize("h,w", SHAPES, ids=["%dx%d" % (w, h) for h, w in SHAPES])
def test_batches_of_1_to_9_frames_from_every_phase(torch, hip, h, w):
    kinds = set()
    for first_fc in (0, 1, 2, 3, 5):
        for n in range(1, 10):
            clip = S.random_clip(n, h, w, 8, 1000 * first_fc + n)
            want, examined, replaced = S.stabilise(clip, 8, first_fc)
            got, count = run(torch, hip, clip, 8, first_fc, start=n)
            same(got, want, (first_fc, n))
            assert count == replaced, (first_fc, n, count, replaced, examined)
            kinds |= {"none" if examined == 0 else "some" if 0 < replaced < examined else "all" if replaced else "zero"}
    assert "none" in kinds and ("some" in kinds or h * w == 16)      # (one block per frame is still or not)


@pytest.mark.parametrize("s", S.STRENGTHS)
def test_crafted_blocks(torch, hip, s):
    clip, still, _ = S.crafted_clip(s)
    want, _, replaced = S.stabilise(clip, s, 0)
    got, count = run(torch, hip, clip, s, 0)
    same(got, want, s)
    assert count == replaced == int(still.sum())


def test_crafted_blocks_in_every_p_frame_of_a_gop(torch, hip):
    """the crafted P-frame of each strength as frames 1, 2 and 3 of one GOP, strength 16: each P-frame has a decision of its own"""
    a = S.crafted_clip(16)
    clip = np.stack([a[0][0], a[0][1], a[0][0] ^ np.uint32(0x01000000), np.roll(a[0][1], 4, axis=1)])
    want, examined, replaced = S.stabilise(clip, 16, 0)
    got, count = run(torch, hip, clip, 16, 0)
    same(got, want, "three P-frames")
    assert count == replaced and 0 < replaced < examined


def test_more_gops_than_the_grid_has_rows(torch, hip):
    n = 4 * 65536 + 4
    clip = S.random_clip(n, 4, 4, 8, 77)
    want, examined, replaced = S.stabilise(clip, 8, 0)
    assert examined == 3 * 65537 and 0 < replaced < examined
    got, count = run(torch, hip, clip, 8, 0)
    same(got, want, "65537 GOPs")
    assert count == replaced


def test_a_frame_offset_past_4_gib(torch, hip):
    """4100 frames of 512 x 512 (1 MiB each), all zero but the last GOP, of which alone the result is downloaded"""
    n, h, w = 4100, 512, 512
    last = S.random_clip(4, h, w, 16, 4100)
    want, examined, replaced = S.stabilise(last, 16, 0)
    assert 0 < replaced < examined
    buf = torch.zeros((n, h, w), dtype=torch.int32, device="cuda")
    buf[n - 4:].copy_(torch.from_numpy(last.view(np.int32).copy()))
    count = torch.zeros((1,), dtype=torch.int64, device="cuda")
    hip.stabilise_frames(buf.reshape(-1), w, h, 16, 0, count)
    torch.cuda.synchronize()
    hip.check()
    same(buf[n - 4:].cpu().numpy().view(np.uint32), want, "the last GOP")
    assert int(buf[n - 8:n - 4].abs().max().item()) == 0
    assert int(count.item()) == replaced + 3 * (n // 4 - 1) * (h // 4) * (w // 4)       # (the zero GOPs are still, and are replaced by zeros)


def test_a_pointer_off_a_16_byte_boundary(torch, hip):
    clip = S.random_clip(7, 8, 260, 8, 31)
    want, _, replaced = S.stabilise(clip, 8, 2)
    for shift in (1, 2, 3):
        got, count = run(torch, hip, clip, 8, 2, shift=shift)
        same(got, want, shift)
        assert count == replaced
    crafted, _, _ = S.crafted_clip(16)
    same(run(torch, hip, crafted, 16, 0, shift=1)[0], S.stabilise(crafted, 16, 0)[0], "crafted, shifted")


def test_without_a_counter_and_without_frames(torch, hip):
    clip = S.random_clip(6, 8, 12, 8, 5)
    want, _, _ = S.stabilise(clip, 8, 0)
    got, _ = run(torch, hip, clip, 8, 0, counted=False)
    same(got, want, "d_replaced NULL")
    buf = torch.full((96,), FILL, dtype=torch.int32, device="cuda")
    count = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    assert hip.L.agmv_hip_stabilise_frames_async(hip.ctx, 8, buf.data_ptr(), 12, 8, 0, 0, count.data_ptr(), hip._stream()) == 0
    assert hip.L.agmv_hip_stabilise_frames_async(hip.ctx, 8, buf.data_ptr(), 12, 8, 1, 0, count.data_ptr(), hip._stream()) == 0      # an I-frame alone
    torch.cuda.synchronize()
    hip.check()
    assert (buf.cpu().numpy().view(np.uint32) == FILL).all() and int(count.item()) == 9


REFUSALS = [
    ("a NULL context", dict(ctx=None), b"NULL context"),
    ("a NULL clip", dict(pix=None), b"d_pix"),
    ("a clip off a word boundary", dict(pix=2), b"d_pix"),
    ("width 0", dict(w=0), b"multiples of 4"),
    ("height 0", dict(h=0), b"multiples of 4"),
    ("width 10", dict(w=10), b"multiples of 4"),
    ("height 6", dict(h=6), b"multiples of 4"),
    ("strength 0", dict(s=0), b"strength"),
    ("strength 65", dict(s=65), b"strength"),
]


@pytest.mark.parametrize("what,change,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(torch, hip, what, change, text):
    """equal frames, which a launch would replace (bits 24 .. 31 would go to zero) and count"""
    buf = torch.full((4 * 8 * 12,), FILL, dtype=torch.int32, device="cuda")
    count = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    a = dict(ctx=hip.ctx, s=8, pix=0, w=12, h=8)
    a.update(change)
    pix = None if a["pix"] is None else C.c_void_p(buf.data_ptr() + a["pix"])
    rc = hip.L.agmv_hip_stabilise_frames_async(a["ctx"], a["s"], pix, a["w"], a["h"], 4, 0, count.data_ptr(), hip._stream())
    assert rc != 0 and text in hip.L.agmv_hip_last_error(), hip.L.agmv_hip_last_error()
    torch.cuda.synchronize()
    hip.check()
    assert (buf.cpu().numpy().view(np.uint32) == FILL).all() and int(count.item()) == 9
