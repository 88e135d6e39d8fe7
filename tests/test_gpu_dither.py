"""agmv_hip_dither_frames_async, the pattern dithering of include/agmv.h, through AgmvHip.dither_frames against the numpy statement
(tests/dither_cases.py), bit for bit.  `nearest` of the statement is the context's own exact table, downloaded once per palette
with quantise_dev over all 2^24 colours (tests/test_gpu_hotpath.py proves that table).  The shapes are the smallest that can go
wrong: one block, one pixel, frames whose width is no multiple of 4 and whose size is no multiple of 16 (the row phase and the
per-frame origin), more frames than the grid has rows, a frame larger than one sweep of the grid, one golden frame; both palette
sizes, strengths 1, 32 and 64, pixels with bits >= 24 set, crafted palettes.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import dither_cases as D

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


use = D.use_palette


def run(torch, hip, frames, s):
    """frames uint32 [n, h, w] -> the kernel's frames; asserts that the words before and after the clip kept their value"""
    n, h, w = frames.shape
    buf = torch.full((GUARD + frames.size + GUARD,), FILL, dtype=torch.int32, device="cuda")
    clip = buf[GUARD:GUARD + frames.size]
    clip.copy_(torch.from_numpy(np.ascontiguousarray(frames).view(np.int32).reshape(-1).copy()))
    assert hip.dither_frames(clip, w, h, s) is clip
    torch.cuda.synchronize()
    hip.check()
    host = buf.cpu().numpy().view(np.uint32)
    assert (host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all(), "words around the clip were written"
    return host[GUARD:-GUARD].reshape(n, h, w).copy()


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "%d of %d pixels differ" % (len(bad), got.size), bad[:4].tolist(),
                           [hex(int(got[tuple(i)])) for i in bad[:4]], [hex(int(want[tuple(i)])) for i in bad[:4]])


# (n, h, w): one block; one pixel; 7x5x3 and 33x3x2; 2100 frames of one pixel (more frames than the grid has rows: the frame loop);
# 1030 x 515 = 530450 pixels (more than one sweep of 8 workgroups x 256 CUs x 256 lanes: the pixel loop); the golden frame
SHAPES = [(1, 4, 4), (1, 1, 1), (3, 5, 7), (2, 3, 33), (2100, 1, 1), (1, 515, 1030), (1, 240, 320)]


@functools.lru_cache(maxsize=None)
def clip_of(shape, mode512):
    """the golden frame, or: random colours, palette colours and pixels of the golden frame in equal parts, bits >= 24 set in a third"""
    frames, _, _ = D.fox()
    if shape == (1, 240, 320):
        clip = frames[D.FOX_FRAME:D.FOX_FRAME + 1].copy()
    else:
        rng = np.random.default_rng(sum(shape))
        pal = D.fox_palette(mode512)
        kind = rng.integers(0, 3, shape)
        clip = np.where(kind == 0, rng.integers(0, 1 << 24, shape), np.where(kind == 1, pal[rng.integers(0, 512 if mode512 else 256, shape)],
                                                                          frames[D.FOX_FRAME].reshape(-1)[rng.integers(0, 76800, shape)])).astype(np.uint32)
    clip[rng_mask(shape)] |= np.uint32(0xC3000000)
    return clip


def rng_mask(shape):
    return np.random.default_rng(99).integers(0, 3, shape) == 0


@pytest.mark.parametrize("s", (1, 32, 64))
@pytest.mark.parametrize("mode512", (False, True), ids=("256", "512"))
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % (w, h, n) for n, h, w in SHAPES])
def test_kernel_equals_the_statement(torch, hip, shape, mode512, s):
    pal = D.fox_palette(mode512)
    near = use(torch, hip, pal, mode512)
    clip = clip_of(shape, mode512)
    got = run(torch, hip, clip, s)
    same(got, D.dither(clip, pal, mode512, s, near), (shape, mode512, s))
    assert (got >> 24 == 0).all() and np.isin(got, pal[:512 if mode512 else 256]).all()


@pytest.mark.parametrize("s", (1, 32, 64))
@pytest.mark.parametrize("name", sorted(D.crafted()))
def test_crafted_palettes(torch, hip, name, s):
    pal, mode512, frames = D.crafted()[name]
    near = use(torch, hip, pal, mode512)
    got = run(torch, hip, frames, s)
    same(got, D.dither(frames, pal, mode512, s, near), (name, s))
    if name == "all_black":
        assert (got == 0).all()
    if name == "two_colours_midway" and s == 64:                       # eight times black, eight times the grey: the matrix picks by luma
        assert (got[0] == np.where(D.B4[np.arange(8)[:, None] & 3, np.arange(8)[None, :] & 3] >= 8, D.GREY, 0)).all()
    if name == "clamps_at_both_ends":                                  # the darkest grey for black, the lightest for white, whatever the strength
        assert (got[0, :, :4] == D.rgb(120, 120, 120)).all() and (got[0, :, 4:] == D.rgb(135, 135, 135)).all()


@pytest.mark.parametrize("mode512", (False, True), ids=("256", "512"))
def test_golden_frame_block_sums_fixed_points_and_second_pass(torch, hip, mode512):
    pal = D.fox_palette(mode512)
    near = use(torch, hip, pal, mode512)
    src = D.fox()[0][D.FOX_FRAME:D.FOX_FRAME + 1]
    got = run(torch, hip, src, 32)
    e0, e1 = D.block_sum_error(D.quantised(src, pal, near), src), D.block_sum_error(got, src)
    print("%d colours: block sums %d -> %d (ratio %.3f)" % (512 if mode512 else 256, e0, e1, e1 / e0))
    assert e1 < e0
    fixed = np.isin(src, pal[:512 if mode512 else 256])
    assert fixed.any() and (got[fixed] == src[fixed]).all()           # a pixel whose colour is in the palette comes back as it is
    same(run(torch, hip, got, 32), got, "second pass")                 # ... so a second call changes nothing
    same(run(torch, hip, got, 64), got, "second pass, another strength")


def test_every_frame_is_its_own_origin(torch, hip):
    """the same 7 x 5 picture three times: three equal results, which a position taken from the index in the batch would not give"""
    pal = D.fox_palette(True)
    use(torch, hip, pal, True)
    one = clip_of((3, 5, 7), True)[:1]
    got = run(torch, hip, np.repeat(one, 3, axis=0), 64)
    assert (got[1] == got[0]).all() and (got[2] == got[0]).all() and (got[0] != (one[0] & 0xFFFFFF)).any()


BAD = {"null_context": dict(ctx=None), "null_pixels": dict(pix=None), "no_palette": dict(fresh=True), "strength_0": dict(s=0), "strength_65": dict(s=65),
       "width_0": dict(w=0), "height_0": dict(h=0), "frame_of_2^31_pixels": dict(w=65536, h=32768)}


@pytest.mark.parametrize("name", sorted(BAD))
def test_refused_arguments_touch_nothing(torch, hip, name):
    from libagmv_amd import AgmvHip
    use(torch, hip, D.fox_palette(True), True)
    a = dict(ctx=hip.ctx, s=32, w=8, h=4, n=2, fresh=False)
    a.update(BAD[name])
    other = AgmvHip(0) if a["fresh"] else None                         # a context that never saw a palette
    buf = torch.full((GUARD + 64 + GUARD,), FILL, dtype=torch.int32, device="cuda")
    pix = None if "pix" in BAD[name] else buf.data_ptr() + 4 * GUARD
    rc = hip.L.agmv_hip_dither_frames_async(other.ctx if other else a["ctx"], a["s"], pix, a["w"], a["h"], a["n"], None)
    torch.cuda.synchronize()
    msg = hip.L.agmv_hip_last_error().decode()
    if other:
        other.close()
    assert rc != 0 and msg.startswith("agmv_hip:") and len(msg) > 20, (rc, msg)
    if name not in ("null_context", "no_palette"):
        assert "dither" in msg, msg
    assert (buf.cpu().numpy().view(np.uint32) == FILL).all(), "a refused call wrote to the device"


def test_no_frames_is_success(torch, hip):
    use(torch, hip, D.fox_palette(True), True)
    buf = torch.full((GUARD,), FILL, dtype=torch.int32, device="cuda")
    assert hip.L.agmv_hip_dither_frames_async(hip.ctx, 32, buf.data_ptr(), 8, 4, 0, None) == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint32) == FILL).all()
    with pytest.raises(ValueError, match="dither_frames"):             # the wrapper's own checks
        hip.dither_frames(buf, 5, 5, 32)
    with pytest.raises(ValueError, match="dither_frames"):
        hip.dither_frames(buf.cpu(), 8, 4, 32)
