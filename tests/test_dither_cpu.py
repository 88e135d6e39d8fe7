"""The pattern dithering without a GPU: the numpy statement (tests/dither_cases.py) with a brute-force nearest entry has the
properties include/agmv.h lists, gives the hand-computed candidates and picks, and on the golden clip brings the 4x4 block sums
closer to the source than nearest-colour quantisation does; the header declares the entry point, the libraries export it and
AGMV_SetDither, and encode_frames checks `dither` before anything else."""
import os
import re

import numpy as np
import pytest

import dither_cases as D
import hostlib as H


def small_runs():
    """(name, pal512, mode512, frames, strength): frames of at most 16 x 8"""
    rng = np.random.default_rng(7)
    runs = []
    for mode512 in (False, True):
        pal = D.fox_palette(mode512)
        frames = rng.integers(0, 1 << 24, (2, 8, 16)).astype(np.uint32)
        frames[0, :2] = pal[rng.integers(0, 512 if mode512 else 256, (2, 16))]      # palette colours among them
        frames[1, 3] |= 0x5A000000
        for s in (1, 32, 64):
            runs.append(("fox%d-s%d" % (512 if mode512 else 256, s), pal, mode512, frames, s))
    for name, (pal, mode512, frames) in D.crafted().items():
        runs.append((name, pal, mode512, frames, 64))
    return runs


RUNS = small_runs()


@pytest.mark.parametrize("name,pal,mode512,frames,s", RUNS, ids=[r[0] for r in RUNS])
def test_properties_of_the_statement(name, pal, mode512, frames, s):
    assert frames.shape[1] <= 8 and frames.shape[2] <= 16
    near = D.brute_nearest(pal, mode512)
    out = D.dither(frames, pal, mode512, s, near)
    colours = pal[:512 if mode512 else 256] & 0xFFFFFF
    assert out.dtype == np.uint32 and out.shape == frames.shape
    assert np.isin(out, colours).all() and (out >> 24 == 0).all()                  # a subset of the palette, zero high byte
    fixed = np.isin(frames & 0xFFFFFF, colours)                                    # a palette-coloured pixel is a fixed point
    assert (out[fixed] == (frames & 0xFFFFFF)[fixed]).all()
    assert (D.dither(out, pal, mode512, s, near) == out).all()                     # ... so a second pass changes nothing
    # positional: the same pixel values shifted by a whole matrix period give the same picks, and every frame is its own origin
    if frames.shape[2] > 4:
        assert (D.dither(frames[:, :, 4:], pal, mode512, s, near) == out[:, :, 4:]).all()
    assert (D.dither(frames[-1:], pal, mode512, s, near) == out[-1:]).all()


def test_midway_pixel_alternates_and_the_matrix_picks_by_luma():
    pal, mode512, frames = D.crafted()["two_colours_midway"]
    near = D.brute_nearest(pal, mode512)
    # (100,100,100) between black in slot 0 and (200,200,200) in every other slot, s = 64: the tie goes to the lowest slot, black,
    # which leaves +100; 100 + 100 finds the grey in slot 1, which leaves 0; and so on: eight of each
    e = D.candidates(frames[0, 0, :1], pal, mode512, 64, near)[:, 0]
    assert e.tolist() == [0, 1] * 8
    out = D.dither(frames, pal, mode512, 64, near)
    want = np.where(D.B4[np.arange(8)[:, None] & 3, np.arange(8)[None, :] & 3] >= 8, D.GREY, 0)   # sorted by luma: 8 x black, 8 x grey
    assert (out[0] == want).all()
    assert int(D.channels(out).sum()) == int(D.channels(frames).sum())             # the mean is the pixel's, exactly
    # one step off the middle at s = 1, where a 64th of the error is fed back: (99,99,99) finds black (error 99), 99 + 1 is the tie:
    # black (198), 99 + 3 the grey (97), and from there 99 + 1 and 99 + 3 in turn: the error stays between 85 and 196
    e = D.candidates(np.array([D.rgb(99, 99, 99)], np.uint32), pal, mode512, 1, near)[:, 0]
    assert e.tolist() == [0, 0] + [1, 0] * 7


def test_one_pixel_by_hand():
    """palette 0 = black, (40,40,40), (80,80,80), (90,0,0) and black again in the other slots; the pixel (50,50,50) at s = 64:
    a: 50 -> (40) acc 10 | 60 -> (40) acc 20 | 70 -> (80) acc -10 | 40 -> (40) acc 0 | then the same four again"""
    p0 = np.zeros(256, np.uint32)
    p0[1], p0[2], p0[3] = D.rgb(40, 40, 40), D.rgb(80, 80, 80), D.rgb(90, 0, 0)
    pal = D.pal512_of(p0)
    near = D.brute_nearest(pal, False)
    px = np.array([D.rgb(50, 50, 50) | 0xFF000000], np.uint32)
    assert D.candidates(px, pal, False, 64, near)[:, 0].tolist() == [1, 1, 2, 1] * 4
    # keys ascending: 12 x entry 1 (luma 40000), 4 x entry 2 (luma 80000): t <= 11 picks (40,40,40), t >= 12 (80,80,80)
    frame = np.full((1, 4, 4), px[0], np.uint32)
    assert (D.dither(frame, pal, False, 64, near)[0] == np.where(D.B4 >= 12, p0[2], p0[1])).all()
    # at s = 32 half the error is fed back: 50, 55, 60 (equally far from 40 and 80: the lower slot), 65 -> (80), acc 0, again
    assert D.candidates(px, pal, False, 32, near)[:, 0].tolist() == [1, 1, 1, 2] * 4
    # the sort is by luma, not by entry number: (90,0,0) in slot 3 (luma 26910) comes before (40,40,40) in slot 1
    red = np.full((1, 4, 4), D.rgb(65, 20, 20), np.uint32)
    # (65,20,20) is equally far from both: slot 1, which leaves (25,-20,-20); (90,0,0) is slot 3 exactly, which leaves 0
    assert D.candidates(red[0, 0, :1], pal, False, 64, near)[:, 0].tolist() == [1, 3] * 8
    assert (D.dither(red, pal, False, 64, near)[0] == np.where(D.B4 < 8, p0[3], p0[1])).all()


@pytest.mark.parametrize("mode512", (False, True), ids=("256", "512"))
def test_block_sums_on_the_golden_clip(mode512):
    """frame 5 of tests/golden/foxlogo.npz, whole (no crop), its p0 (256 colours) and p0 | p1 (512), strength 32"""
    frames, _, _ = D.fox()
    src, pal = frames[D.FOX_FRAME:D.FOX_FRAME + 1], D.fox_palette(mode512)
    near = D.brute_nearest(pal, mode512)
    plain, out = D.quantised(src, pal, near), D.dither(src, pal, mode512, 32, near)
    e0, e1 = D.block_sum_error(plain, src), D.block_sum_error(out, src)
    sse = [int(((D.channels(x) - D.channels(src)) ** 2).sum()) for x in (plain, out)]
    print("%d colours: block sums %d -> %d (ratio %.3f; in box-mean units %.0f -> %.0f), uniform blocks %d -> %d of %d, per-pixel SSE %d -> %d"
          % (512 if mode512 else 256, e0, e1, e1 / e0, e0 / 256, e1 / 256, D.uniform_blocks(plain), D.uniform_blocks(out), 60 * 80, sse[0], sse[1]))
    assert e1 < e0


def test_header_declares_and_libraries_export():
    import ctypes as C

    from libagmv_amd import hip
    hdr = open(os.path.join(H.ROOT, "include", "agmv_hip.h")).read()
    assert re.search(r"int\s+agmv_hip_dither_frames_async\s*\(\s*agmv_hip_ctx\s*\*\s*ctx,\s*uint32_t\s+strength,\s*uint32_t\s*\*\s*d_pix,\s*"
                     r"uint32_t\s+w,\s*uint32_t\s+h,\s*uint32_t\s+n_frames,\s*void\s*\*\s*stream\s*\)\s*;", hdr)
    assert "void AGMV_SetDither(unsigned strength);" in open(os.path.join(H.ROOT, "include", "agmv.h")).read()
    host = H.lib()                                                                  # (builds both libraries)
    assert hasattr(host, "AGMV_SetDither")
    assert "agmv_hip_dither_frames_async" in hip.ABI_SYMBOLS
    assert hasattr(C.CDLL(os.path.join(H.ROOT, "libagmv_amd", "libagmv_hip.so")), "agmv_hip_dither_frames_async")


@pytest.mark.parametrize("bad", (0, 65, True, 1.5, "x"), ids=repr)
def test_encode_frames_refuses_dither(bad, tmp_path):
    """... on a CPU tensor and with an unknown filter, which later checks would refuse: the argument is looked at first"""
    import torch

    import libagmv_amd
    frames = torch.zeros((4, 16, 16), dtype=torch.int32)
    with pytest.raises(ValueError, match="dither"):
        libagmv_amd.encode_frames(str(tmp_path / "x.agmv"), frames, dither=bad, scale="no such filter")
    assert not (tmp_path / "x.agmv").exists()
