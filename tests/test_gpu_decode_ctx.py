"""The decoder's part of a context (agmv_decode_hip.hip: struct dec_ws, one of the work areas of agmv_hip_ctx) is created by the
first parse or decode call and freed by agmv_hip_destroy: contexts that never decode, two contexts side by side, a work area
that shrinks and grows again, and the timing groups the decoder marks in the core's events.  Expected pixels: the CPU oracle."""
import math

import numpy as np
import pytest

import oracles as O
import synth as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    return torch


class Clip:
    """w x h x n synthetic frames as the oracle encodes them (one slab row per frame), and the pixels / entered blocks the oracle decodes"""

    def __init__(self, w, h, n, p0, p1):
        self.w, self.h, self.n = w, h, n
        enc, dec = O.OracleEncoder(w, h, True, p0, p1), O.OracleDecoder(w, h, True, p0, p1)
        streams = [enc.encode(S.synth_frame(w, h, t)) for t in range(n)]
        tables = [dec.decode(b, want_tables=True) for b in streams]
        self.pix = np.stack([t[0] for t in tables]).reshape(n, h, w)
        self.nent = np.array([t[3] for t in tables], np.int32)
        stride = (max(len(b) for b in streams) + 16 + 255) & ~255
        self.bits = np.zeros((n, stride), np.uint8)
        for i, b in enumerate(streams):
            self.bits[i, :len(b)] = b
        self.bpos = np.array([len(b) for b in streams], np.int32)


@pytest.fixture(scope="module")
def clips():
    """8x4 (2 blocks: one tile, one region) x 5 frames and 64x48 (192 blocks) x 9 frames: a GOP boundary and a ragged last GOP"""
    p0, p1 = S.content_palettes([S.synth_frame(64, 48, t) for t in range(4)])
    return (p0, p1), Clip(8, 4, 5, p0, p1), Clip(64, 48, 9, p0, p1)


def new_context(pal):
    from libagmv_amd import AgmvHip
    h = AgmvHip(0)
    h.set_palette(pal[0], pal[1], True)
    return h


def check_bitmap_form(torch, hip, clip):
    """agmv_hip_decode_bitstreams_dev with the caller's nentered[] and with the context's own: the oracle's pixels both times"""
    bits, bpos = torch.from_numpy(clip.bits).cuda(), torch.from_numpy(clip.bpos).cuda()
    nent = torch.full((clip.n,), -1, dtype=torch.int32, device=bits.device)
    out = hip.decode_bitstreams_dev(bits, bpos, clip.n, clip.w, clip.h, nentered=nent)
    own = hip.decode_bitstreams_dev(bits, bpos, clip.n, clip.w, clip.h, nentered=None)
    torch.cuda.synchronize()
    assert (nent.cpu().numpy() == clip.nent).all()
    assert (out.cpu().numpy().view(np.uint32) == clip.pix).all()
    assert (own.cpu().numpy().view(np.uint32) == clip.pix).all()


def check_two_call_form(torch, hip, clip):
    bits, bpos = torch.from_numpy(clip.bits).cuda(), torch.from_numpy(clip.bpos).cuda()
    offs, nent = hip.parse_dev(bits, bpos, clip.n, clip.w, clip.h)
    out = hip.decode_dev(bits, bpos, offs, nent, clip.n, clip.w, clip.h)
    torch.cuda.synchronize()
    assert (nent.cpu().numpy() == clip.nent).all()
    assert (out.cpu().numpy().view(np.uint32) == clip.pix).all()


def test_context_without_decode(torch, clips):
    pal = clips[0]
    new_context(pal).close()                                   # no work area: nothing of the decoder's to free
    h = new_context(pal)
    try:
        assert h.parse_fallback_frames() == 0
        with pytest.raises(RuntimeError, match="no decode has run on this context"):
            h.decode_depends_on_prior(8, 4)
    finally:
        h.close()


def test_two_contexts_do_not_share_work_areas(torch, clips, monkeypatch):
    pal, small, large = clips
    a, b = new_context(pal), new_context(pal)
    try:
        check_bitmap_form(torch, a, large)
        check_two_call_form(torch, b, small)
        monkeypatch.setenv("AGMV_HIP_PARSE", "robust")         # the robust kernels' workspace too
        check_bitmap_form(torch, a, small)                     # shrink ...
        monkeypatch.delenv("AGMV_HIP_PARSE")
        check_bitmap_form(torch, a, large)                     # ... and grow again
        check_two_call_form(torch, b, small)                   # b's results are still its own
    finally:
        a.close()
        b.close()


def test_timing_groups_after_decode(torch, clips):
    pal, _, large = clips
    h = new_context(pal)
    try:
        h.enable_timing(True)
        bits, bpos = torch.from_numpy(large.bits).cuda(), torch.from_numpy(large.bpos).cuda()
        h.decode_bitstreams_dev(bits, bpos, large.n, large.w, large.h)
        for which in (1, 2, 3):                                # the parser, k_decode + k_fixup, the whole call
            ms = h.last_kernel_ms(which)
            assert math.isfinite(ms) and ms >= 0, (which, ms)
        h.enable_timing(False)
        for which in (1, 2, 3):
            assert h.last_kernel_ms(which) < 0, which
    finally:
        h.close()
