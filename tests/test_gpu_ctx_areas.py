"""The work areas of a context (agmv_hip_impl.h: the table agmv_hip_ctx::ws, one area per stage, created by the stage's first call,
grown on demand, freed by agmv_hip_destroy): contexts that never use one, every stage on one context in either order, inputs that
shrink and grow again, and two contexts side by side.  Expected values come from the suite's references: the brute force and
the host stages (lzss_cases, lz77_cases, lz_decode_cases), the numpy k-means (palette_cases) and the CPU decoder (oracles)."""
import numpy as np
import pytest

import hostlib as H
import lz77_cases as Z77
import lz_decode_cases as LD
import lzss_cases as Z
import palette_cases as PC
from test_gpu_decode_ctx import Clip, check_bitmap_form

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SMALL, LARGE = (64, 300, 5000), (200000,)     # bytes per stream; the large one is above every first capacity of an area


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    return torch


class LzRef:
    """streams over a 4-symbol alphabet, their LZSS and LZ77 payloads, and what the decoder's LZ stage makes of those payloads"""

    def __init__(self, sizes, seed, brute_force):
        rng = np.random.default_rng(seed)
        self.streams = [rng.integers(0, 4, n, dtype=np.uint8) for n in sizes]
        host = [H.lzss(x) for x in self.streams], [H.lz77(x) for x in self.streams]
        self.lzss = [Z.orc(x) for x in self.streams] if brute_force else [p for p, _ in host[0]]
        self.lz77 = [Z77.orc77(x) for x in self.streams] if brute_force else [p for p, _ in host[1]]
        self.cap = max(sizes) + 64
        self.per0 = rng.integers(0, 256, self.cap, dtype=np.uint8)
        self.frames, self.decoded = {}, {}
        for version, comp in ((1, host[0]), (3, host[1])):
            self.frames[version] = [LD.Frame(p, len(x), c) for (p, c), x in zip(comp, self.streams)]
            self.decoded[version] = LD.host_batch(version, self.frames[version], self.cap, persist=self.per0)


@pytest.fixture(scope="module")
def refs():
    """every expected value, computed once and never written again"""
    small, large = LzRef(SMALL, 1, True), LzRef(LARGE, 2, False)
    rng = np.random.default_rng(3)
    hist = np.zeros(1 << 19, np.uint32)
    hist[rng.choice(1 << 19, 300, replace=False)] = rng.integers(1, 5000, 300)
    start = rng.integers(0, 1 << 24, 256).astype(np.uint32)
    pal = {"hist": hist, "start": start, "want": PC.refine(hist, PC.HIGH, start, 256, 1)}
    import synth as S
    p0, p1 = S.content_palettes([S.synth_frame(16, 16, t) for t in range(4)])
    return {"small": small, "large": large, "pal": pal, "palettes": (p0, p1), "clip": Clip(16, 16, 4, p0, p1)}


def new_context(refs):
    from libagmv_amd import AgmvHip
    h = AgmvHip(0)
    h.set_palette(refs["palettes"][0], refs["palettes"][1], True)
    return h


def run_lzss(torch, hip, ref):
    got = Z.gpu_batch(hip, ref.streams)
    for g, e in zip(got, ref.lzss):
        assert Z77.same(g, e)


def run_lz77(torch, hip, ref):
    got = Z77.gpu_batch77(hip, ref.streams)
    for g, e in zip(got, ref.lz77):
        assert Z77.same(g, e)


def _i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.int64).astype(np.uint32).view(np.int32).copy()).cuda()


def run_lz_decode(torch, hip, ref, versions=(1, 3)):
    for version in versions:
        frames, n, cap = ref.frames[version], len(ref.streams), ref.cap
        _, rows, bpos, used, per = ref.decoded[version]
        src, off, avail = LD.image(frames)
        bits = torch.full((n, cap), SENTINEL, dtype=torch.uint8, device="cuda")
        bits, d_bpos, d_used = hip.lz_decode_frames_dev(version, torch.from_numpy(src).cuda(), torch.from_numpy(off).cuda(), _i32(torch, avail),
                                                        _i32(torch, [f.usize for f in frames]), _i32(torch, [f.csize for f in frames]), n, cap, bits=bits)
        d_per = torch.from_numpy(ref.per0.copy()).cuda()
        hip.lz_decode_commit_dev(bits, d_bpos, n, d_per)
        assert hip.lz_decode_fallback_frames() == 0
        assert (d_bpos.cpu().numpy().view(np.uint32) == bpos).all() and (d_used.cpu().numpy().view(np.uint32) == used).all()
        assert (d_per.cpu().numpy() == per).all()
        got = bits.cpu().numpy()
        for f in range(n):
            e = min(int(bpos[f]) + 16, cap)
            assert (got[f, :e] == rows[f, :e]).all(), (version, f)
            assert (got[f, e:] == SENTINEL).all(), (version, f)


def run_palette(torch, hip, refs):
    p = refs["pal"]
    d_hist = torch.from_numpy(p["hist"].copy().view(np.int32)).cuda()
    d_pal = torch.from_numpy(p["start"].copy().view(np.int32)).cuda()
    rounds, sse = hip.palette_refine_dev(d_hist, PC.HIGH, d_pal, 256, 1)
    torch.cuda.synchronize()
    assert (d_pal.cpu().numpy().view(np.uint32) == p["want"]["pal"]).all()
    assert int(rounds.item()) == p["want"]["rounds"]
    assert tuple(int(v) for v in sse.cpu().numpy().view(np.uint64)) == tuple(p["want"]["sse"])


def stages(torch, refs):
    small = refs["small"]
    return [lambda h: run_lzss(torch, h, small), lambda h: run_lz77(torch, h, small), lambda h: run_lz_decode(torch, h, small),
            lambda h: run_palette(torch, h, refs), lambda h: check_bitmap_form(torch, h, refs["clip"])]


def test_contexts_that_use_no_area(torch):
    from libagmv_amd import AgmvHip
    for _ in range(8):
        AgmvHip(0).close()


@pytest.mark.parametrize("order", ("forward", "reverse"))
def test_every_stage_on_one_context(torch, refs, order):
    h = new_context(refs)
    try:
        todo = stages(torch, refs)
        for stage in (todo if order == "forward" else todo[::-1]):
            stage(h)
        h.check()
    finally:
        h.close()


@pytest.mark.parametrize("stage", ("lzss", "lz77", "lz_decode_lzss", "lz_decode_lz77"))
def test_small_large_small(torch, refs, stage):
    run = {"lzss": run_lzss, "lz77": run_lz77, "lz_decode_lzss": lambda t, h, r: run_lz_decode(t, h, r, (1,)),
           "lz_decode_lz77": lambda t, h, r: run_lz_decode(t, h, r, (3,))}[stage]
    h = new_context(refs)
    try:
        for ref in (refs["small"], refs["large"], refs["small"]):
            run(torch, h, ref)
    finally:
        h.close()


def test_areas_belong_to_their_context(torch, refs):
    small, large = refs["small"], refs["large"]
    a, b = new_context(refs), new_context(refs)
    try:
        run_lzss(torch, a, large)
        run_lzss(torch, b, small)
        run_lzss(torch, a, small)
        run_lzss(torch, b, large)
    finally:
        a.close()
    try:
        run_lzss(torch, b, large)
        run_lzss(torch, b, small)
    finally:
        b.close()
