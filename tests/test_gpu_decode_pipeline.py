"""k_decode as a loop over (GOP, tile) items (agmv_decode_hip.hip), last GOP first: a workgroup that takes several items one
after the other must give what one workgroup per item gives, whatever the order.  AGMV_DEC_GRID caps the grid: 1 = every
item in one workgroup, 2 and 3 = odd and even item counts per workgroup and, on the small shapes, idle workgroups; unset =
one workgroup per item.  Every case compares pixels, nentered and the prior-dependence flag with OracleDecoder started from
the same state, through the offsets form (parse_dev + decode_dev) and the bitmap form (decode_bitstreams_dev).

Shapes (a tile is 256 blocks): 64x64 one full tile; 68x64 a 16-block last tile; 320x240 19 tiles, the last of 192 blocks;
1028x4 and 4x1028: block nblk-1 is lane 0 of its tile (its FILL takes a neighbour from another tile: k_fixup).
Frames and starts: a single I-frame, a short first GOP, a short last GOP, whole GOPs.  Streams: encoder output of the
synthetic clip and of per-channel noise (blocks of 17-33 bytes: windows longer than the LDS stage, the global fallback), bpos
cut inside a FILL and inside a NORMAL block, stray bytes between blocks (on 320x240 enough for the `wide` bitmap path), an
empty stream between full ones.  A batch that starts inside a GOP gets random prev / prev_iframe.

The prior-dependence flag's reference: the oracle decodes the batch a second time from the complemented state (every pixel
of prev and prev_iframe different); the batch depends on its prior state exactly when any pixel comes out different."""
import numpy as np
import pytest

import oracles as O
import synth as S

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (68, 64), (320, 240), (1028, 4), (4, 1028)]
BATCHES = [(1, 0), (3, 1), (4, 0), (5, 3), (9, 2), (9, 0), (5, 0)]       # (frames, first_fc)
KINDS = ["synth", "noise", "cut", "stray", "empty"]
GRIDS = [None, 1, 2, 3]
CLIP = 12                                                              # frames encoded per clip: a batch is a slice of them
FLAGS = (0x4E, 0x2F, 0x5E)


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


def to_u32(t):
    return t.cpu().numpy().view(np.uint32)


class Case:
    """one batch: the slab and bpos handed to the GPU, the state it starts from, and what the oracle makes of it"""

    def __init__(self, name, w, h, mode512, pal, streams, first_fc, rng):
        self.name, self.w, self.h, self.mode512, self.first_fc, self.n = name, w, h, mode512, first_fc, len(streams)
        self.pal = pal
        self.prev = self.previ = None
        if first_fc & 3:                                               # inside a GOP: the caller hands the decoder's state in
            self.prev = rng.integers(0, 1 << 24, w * h, dtype=np.uint32)
            self.previ = rng.integers(0, 1 << 24, w * h, dtype=np.uint32)
        dec = O.OracleDecoder(w, h, mode512, *pal)
        dec.set_state(self.prev, self.previ, first_fc)
        pix, pads, nent = [], [], []
        for b in streams:
            p, padded, _, ne = dec.decode(b, want_tables=True)
            pix.append(p)
            pads.append(padded[len(b):len(b) + 16])
            nent.append(ne)
        alt = O.OracleDecoder(w, h, mode512, *pal)
        flip = lambda a: (np.zeros(w * h, np.uint32) if a is None else a) ^ np.uint32(0xFFFFFF)
        alt.set_state(flip(self.prev), flip(self.previ), first_fc)
        self.dep = any((alt.decode(b) != p).any() for b, p in zip(streams, pix))
        dec.close()
        alt.close()
        self.pix, self.nent = np.stack(pix), np.array(nent, np.int32)
        stride = (max(len(b) for b in streams) + 16 + 255) & ~255
        self.bits = np.zeros((self.n, stride), np.uint8)
        for i, b in enumerate(streams):
            self.bits[i, :len(b)] = b
            self.bits[i, len(b):len(b) + 16] = pads[i]
        self.bpos = np.array([len(b) for b in streams], np.int32)


def entry_offsets(w, h, mode512, pal, b):
    dec = O.OracleDecoder(w, h, mode512, *pal)
    _, _, offs, ne = dec.decode(b, want_tables=True)
    dec.close()
    return offs[:ne]


def cut_inside(w, h, mode512, pal, b, flag, keep):
    """b cut `keep` bytes behind the flag of the entered block of that type nearest the middle of the frame"""
    offs = entry_offsets(w, h, mode512, pal, b)
    ks = [k for k in range(len(offs)) if b[offs[k]] == flag]
    if not ks:
        return b
    k = min(ks, key=lambda k: abs(k - len(offs) // 2))
    return b[:offs[k] + keep]


def with_stray_bytes(w, h, mode512, pal, b, rng, want):
    """`want` bytes that are no flag (as many as the oracle's stream buffer has room for) in front of a block a third into the frame"""
    room = w * h * 3 + 64 - 16 - len(b)
    n = min(want, room)
    if n < 1:
        return b
    offs = entry_offsets(w, h, mode512, pal, b)
    at = int(offs[len(offs) // 3])
    junk = rng.integers(0, 256, n, dtype=np.uint8)
    junk[np.isin(junk, FLAGS)] = 0x11
    return np.concatenate([b[:at], junk, b[at:]])


_cases = {}


def cases_of(shape):
    """the cases of a shape, both palette modes: built once, shared by the grids"""
    if shape in _cases:
        return _cases[shape]
    w, h = shape
    rng = np.random.default_rng(w * 10007 + h)
    fw, fh = max(w, 8), max(h, 8)
    clean = np.stack([S.synth_frame(fw, fh, t)[:h, :w] for t in range(CLIP)]).astype(np.uint32)
    noisy = clean ^ (rng.integers(0, 8, clean.shape, dtype=np.uint32) | rng.integers(0, 8, clean.shape, dtype=np.uint32) << 8 |
                     rng.integers(0, 8, clean.shape, dtype=np.uint32) << 16)
    out = []
    for mode512 in (True, False):
        pal = S.content_palettes(clean[:4])
        enc = {}
        for kind, frames in (("synth", clean), ("noise", noisy)):
            e = O.OracleEncoder(w, h, mode512, *pal)
            enc[kind] = [e.encode(f).copy() for f in frames]
            e.close()
        for n, fc in BATCHES:
            for kind in KINDS:
                st = [b.copy() for b in enc["noise" if kind == "noise" else "synth"][fc:fc + n]]
                hurt = min(1, n - 1)
                if kind == "cut":
                    st[hurt] = cut_inside(w, h, mode512, pal, st[hurt], 0x4E, 1)
                    st[n - 1] = cut_inside(w, h, mode512, pal, enc["noise"][fc + n - 1].copy() if n > 1 else st[0], 0x2F, 6)
                elif kind == "stray":
                    st[hurt] = with_stray_bytes(w, h, mode512, pal, st[hurt], rng, 17000)
                elif kind == "empty":
                    st[hurt] = st[hurt][:0]
                out.append(Case("%s n=%d fc=%d m%d" % (kind, n, fc, 512 if mode512 else 256), w, h, mode512, pal, st, fc, rng))
    _cases[shape] = out
    return out


def check_case(torch, hip, c, tag=""):
    w, h, n = c.w, c.h, c.n
    bits, bpos = torch.from_numpy(c.bits).cuda(), torch.from_numpy(c.bpos).cuda()
    prev = dev_u32(torch, c.prev) if c.prev is not None else None
    previ = dev_u32(torch, c.previ) if c.previ is not None else None
    what = "%s%s %dx%d" % (tag, c.name, w, h)
    # offsets form
    offs, nent = hip.parse_dev(bits, bpos, n, w, h)
    out = hip.decode_dev(bits, bpos, offs, nent, n, w, h, c.first_fc, prev=prev, prev_iframe=previ)
    dep = hip.decode_depends_on_prior(w, h)
    assert (nent.cpu().numpy() == c.nent).all(), "offsets form, nentered: " + what
    bad = (to_u32(out).reshape(n, -1) != c.pix).any(axis=1).nonzero()[0]
    assert bad.size == 0, "offsets form, pixels of frames %s: %s" % (bad[:8], what)
    assert dep == c.dep, "offsets form, prior dependence: " + what
    # bitmap form
    nent2 = torch.full((n,), -1, dtype=torch.int32, device=bits.device)
    out2 = hip.decode_bitstreams_dev(bits, bpos, n, w, h, c.first_fc, nentered=nent2, prev=prev, prev_iframe=previ)
    dep2 = hip.decode_depends_on_prior(w, h)
    assert (nent2.cpu().numpy() == c.nent).all(), "bitmap form, nentered: " + what
    bad = (to_u32(out2).reshape(n, -1) != c.pix).any(axis=1).nonzero()[0]
    assert bad.size == 0, "bitmap form, pixels of frames %s: %s" % (bad[:8], what)
    assert dep2 == c.dep, "bitmap form, prior dependence: " + what


def set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("AGMV_DEC_GRID", raising=False)
    else:
        monkeypatch.setenv("AGMV_DEC_GRID", str(grid))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_items_in_a_loop_match_oracle(torch, hip, monkeypatch, shape, grid):
    set_grid(monkeypatch, grid)
    mode = None
    for c in cases_of(shape):
        if c.mode512 != mode:
            mode = c.mode512
            hip.set_palette(c.pal[0], c.pal[1], mode)
        check_case(torch, hip, c, "grid %s: " % grid)


def _clean_head(shape):
    w, h = shape
    return np.stack([S.synth_frame(max(w, 8), max(h, 8), t)[:h, :w] for t in range(4)]).astype(np.uint32)


@pytest.mark.parametrize("grid", GRIDS)
def test_slices_run_the_loop_over_gop_ranges(torch, hip, monkeypatch, grid):
    """agmv_hip_parse_decode_frames_dev with AGMV_DEC_SLICES=3: k_decode runs over GOP ranges [g0, g1), each range its own grid"""
    set_grid(monkeypatch, grid)
    monkeypatch.setenv("AGMV_DEC_SLICES", "3")
    shape = (320, 240)
    hip.set_palette(*S.content_palettes(_clean_head(shape)), True)
    for c in cases_of(shape):
        if not c.mode512 or c.n != 9:
            continue
        w, h, n = c.w, c.h, c.n
        bits, bpos = torch.from_numpy(c.bits).cuda(), torch.from_numpy(c.bpos).cuda()
        prev = dev_u32(torch, c.prev) if c.prev is not None else None
        previ = dev_u32(torch, c.previ) if c.previ is not None else None
        out, _, nent = hip.parse_decode_dev(bits, bpos, n, w, h, c.first_fc, prev=prev, prev_iframe=previ)
        dep = hip.decode_depends_on_prior(w, h)
        assert (nent.cpu().numpy() == c.nent).all(), c.name
        assert (to_u32(out).reshape(n, -1) == c.pix).all(), c.name
        assert dep == c.dep, c.name


@pytest.mark.parametrize("grid", [None, 2])
def test_two_contexts_on_two_streams(torch, monkeypatch, grid):
    """two contexts decode alternately, each on a stream of its own: a workgroup that loops must not assume it owns the device"""
    from libagmv_amd import AgmvHip
    set_grid(monkeypatch, grid)
    shape = (320, 240)
    pal = S.content_palettes(_clean_head(shape))
    cs = [c for c in cases_of(shape) if c.mode512 and c.n == 9 and c.first_fc == 0 and c.name.split()[0] in ("synth", "noise")]
    assert len(cs) == 2
    ctx = [AgmvHip(0), AgmvHip(0)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        outs, nents, keep = [[], []], [[], []], []
        for k in (0, 1):
            with torch.cuda.stream(streams[k]):
                ctx[k].set_palette(pal[0], pal[1], True)
        torch.cuda.synchronize()
        dev = [(torch.from_numpy(c.bits).cuda(), torch.from_numpy(c.bpos).cuda()) for c in cs]
        torch.cuda.synchronize()
        for rep in range(3):
            for k in (0, 1):
                with torch.cuda.stream(streams[k]):
                    ne = torch.full((cs[k].n,), -1, dtype=torch.int32, device="cuda")
                    outs[k].append(ctx[k].decode_bitstreams_dev(dev[k][0], dev[k][1], cs[k].n, cs[k].w, cs[k].h, nentered=ne))
                    nents[k].append(ne)
        torch.cuda.synchronize()
        for k in (0, 1):
            for o, ne in zip(outs[k], nents[k]):
                assert (ne.cpu().numpy() == cs[k].nent).all(), cs[k].name
                assert (to_u32(o).reshape(cs[k].n, -1) == cs[k].pix).all(), cs[k].name
            with torch.cuda.stream(streams[k]):
                assert ctx[k].decode_depends_on_prior(cs[k].w, cs[k].h) == cs[k].dep
    finally:
        for c in ctx:
            c.close()
