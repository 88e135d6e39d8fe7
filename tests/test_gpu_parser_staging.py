"""How the fast parser stages a region (fp_walk_region, agmv_decode_hip.hip): the span's bytes come through a buffer descriptor
on the frame's row, so bytes in front of the row and at or past its stride must read as 0 whatever lies there in memory; and
the fixed costs of a call cut into ranges: range 0's prior-dependence word, one timing mark per boundary.

Shapes: 64x64 of the synthetic clip (256 blocks: one k_decode tile, streams of one region) and 128x128 with three bits of
noise per channel (1024 blocks, four tiles, streams of about 20 KB: six regions of 59 pieces, so run-in, the piece behind
and region-to-region proofs all occur).  Batches of 5 and 9 frames from first_fc 0 and 2, both palette modes.

The expectation is OracleDecoder fed, frame by frame, with the bytes of the row up to bpos while its persistent stream buffer
holds the WHOLE row (the reference reads on past bpos into whatever its buffer holds; the GPU reads the row, and zeros from
the stride on).  A batch that starts inside a GOP gets random prev / prev_iframe."""
import numpy as np
import pytest

import oracles as O
import synth as S

pytestmark = pytest.mark.gpu

FC, FRB = 64, 59 * 64                                                  # bytes of a piece, bytes a region owns
SHAPES = [(64, 64), (128, 128)]
BATCHES = [(5, 0), (5, 2), (9, 0), (9, 2)]                             # (frames, first_fc)
CLIP = 15
FLAGS = np.array([0x2F, 0x4E, 0x5E], np.uint8)
CUTS = [0, 1, 2, 3, 63, 64, 65, FRB - 1, FRB, FRB + 1, 2 * FRB - 1, 2 * FRB + 1]


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
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def to_u32(t):
    return t.cpu().numpy().view(np.uint32)


_clips = {}


def clip_of(shape, mode512):
    """(palettes, the encoder's streams of CLIP frames, a seeded generator): built once"""
    key = (shape, mode512)
    if key not in _clips:
        w, h = shape
        rng = np.random.default_rng(w * 131 + h + (7 if mode512 else 0))
        frames = np.stack([S.synth_frame(w, h, t) for t in range(CLIP)]).astype(np.uint32)
        pal = S.content_palettes(frames[:4])
        if shape == (128, 128):
            for sh in (0, 8, 16):
                frames ^= rng.integers(0, 8, frames.shape, dtype=np.uint32) << sh
        e = O.OracleEncoder(w, h, mode512, *pal)
        streams = [e.encode(f).copy() for f in frames]
        e.close()
        _clips[key] = (pal, streams)
    return _clips[key]


def rows_of(streams, stride):
    """the zero-filled slab of these streams (cut at the stride) and their bpos"""
    bits = np.zeros((len(streams), stride), np.uint8)
    for i, b in enumerate(streams):
        n = min(len(b), stride)
        bits[i, :n] = b[:n]
    return bits, np.array([min(len(b), stride) for b in streams], np.int32)


def prior_of(shape, fc, seed=5):
    if not fc & 3:
        return None, None
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    return rng.integers(0, 1 << 24, n, dtype=np.uint32), rng.integers(0, 1 << 24, n, dtype=np.uint32)


def oracle_rows(shape, mode512, pal, bits, bpos, fc, prev, previ):
    """pixels and nentered of the rows: the oracle's stream buffer holds the row (zeros behind it), the stream ends at bpos"""
    w, h = shape
    dec = O.OracleDecoder(w, h, mode512, *pal)
    dec.set_state(prev, previ, fc)
    cap = int(dec.s.bitstream_cap)
    pix, nent = [], []
    for row, n in zip(bits, bpos):
        img, ifr, count, _ = dec.state()
        buf = np.zeros(cap, np.uint8)
        m = min(cap, len(row))
        buf[:m] = row[:m]
        dec.set_state(img, ifr, count, bitstream=buf)
        p, _, _, ne = dec.decode(row[:n], want_tables=True)
        pix.append(p)
        nent.append(ne)
    dec.close()
    return np.stack(pix), np.array(nent, np.int32)


def gpu_rows(torch, hip, shape, dbits, bpos, fc, prev, previ):
    """the bitmap form on rows already on the device: pixels, nentered, frames the fast parser gave up on, prior dependence"""
    w, h = shape
    n = len(bpos)
    nent = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    out = hip.decode_bitstreams_dev(dbits, torch.from_numpy(np.asarray(bpos, np.int32)).cuda(), n, w, h, fc, nentered=nent,
                                    prev=dev_u32(torch, prev), prev_iframe=dev_u32(torch, previ))
    return to_u32(out).reshape(n, -1), nent.cpu().numpy(), hip.parse_fallback_frames(), hip.decode_depends_on_prior(w, h)


def check_rows(torch, hip, shape, mode512, pal, bits, bpos, fc, what):
    prev, previ = prior_of(shape, fc)
    pix, nent = oracle_rows(shape, mode512, pal, bits, bpos, fc, prev, previ)
    g_pix, g_nent, _, _ = gpu_rows(torch, hip, shape, torch.from_numpy(bits).cuda(), bpos, fc, prev, previ)
    assert (g_nent == nent).all(), "nentered %s: %s against %s" % (what, g_nent, nent)
    bad = (g_pix != pix).any(axis=1).nonzero()[0]
    assert bad.size == 0, "pixels of frames %s: %s" % (bad[:8], what)


def flag_bytes(rng, n):
    return FLAGS[rng.integers(0, 3, n)]


@pytest.mark.parametrize("mode512", [True, False], ids=["m512", "m256"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_slab_inside_flag_valued_memory(torch, hip, monkeypatch, shape, mode512):
    """the slab is a window into a tensor of 0x2F / 0x4E / 0x5E: flag bytes directly in front of row 0, behind the last row and
    from every row's bpos to the next row's start.  Pixels, nentered and the fallback count are those of the zero-filled slab
    (and of the oracle): a negative offset or one past the stride that read memory would find block starts there"""
    monkeypatch.delenv("AGMV_DEC_GRID", raising=False)
    monkeypatch.delenv("AGMV_DEC_RANGE_FRAMES", raising=False)
    pal, streams = clip_of(shape, mode512)
    hip.set_palette(pal[0], pal[1], mode512)
    rng = np.random.default_rng(11)
    for n, fc in BATCHES:
        st = streams[fc:fc + n]
        stride = (max(len(b) for b in st) + 255) & ~255                # tight: the last region's pieces reach past it
        zeros, bpos = rows_of(st, stride)
        front, back = 2 * FRB + 4 * 37, 2 * FRB + 12                    # (a 4-byte aligned base that is not 256-byte aligned)
        big = flag_bytes(rng, front + n * stride + back)
        slab = big[front:front + n * stride].reshape(n, stride)
        for i, b in enumerate(st):
            slab[i, :len(b)] = b
        dbig = torch.from_numpy(big).cuda()
        dslab = dbig[front:front + n * stride].view(n, stride)
        assert dslab.data_ptr() % 4 == 0
        prev, previ = prior_of(shape, fc)
        z = gpu_rows(torch, hip, shape, torch.from_numpy(zeros).cuda(), bpos, fc, prev, previ)
        f = gpu_rows(torch, hip, shape, dslab, bpos, fc, prev, previ)
        what = "%dx%d n=%d fc=%d" % (shape + (n, fc))
        assert (f[1] == z[1]).all(), "nentered, " + what
        assert f[2] == z[2], "fallback frames %d against %d, %s" % (f[2], z[2], what)
        assert (f[0] == z[0]).all(), "pixels, " + what
        pix, nent = oracle_rows(shape, mode512, pal, zeros, bpos, fc, prev, previ)
        assert (z[1] == nent).all() and (z[0] == pix).all(), "zero-filled slab against the oracle, " + what


@pytest.mark.parametrize("mode512", [True, False], ids=["m512", "m256"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_tight_strides(torch, hip, monkeypatch, shape, mode512):
    """the stride right behind the longest stream; one whose distance from the start of the last region is no multiple of a
    piece; and a row that its stream fills to the last byte, and to 1, 2, 3 bytes before it"""
    monkeypatch.delenv("AGMV_DEC_GRID", raising=False)
    monkeypatch.delenv("AGMV_DEC_RANGE_FRAMES", raising=False)
    pal, streams = clip_of(shape, mode512)
    hip.set_palette(pal[0], pal[1], mode512)
    for n, fc in BATCHES:
        st = streams[fc:fc + n]
        longest = max(len(b) for b in st)
        tight = (longest + 255) & ~255
        odd = (longest + 3) & ~3
        while (odd - (odd - 1) // FRB * FRB) % FC == 0 or odd == tight:
            odd += 4
        for stride in (tight, odd):
            bits, bpos = rows_of(st, stride)
            check_rows(torch, hip, shape, mode512, pal, bits, bpos, fc, "stride %d n=%d fc=%d" % (stride, n, fc))
        # the row of the longest stream is full: bpos = stride - d (the stream cut there; the other rows as they are)
        full = longest & ~3
        k = max(range(n), key=lambda i: len(st[i]))
        for d in range(4):
            bits, bpos = rows_of(st, full)
            bpos[k] = full - d
            check_rows(torch, hip, shape, mode512, pal, bits, bpos, fc, "stride %d bpos[%d] = stride - %d n=%d fc=%d" % (full, k, d, n, fc))


@pytest.mark.parametrize("mode512", [True, False], ids=["m512", "m256"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_truncated_streams(torch, hip, monkeypatch, shape, mode512):
    """valid streams with bpos set to a few bytes, around a piece, around one and two regions: the bytes behind bpos are still
    those of the stream"""
    monkeypatch.delenv("AGMV_DEC_GRID", raising=False)
    monkeypatch.delenv("AGMV_DEC_RANGE_FRAMES", raising=False)
    pal, streams = clip_of(shape, mode512)
    hip.set_palette(pal[0], pal[1], mode512)
    for n, fc in BATCHES:
        st = streams[fc:fc + n]
        bits, full = rows_of(st, (max(len(b) for b in st) + 255) & ~255)
        for i0 in range(0, len(CUTS), n):                              # every frame of the batch cut at another of the lengths
            bpos = full.copy()
            for i, cut in enumerate(CUTS[i0:i0 + n]):
                bpos[i] = min(cut, full[i])
            check_rows(torch, hip, shape, mode512, pal, bits, bpos, fc, "bpos %s n=%d fc=%d" % (list(bpos), n, fc))
        for cut in CUTS:                                               # ... and all frames at the same
            bpos = np.minimum(full, cut).astype(np.int32)
            check_rows(torch, hip, shape, mode512, pal, bits, bpos, fc, "bpos %d n=%d fc=%d" % (cut, n, fc))


def block_frames(shape, mode512, n, copies):
    """n hand-made frames: every block of the frames in `copies` is a COPY, every block of the others a two-byte FILL"""
    nblk = shape[0] * shape[1] // 16
    out = []
    for f in range(n):
        if f in copies:
            out.append(np.full(nblk, 0x5E, np.uint8))
        else:
            b = np.empty((nblk, 2), np.uint8)
            b[:, 0] = 0x4E
            b[:, 1] = (np.arange(nblk) * 7 + f * 13) % 100
            out.append(b.reshape(-1))
    return out


@pytest.mark.parametrize("fc", [0, 2])
@pytest.mark.parametrize("mode512", [True, False], ids=["m512", "m256"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_ranges_pixels_and_prior_dependence(torch, monkeypatch, shape, mode512, fc):
    """13 frames in ranges of 4 (first_fc 0: 4 + 4 + 4 + 1; 2: 6 + 4 + 3) against the uncut call: the encoder's clip, and
    three hand-made clips that copy the caller's I-frame snapshot in range 0 only, in a later GOP's I-frame only (that reads
    the range before it: not dependent) and in both -- on a fresh context and on one that has just decoded a dependent batch"""
    from libagmv_amd import AgmvHip
    monkeypatch.delenv("AGMV_DEC_GRID", raising=False)
    n = 13
    pal, streams = clip_of(shape, mode512)
    late = 8 if fc == 0 else 10                                        # an I-frame in the third range
    clips = {"encoded": streams[fc:fc + n], "range 0": block_frames(shape, mode512, n, {0}),
             "later": block_frames(shape, mode512, n, {late}), "both": block_frames(shape, mode512, n, {0, late})}
    prev, previ = prior_of(shape, fc)
    if previ is None:
        prev, previ = prior_of(shape, 1)                                # (COPY in the first I-frame reads the snapshot handed in)
    for stale in (False, True):
        t = AgmvHip(0)
        try:
            t.set_palette(pal[0], pal[1], mode512)
            for name, st in clips.items():
                bits, bpos = rows_of(st, (max(len(b) for b in st) + 255) & ~255)
                dbits = torch.from_numpy(bits).cuda()
                monkeypatch.setenv("AGMV_DEC_RANGE_FRAMES", "0")
                whole = gpu_rows(torch, t, shape, dbits, bpos, fc, prev, previ)
                if stale:                                              # leave a set prior-dependence word behind
                    dep_bits, dep_bpos = rows_of(clips["both"], 2 * (shape[0] * shape[1] // 16))
                    monkeypatch.setenv("AGMV_DEC_RANGE_FRAMES", "4")
                    assert gpu_rows(torch, t, shape, torch.from_numpy(dep_bits).cuda(), dep_bpos, fc, prev, previ)[3]
                monkeypatch.setenv("AGMV_DEC_RANGE_FRAMES", "4")
                cut = gpu_rows(torch, t, shape, dbits, bpos, fc, prev, previ)
                what = "%s, fc %d, %s context" % (name, fc, "used" if stale else "fresh")
                assert (cut[0] == whole[0]).all() and (cut[1] == whole[1]).all(), "pixels / nentered: " + what
                assert cut[3] == whole[3], "prior dependence %d, uncut %d: %s" % (cut[3], whole[3], what)
                if name == "later":
                    assert cut[3] == 0, what
                if name in ("range 0", "both"):
                    assert cut[3] == 1, what
                pix, nent = oracle_rows(shape, mode512, pal, bits, bpos, fc, prev, previ)
                assert (whole[0] == pix).all() and (whole[1] == nent).all(), "uncut call against the oracle: " + what
        finally:
            t.close()


@pytest.mark.parametrize("n,fc", [(9, 0), (13, 2)], ids=["n9-fc0", "n13-fc2"])
@pytest.mark.parametrize("mode512", [True, False], ids=["m512", "m256"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_timing_marks_over_three_ranges(torch, monkeypatch, shape, mode512, n, fc):
    """three ranges of 4 frames (9 frames from first_fc 0: 4 + 4 + 1; 13 from first_fc 2: 6 + 4 + 3; 5 frames, or 9 from first_fc
    2, are two ranges at most) with timing on: parser and k_decode + k_fixup times are positive and together fit inside the
    call as two torch events on the same stream see it (+ 0.1 ms); with timing off the outputs are byte for byte the same"""
    from libagmv_amd import AgmvHip
    monkeypatch.delenv("AGMV_DEC_GRID", raising=False)
    monkeypatch.setenv("AGMV_DEC_RANGE_FRAMES", "4")
    pal, streams = clip_of(shape, mode512)
    st = streams[fc:fc + n]
    assert len(st) == n
    bits, bpos = rows_of(st, (max(len(b) for b in st) + 255) & ~255)
    dbits, dbpos = torch.from_numpy(bits).cuda(), torch.from_numpy(bpos).cuda()
    prev, previ = prior_of(shape, fc)
    dprev, dprevi = dev_u32(torch, prev), dev_u32(torch, previ)
    t = AgmvHip(0)
    try:
        t.set_palette(pal[0], pal[1], mode512)
        outs = {}
        for on in (True, False):
            t.enable_timing(on)
            nent = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            for _ in range(3):                                         # (the first call allocates)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = t.decode_bitstreams_dev(dbits, dbpos, n, shape[0], shape[1], fc, nentered=nent, prev=dprev, prev_iframe=dprevi)
                e1.record()
            torch.cuda.synchronize()
            outs[on] = (to_u32(out).copy(), nent.cpu().numpy().copy())
            if on:
                parse, dec, call = (t.last_kernel_ms(k) for k in (1, 2, 3))
                span = e0.elapsed_time(e1)
                print("parser %.4f, k_decode + k_fixup %.4f, call %.4f, between torch events %.4f ms" % (parse, dec, call, span))
                assert parse > 0 and dec > 0
                assert parse + dec <= span + 0.1
                assert parse + dec <= call <= span + 0.1
        assert (outs[True][0] == outs[False][0]).all() and (outs[True][1] == outs[False][1]).all()
        pix, nent = oracle_rows(shape, mode512, pal, bits, bpos, fc, prev, previ)
        assert (outs[True][0].reshape(n, -1) == pix).all() and (outs[True][1] == nent).all()
    finally:
        t.close()
