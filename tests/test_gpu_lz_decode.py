"""The decoder's LZ stage on the GPU (agmv_hip_lz_decode_frames_dev / _commit_dev, AgmvHip.lz_decode_*) against the host
stage agmv_lz_decode_mem run frame by frame over one persistent buffer (tests/lz_decode_cases.py).  Every check compares
bpos, used, every output byte, the 16 tail bytes after a commit and the persistent buffer, and that bytes of a row behind
bpos (before the commit) and behind bpos + 16 (after it) keep what they held."""
import hashlib
import os

import numpy as np
import pytest

import hostlib as H
import lz_decode_cases as Z
from lz_decode_cases import Frame, lz77_frame, lzss_frame

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
LZSS_VERSIONS = (1, 2)
ALL_VERSIONS = (1, 2, 3, 4, 9)


@pytest.fixture(scope="module")
def hip():
    import torch
    from libagmv_amd import AgmvHip
    assert torch.cuda.is_available()
    h = AgmvHip(0)
    yield h
    h.close()


def _i32(a):
    import torch
    return torch.from_numpy(np.asarray(a, np.int64).astype(np.uint32).view(np.int32).copy()).cuda()


def upload(frames):
    import torch
    src, off, avail = Z.image(frames)
    return (torch.from_numpy(src).cuda(), torch.from_numpy(off).cuda(), _i32(avail),
            _i32([f.usize for f in frames]), _i32([f.csize for f in frames]))


def host_sizes(frames):
    """avail, usize, csize as host arrays: lz_decode_frames_dev then calls agmv_hip_lz_decode_frames_sized_dev"""
    _, _, avail = Z.image(frames)
    return avail, np.array([f.usize for f in frames], np.int64), np.array([f.csize for f in frames], np.int64)


def run(hip, version, frames, cap, persist=None, stride=None, commit_n=None, fallback=None, sized=False):
    """one lz_decode_frames_dev + lz_decode_commit_dev call on image(frames), checked against the host batch reference.
    Returns (bpos, used, fallback frames)."""
    import torch
    n = len(frames)
    stride = cap if stride is None else stride
    rng = np.random.default_rng(n * 7 + cap)
    per0 = rng.integers(0, 256, cap, dtype=np.uint8) if persist is None else np.asarray(persist, np.uint8)
    src, off, avail, us, cs = upload(frames)
    if sized:
        avail, us, cs = host_sizes(frames)
    bits = torch.full((n, stride), SENTINEL, dtype=torch.uint8, device="cuda")
    bits, bpos, used = hip.lz_decode_frames_dev(version, src, off, avail, us, cs, n, cap, bits=bits)
    fb = hip.lz_decode_fallback_frames()
    s_src, s_off, s_avail = Z.image(frames)
    hrows, hbpos, hused = Z.host_lz(version, s_src, s_off, s_avail, [f.usize for f in frames], [f.csize for f in frames], cap, stride)
    gb = bpos.cpu().numpy().view(np.uint32).astype(np.int64)
    gu = used.cpu().numpy().view(np.uint32).astype(np.int64)
    assert (gb == hbpos).all(), np.nonzero(gb != hbpos)[0][:8]
    assert (gu == hused).all(), np.nonzero(gu != hused)[0][:8]
    exp = np.full((n, stride), SENTINEL, np.uint8)
    for f in range(n):
        exp[f, :hbpos[f]] = hrows[f, :hbpos[f]]
    got = bits.cpu().numpy()
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, "rows differ: %s" % bad[:8]
    if fallback is not None:
        assert fb == fallback if isinstance(fallback, int) else fallback(fb), fb
    m = n if commit_n is None else commit_n
    per = torch.from_numpy(per0.copy()).cuda()
    hip.lz_decode_commit_dev(bits, bpos, m, per)
    exp, eper = Z.commit(exp, hbpos, per0.copy(), m)
    got = bits.cpu().numpy()
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, "rows after the commit differ: %s" % bad[:8]
    assert (per.cpu().numpy() == eper).all()
    return hbpos, hused, fb


# ---------------------------------------------------------------------------------------------------------------------
# round trips of compressor output
# ---------------------------------------------------------------------------------------------------------------------
def compressed(version, xs):
    fr = []
    for x in xs:
        comp, c = H.lzss(x) if version in LZSS_VERSIONS else H.lz77(x)
        fr.append(Frame(comp, len(x), c))
    return fr


@pytest.mark.parametrize("version", ALL_VERSIONS)
def test_roundtrip_small_inputs(hip, version):
    from test_hostlib import lz_cases
    xs = list(lz_cases()) + Z.splash_rng_cases(np.random.default_rng(version))
    fr = compressed(version, xs)
    cap = max(len(x) for x in xs) + 64
    run(hip, version, fr, cap, fallback=0)


def test_roundtrip_gpu_lzss_output(hip):
    import torch
    xs = Z.splash_rng_cases(np.random.default_rng(5))
    n = len(xs)
    stride = max(len(x) for x in xs) + 1
    b = np.zeros((n, stride), np.uint8)
    for i, x in enumerate(xs):
        b[i, :len(x)] = x
    out, cs = hip.lzss_frames_dev(torch.from_numpy(b).cuda(), torch.tensor([len(x) for x in xs], dtype=torch.int32).cuda(), n)
    out, cs = out.cpu().numpy(), cs.cpu().numpy()
    fr = [Frame(out[i, :cs[i]], len(xs[i]), cs[i]) for i in range(n)]
    for f in range(n):
        assert bytes(compressed(1, [xs[f]])[0].payload) == fr[f].payload
    run(hip, 1, fr, stride + 64, fallback=0)


def test_roundtrip_1080p_frames_encoded_on_the_gpu(hip):
    import torch
    import synth as S
    W, Hh, T = 1920, 1080, 3
    frames = np.stack([S.synth_frame(W, Hh, t) for t in range(T)])
    p0, p1 = S.content_palettes(frames[:2])
    hip.set_palette(p0, p1, True)
    out, sizes = hip.encode_dev(torch.from_numpy(frames.view(np.int32)).cuda(), T, W, Hh)
    pay, cs = hip.lzss_frames_dev(out, sizes, T)
    pay, cs, sizes = pay.cpu().numpy(), cs.cpu().numpy(), sizes.cpu().numpy()
    fr = [Frame(pay[i, :cs[i]], sizes[i], cs[i]) for i in range(T)]
    bp, _, _ = run(hip, 1, fr, hip.max_usize(W, Hh) + 4096, fallback=0)
    assert (bp >= sizes).all()
    xs = [out[i, :sizes[i]].cpu().numpy() for i in range(T)]
    run(hip, 3, compressed(3, xs), hip.max_usize(W, Hh) + 4096, fallback=0)


# ---------------------------------------------------------------------------------------------------------------------
# crafted streams
# ---------------------------------------------------------------------------------------------------------------------
def crafted_lzss():
    L = lambda b: ("L", b)                                                   # noqa: E731
    M = lambda o, n: ("M", o, n)                                             # noqa: E731
    cases = [
        [L(1), M(0, 9), L(2), M(0, 15)],                                     # offset 0: nothing copied
        [L(5), L(6), M(1, 0), M(2, 1), M(2, 2), M(1, 15)],                   # len 0, 1, 2; overlapping copies
        [M(3, 5)],                                                           # offset > pos at pos 0 (last token)
        [L(1), L(2), M(7, 9)],                                               # offset > pos, partial copy, last token
        [L(1), L(2), M(7, 3)],                                               # ... nothing left to copy
        [L(9)] * 30,                                                         # usize reached by a literal (usize set below)
        [L(3), M(1, 15), M(1, 15)],                                          # a match that runs past usize
        [L(7)] + [M(1, 15)] * 400,                                           # a long offset-1 chain
        [],                                                                  # csize 0
    ]
    fr = [lzss_frame(t) for t in cases]
    fr[5].usize = 17
    fr[6].usize = 20
    fr.append(Frame(b"", 0, 0))                                              # usize 0
    fr.append(Frame(b"\xff\xff\xff", 0, 3))                                  # usize 0, csize > 0
    fr.append(lzss_frame([L(4), L(5), M(2, 12)] * 3, csize=40))             # csize runs into the guard
    g = lzss_frame([L(i) for i in range(50)])
    fr.append(Frame(g.payload, g.usize, g.csize, avail=20))                  # avail < csize: zeros, used capped
    fr.append(Frame(g.payload, g.usize, g.csize + 100, avail=len(g.payload) + 5))
    return fr


def crafted_lz77():
    cases = [
        [(0, 9, 1), (0, 0, 2), (1, 0, 3)],                                   # offset 0, len 0
        [(0, 0, 5), (1, 1, 6), (2, 2, 7), (1, 255, 8)],                      # len 1, 2, 255
        [(3, 5, 1)],                                                         # offset > pos at pos 0
        [(0, 0, 1), (0, 0, 2), (7, 9, 3)],                                   # offset > pos, partial copy, last token
        [(0, 0, 7)] + [(1, 255, 7)] * 40,                                    # a long offset-1 chain
        [],
    ]
    fr = [lz77_frame(t) for t in cases]
    for r in (1, 2, 3):                                                       # csize % 4 in {1, 2, 3}
        g = lz77_frame([(0, 0, 1), (1, 3, 2), (2, 4, 3)])
        fr.append(Frame(g.payload, g.usize, g.csize - 4 + r))
        fr.append(Frame(g.payload, g.usize, g.csize + r))
    g = lz77_frame([(0, 0, i) for i in range(40)])
    fr.append(Frame(g.payload, g.usize, g.csize, avail=30))
    fr.append(Frame(g.payload, g.usize, 5000, avail=len(g.payload) + 9))       # zero tail
    return fr


@pytest.mark.parametrize("cap", [64, 1100, 9000])
def test_crafted_lzss(hip, cap):
    """cap 64: lim = 48 is reached in the middle of matches"""
    for v in LZSS_VERSIONS:
        run(hip, v, crafted_lzss(), cap)


@pytest.mark.parametrize("cap", [17, 64, 1100, 20000])
def test_crafted_lz77(hip, cap):
    for v in (3, 4, 200):
        run(hip, v, crafted_lz77(), cap)


def test_offset_one_chain_the_length_of_a_frame(hip):
    n = 15 * 60000
    fr = [lzss_frame([("L", 0x5A)] + [("M", 1, 15)] * (n // 15))]
    bp, _, _ = run(hip, 1, fr, n + 64, fallback=0)
    assert bp[0] == n + 1
    fr = [lz77_frame([(0, 0, 0x5A)] + [(1, 255, 0x11)] * 3000)]
    run(hip, 3, fr, 256 * 3000 + 64, fallback=0)


@pytest.mark.parametrize("version", [1, 3])
def test_csize_far_beyond_avail_is_closed_form(hip, version):
    """csize 2^28 with a few hundred readable bytes: the tail of zero tokens is settled in closed form"""
    if version == 1:
        g = lzss_frame([("L", i) for i in range(200)])
    else:
        g = lz77_frame([(0, 0, i) for i in range(200)])
    fr = [Frame(g.payload, 1 << 30, 1 << 28, avail=len(g.payload) + 3), Frame(g.payload, 5000, (1 << 28) + 3, avail=len(g.payload)),
          Frame(g.payload, 1 << 30, (1 << 28) + 1)]                          # (this one reads on into the next chunk)
    bp, used, _ = run(hip, version, fr, 70000)
    assert used[0] == len(g.payload) + 3 and used[1] == len(g.payload)


# ---------------------------------------------------------------------------------------------------------------------
# fallback: encoder output never needs it; a match with offset > pos followed by tokens does
# ---------------------------------------------------------------------------------------------------------------------
def last_lzss_token(payload, usize, csize, guard=Z.GUARD):
    """(offset, pos) of the last token the reader takes when it is a match, else None"""
    data = int.from_bytes(bytes(payload) + guard, "little")
    b = pos = 0
    last = None
    while b < 8 * csize and pos < usize:
        if (data >> b) & 1:
            pos += 1
            b += 9
            last = None
        else:
            o, n = (data >> (b + 1)) & 0xFFFF, (data >> (b + 17)) & 15
            last = (o, pos)
            pos += n if 0 < o <= pos else 0
            b += 21
    return last


def test_encoder_output_whose_last_match_reads_guard_bits(hip):
    rng = np.random.default_rng(11)
    fr, wrapped = [], 0
    for n in range(3, 400):
        x = np.tile(rng.integers(0, 4, 3, dtype=np.uint8), n // 3 + 1)[:n]
        comp, c = H.lzss(x)
        t = last_lzss_token(comp, n, c)
        fr.append(Frame(comp, n, c))
        wrapped += t is not None and t[0] > t[1]
    assert wrapped > 10, wrapped
    run(hip, 1, fr, 512, fallback=0)


def test_fallback_frames_are_exact_and_counted(hip):
    mid = [lzss_frame([("L", 1), ("L", 2), ("M", 9, 12), ("L", 3), ("M", 1, 5)]),
           lzss_frame([("M", 4, 4), ("L", 6), ("M", 1, 15)])]
    good = compressed(1, Z.splash_rng_cases(np.random.default_rng(3)))
    run(hip, 1, mid, 256, fallback=2)
    run(hip, 1, good[:5] + mid[:1] + good[5:] + mid[1:], 6000, fallback=2)
    mid77 = [lz77_frame([(0, 0, 1), (5, 9, 2), (1, 3, 4)]), lz77_frame([(2, 2, 2), (0, 0, 5)])]
    run(hip, 3, compressed(3, Z.splash_rng_cases(np.random.default_rng(4))) + mid77, 6000, fallback=2)
    big = lz77_frame([(0, 0, 1)] + [(1, 255, 2)] * 8, usize=10)              # output far past usize + 256
    run(hip, 3, [big], 4096, fallback=1)


# ---------------------------------------------------------------------------------------------------------------------
# LZSS pieces (2048 bits): a token straddles a boundary at every entry offset 0..20
# ---------------------------------------------------------------------------------------------------------------------
def boundary_frame(boundary, e, tl):
    s = boundary + e - tl                                                    # the token [s, s + tl) ends e bits into the piece
    rest = s - 9
    for nm in range(3):
        if rest - 21 * nm >= 0 and (rest - 21 * nm) % 9 == 0:
            break
    else:
        return None
    toks = [("L", 0x33)] + [("M", 1, 3)] * nm + [("L", (i * 7) & 255) for i in range((rest - 21 * nm) // 9)]
    toks += [("M", 2, 9) if tl == 21 else ("L", 0xC4)] + [("L", 9), ("M", 3, 4), ("L", 8)] * 40
    return lzss_frame(toks)


def test_tokens_straddling_piece_boundaries_at_every_entry(hip):
    fr, seen = [], set()
    for m in (1, 2, 3):
        for e in range(21):
            for tl in (9, 21):
                if e >= tl or (m * 2048 + e - tl) % 3:
                    continue
                f = boundary_frame(m * 2048, e, tl)
                if f is not None:
                    fr.append(f)
                    seen.add(e)
    assert seen == set(range(21)), sorted(set(range(21)) - seen)
    run(hip, 1, fr, 8192, fallback=0)
    run(hip, 2, fr[::-1], 8192, fallback=0)


# ---------------------------------------------------------------------------------------------------------------------
# the persistent buffer
# ---------------------------------------------------------------------------------------------------------------------
def lit_frame(n, seed):
    rng = np.random.default_rng(seed)
    return lzss_frame([("L", int(b)) for b in rng.integers(0, 256, n)])


def test_persistent_buffer_with_rising_and_falling_bpos(hip):
    fr = [lit_frame(n, i) for i, n in enumerate((100, 5000, 30, 5000, 4990, 0, 6000, 17, 6000, 5999))]
    run(hip, 1, fr, 8192)
    run(hip, 1, fr, 6016)                                                    # bpos at lim: tails end at cap
    run(hip, 1, fr, 8192, stride=8200)


def test_commit_of_fewer_frames_and_chained_commits(hip):
    import torch
    fr = [lit_frame(n, i) for i, n in enumerate((300, 40, 700, 700, 10, 0, 900, 5, 640))]
    run(hip, 1, fr, 1024, commit_n=4)
    cap = 1024
    eper = np.random.default_rng(1).integers(0, 256, cap, dtype=np.uint8)
    per = torch.from_numpy(eper.copy()).cuda()
    for lo, hi in ((0, 3), (3, 4), (4, 9)):
        part = fr[lo:hi]
        src, off, avail, us, cs = upload(part)
        bits = torch.full((len(part), cap), SENTINEL, dtype=torch.uint8, device="cuda")
        bits, bpos, used = hip.lz_decode_frames_dev(1, src, off, avail, us, cs, len(part), cap, bits=bits)
        hip.lz_decode_commit_dev(bits, bpos, len(part), per)
        _, exp, eb, _, eper = Z.host_batch(1, part, cap, persist=eper)
        got = bits.cpu().numpy()
        for f in range(len(part)):
            e = min(int(eb[f]) + 16, cap)
            assert (got[f, :e] == exp[f, :e]).all() and (got[f, e:] == SENTINEL).all(), (lo, f)
        assert (per.cpu().numpy() == eper).all(), (lo, hi)


# ---------------------------------------------------------------------------------------------------------------------
# batch shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_batch_sizes(hip, n):
    rng = np.random.default_rng(n)
    xs = [rng.integers(0, int(rng.integers(1, 9)), int(rng.integers(0, 700)), dtype=np.uint8) for _ in range(n)]
    for v in (1, 3):
        run(hip, v, compressed(v, xs), 768, fallback=0)


def test_70000_tiny_frames_in_one_call(hip):
    rng = np.random.default_rng(70)
    xs = [rng.integers(0, 3, int(rng.integers(0, 9)), dtype=np.uint8) for _ in range(70000)]
    run(hip, 1, compressed(1, xs), 32, fallback=0)


def test_work_areas_grow_and_shrink(hip):
    rng = np.random.default_rng(8)
    for n, m in ((3, 200), (40, 20000), (2, 10), (300, 3000), (1, 70000)):
        xs = [rng.integers(0, 5, m, dtype=np.uint8) for _ in range(n)]
        run(hip, 1 if n % 2 else 3, compressed(1 if n % 2 else 3, xs), m + 300, fallback=0)


def test_sizes_from_host_memory(hip):
    """agmv_hip_lz_decode_frames_sized_dev (no stream synchronisation) gives what the device-size form gives"""
    run(hip, 1, crafted_lzss(), 1100, sized=True)
    run(hip, 3, crafted_lz77(), 1100, sized=True)
    run(hip, 1, compressed(1, Z.splash_rng_cases(np.random.default_rng(6))), 6000, fallback=0, sized=True)


# ---------------------------------------------------------------------------------------------------------------------
# chunks cut by the word limit (2^26 output positions) and the piece limit (2^18 pieces of 2048 bits); work areas that
# are sized per array across calls of other shapes
# ---------------------------------------------------------------------------------------------------------------------
def run_lean(hip, version, frames, cap, sized=False):
    """run() for rows too large to mirror whole on the host: bpos, used, every byte of [0, bpos), the 16 tail bytes after a
    commit from a zero buffer, 4 KiB of untouched bytes behind them, and the buffer"""
    import ctypes as C
    import torch
    n = len(frames)
    src, off, avail = Z.image(frames)
    dsrc = torch.from_numpy(src).cuda()
    doff = torch.from_numpy(off).cuda()
    sizes = host_sizes(frames) if sized else (_i32(avail), _i32([f.usize for f in frames]), _i32([f.csize for f in frames]))
    bits = torch.full((n, cap), SENTINEL, dtype=torch.uint8, device="cuda")
    bits, bpos, used = hip.lz_decode_frames_dev(version, dsrc, doff, *sizes, n, cap, bits=bits)
    per = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    hip.lz_decode_commit_dev(bits, bpos, n, per)
    gb = bpos.cpu().numpy().view(np.uint32)
    gu = used.cpu().numpy().view(np.uint32)
    eper = np.zeros(cap, np.uint8)
    row = np.zeros(cap, np.uint8)
    for f in range(n):
        u = C.c_size_t(0)
        b = H.lib().agmv_lz_decode_mem(version, np.ascontiguousarray(src[off[f]:off[f] + avail[f]]), int(avail[f]), frames[f].usize,
                                       frames[f].csize, row, cap, C.byref(u))
        assert (int(gb[f]), int(gu[f])) == (b, u.value), f
        e = min(b + 16, cap)
        exp = row[:e].copy()
        exp[b:e] = eper[b:e]
        got = bits[f, :min(e + 4096, cap)].cpu().numpy()
        assert (got[:e] == exp).all() and (got[e:] == SENTINEL).all(), f
        eper[:b] = row[:b]
    assert (per.cpu().numpy() == eper).all()
    return gb, gu


def test_chunks_cut_by_the_word_limit_and_a_frame_beyond_it(hip):
    """two frames of 30 M output positions share a chunk, a third of 2^26 + 4096 (more than a chunk holds) has one alone"""
    fr = [Z.chain_frame(2_000_000), Z.chain_frame(2_000_000, lead=7), Z.chain_frame(((1 << 26) + 4096) // 15, lead=9)]
    bp, _ = run_lean(hip, 1, fr, (1 << 26) + 8192)
    assert bp[2] > 1 << 26
    assert hip.lz_decode_fallback_frames() == 0


def zero_frame(nbytes, usize):
    """nbytes of zero payload: 21-bit zero-length matches, no output; the walk covers all of it"""
    return Frame(bytes(nbytes), usize, nbytes)


def test_chunks_cut_by_the_piece_limit(hip):
    """3 frames of 2^17 + 100 pieces: no two fit in one chunk of 2^18 pieces"""
    fr = [zero_frame(((1 << 17) + 100) * 256, 50) for _ in range(3)]
    run_lean(hip, 1, fr, 128)
    run_lean(hip, 1, fr[:2] + [lit_frame(40, 3)], 128, sized=True)


def test_work_areas_sized_per_array_across_calls():
    """frame tables (one entry per frame) and piece bases (one per frame and chunk) grow each on its own need: a call of
    fewer frames in more chunks after one of more frames in one chunk, and a call of more frames in one chunk after one of
    fewer frames in several chunks (word limit: frames of 12 M output positions, five per chunk).  A context of its own, so
    the work areas start from these calls' sizes."""
    from libagmv_amd import AgmvHip
    hip = AgmvHip(0)
    run(hip, 1, [lit_frame(30, i) for i in range(4)], 128)
    run_lean(hip, 1, [zero_frame(((1 << 17) + 100) * 256, 50) for _ in range(3)], 128)
    big = [zero_frame(1 << 20, 12_000_000) for _ in range(12)]
    run_lean(hip, 1, big, 12_000_064)
    run(hip, 1, [lit_frame(30, i) for i in range(13)], 128)
    run_lean(hip, 1, big[:7], 12_000_064, sized=True)
    run(hip, 3, compressed(3, Z.splash_rng_cases(np.random.default_rng(9))), 6000, fallback=0)
    hip.close()


def test_zero_frames(hip):
    import torch
    z = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.lz_decode_frames_dev(1, torch.zeros(1, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"),
                             z, z, z, 0, 64, bits=torch.zeros((1, 64), dtype=torch.uint8, device="cuda"), bpos=z.clone(), used=z.clone())
    assert hip.lz_decode_fallback_frames() == 0


# ---------------------------------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_wrapper_rejects_what_it_would_misread(hip):
    import torch
    fr = [lit_frame(10, 1), lit_frame(20, 2)]
    src, off, avail, us, cs = upload(fr)
    ok = dict(bits=torch.zeros((2, 64), dtype=torch.uint8, device="cuda"))
    bad = [
        (src.cpu(), off, avail, us, cs, {}),
        (src.to(torch.int32), off, avail, us, cs, {}),
        (src, off.to(torch.int32), avail, us, cs, {}),
        (src, off[:1], avail, us, cs, {}),
        (src, off, avail.to(torch.int64), us, cs, {}),
        (src, off, avail, us[:1], cs, {}),
        (src, off, avail, us, cs.cpu(), {}),
        (src, off, avail, us, cs, dict(bits=torch.zeros((1, 64), dtype=torch.uint8, device="cuda"))),
        (src, off, avail, us, cs, dict(bits=torch.zeros((2, 64), dtype=torch.int32, device="cuda"))),
        (src, off, avail, us, cs, dict(bits=torch.zeros((64, 2), dtype=torch.uint8, device="cuda").t())),
        (src, off, avail, us, cs, dict(bits=torch.zeros((2, 32), dtype=torch.uint8, device="cuda"))),
        (src, off, avail, us, cs, dict(bpos=torch.zeros(2, dtype=torch.int64, device="cuda"), **ok)),
        (src, off, avail, us, cs, dict(used=torch.zeros(1, dtype=torch.int32, device="cuda"), **ok)),
    ]
    for a in bad:
        with pytest.raises(ValueError):
            hip.lz_decode_frames_dev(1, a[0], a[1], a[2], a[3], a[4], 2, 64, **a[5])
    bits, bpos, used = hip.lz_decode_frames_dev(1, src, off, avail, us, cs, 2, 64, **ok)
    for args in ((bits.cpu(), bpos, 2, torch.zeros(64, dtype=torch.uint8, device="cuda")),
                 (bits, bpos.to(torch.int64), 2, torch.zeros(64, dtype=torch.uint8, device="cuda")),
                 (bits, bpos, 3, torch.zeros(64, dtype=torch.uint8, device="cuda")),
                 (bits, bpos, 2, torch.zeros(64, dtype=torch.int32, device="cuda")),
                 (bits, bpos, 2, torch.zeros(64, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            hip.lz_decode_commit_dev(*args)
    with pytest.raises(ValueError):
        hip.lz_decode_frames(1, [np.zeros(3, np.uint8)], [1, 2], [3], 64)


def test_host_form_matches_the_batch_reference(hip):
    fr = compressed(1, Z.splash_rng_cases(np.random.default_rng(2)))
    src, off, avail = Z.image(fr)
    pays = [src[off[i]:] for i in range(len(fr))]
    per0 = np.random.default_rng(4).integers(0, 256, 6000, dtype=np.uint8)
    rows, bpos, used, per = hip.lz_decode_frames(1, pays, [f.usize for f in fr], [f.csize for f in fr], 6000, persist=per0)
    before, exp, eb, eu, eper = Z.host_batch(1, fr, 6000, persist=per0)
    assert (bpos == eb).all() and (used == eu).all() and (per == eper).all()
    for f in range(len(fr)):
        e = min(int(eb[f]) + 16, 6000)
        assert (rows[f, :e] == exp[f, :e]).all(), f


# ---------------------------------------------------------------------------------------------------------------------
# device-resident decode of whole files: lz_decode -> commit -> decode_bitstreams_dev
# ---------------------------------------------------------------------------------------------------------------------
def walk_chunks(data, first, nframes, version, cap):
    """chunk positions as the reference's reader finds them (the host LZ stage decides where each reader stops), and the
    host stage's bpos / used there"""
    import ctypes as C
    buf = np.frombuffer(data, np.uint8)
    off, avail, us, cs, used, bpos = [], [], [], [], [], []
    pos = first
    for _ in range(nframes):
        c = data.find(b"AGFC", pos)
        if c < 0 or c + 16 > len(data):
            break
        u = int.from_bytes(data[c + 8:c + 12], "little")
        s = int.from_bytes(data[c + 12:c + 16], "little")
        row = np.zeros(cap, np.uint8)
        got = C.c_size_t(0)
        bpos.append(H.lib().agmv_lz_decode_mem(version, np.ascontiguousarray(buf[c + 16:]), len(data) - c - 16, u, s, row, cap,
                                               C.byref(got)))
        off.append(c + 16); avail.append(len(data) - c - 16); us.append(u); cs.append(s); used.append(got.value)
        pos = c + 16 + got.value
    return off, avail, us, cs, used, bpos


def device_resident_decode(hip, data):
    """a whole file image through lz_decode_frames_dev -> lz_decode_commit_dev -> decode_bitstreams_dev, the rows never on
    the host; used and bpos checked against the host stage.  Returns (w, h, bpos, pixels u32 [n, w*h])"""
    import ctypes as C
    import torch
    import oracles as O
    buf = np.frombuffer(data, np.uint8).copy()
    info = O._FileInfo()
    p0 = np.zeros(256, np.uint32)
    p1 = np.zeros(256, np.uint32)
    assert O.oracle().orc_parse_header(buf, len(buf), C.byref(info), p0, p1) == 0
    w, h, ver = info.w, info.h, info.version
    cap = w * h * 33 // 16 + 4096
    stride = (cap + 255) & ~255
    off, avail, us, cs, used, hbpos = walk_chunks(data, info.first_chunk, info.num_frames, ver, cap)
    n = len(off)
    src = torch.from_numpy(buf).cuda()
    bits = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
    bits, bpos, gused = hip.lz_decode_frames_dev(ver, src, torch.tensor(off, dtype=torch.int64).cuda(), _i32(avail), _i32(us), _i32(cs),
                                                 n, cap, bits=bits)
    assert hip.lz_decode_fallback_frames() == 0
    assert (gused.cpu().numpy() == np.array(used)).all()
    assert (bpos.cpu().numpy() == np.array(hbpos)).all()
    persist = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    hip.lz_decode_commit_dev(bits, bpos, n, persist)
    hip.set_palette(p0, p1, ver in (1, 3))
    pix = hip.decode_bitstreams_dev(bits, bpos, n, w, h)
    return w, h, bpos.cpu().numpy(), pix.cpu().numpy().view(np.uint32).reshape(n, -1)


@pytest.mark.parametrize("name", ["agmv_splash", "FOXLOGO"])
def test_device_resident_file_decode_matches_golden_pixels(hip, golden, golden_fox, golden_dir, name):
    g = golden["agmv_splash"] if name == "agmv_splash" else golden_fox["FOXLOGO"]
    _, _, bpos, pix = device_resident_decode(hip, open(os.path.join(golden_dir, name + ".agmv"), "rb").read())
    assert len(pix) == g["n"] and (bpos == np.array(g["bpos"][:g["n"]])).all()
    for k in range(len(pix)):
        assert hashlib.sha256(pix[k].tobytes()).hexdigest() == g["pix_sha"][k], k


def test_device_resident_lz77_file_decode_matches_golden_bmps(hip, golden, tmp_path):
    """the LZ77 file case (written by this library, byte-identical to the reference's): its BMPs, written from the device
    decode's pixels with the library's BMP writer, are the reference's"""
    from test_gpu_lz_decode_files import encode
    g = golden["files"]["agmv_opt2_low_lz77_160x128"]
    f = encode(tmp_path, g["driver"], g["T"], g["W"], g["H"], g["opt"], g["quality"], g["compression"])
    data = open(f, "rb").read()
    assert hashlib.sha256(data).hexdigest() == g["file_sha"]
    w, h, _, pix = device_resident_decode(hip, data)
    assert len(pix) == g["frames"]
    sha = hashlib.sha256()
    for k in range(len(pix)):
        H.write_bmp(str(tmp_path / "dev.bmp"), pix[k].reshape(h, w))
        sha.update(open(tmp_path / "dev.bmp", "rb").read())
    assert sha.hexdigest() == g["decoded_bmps_sha"]
