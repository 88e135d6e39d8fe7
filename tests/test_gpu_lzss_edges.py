"""The LZSS stage on the GPU (agmv_hip_lzss_frames_dev) at the edges its host driver and kernels are built around
(libagmv_amd/csrc/agmv_lz_hip.hip, DESIGN.md section 4 "LZSS stage"): chunks cut at 256 frames and at 2^24 positions,
parse pieces of 512 positions entered at carries 1..14, frames back to back in one chunk, the 65535-byte window of a frame
deep inside a chunk, the row contract and error returns of include/agmv_hip.h, reuse of a context's work areas, and the
file pipeline with batches of several chunks.

References: the brute-force restatement (orc_lzss_compress) for frames up to a few KB, the host stage (agmv_lzss_mem, pinned
against the brute force by the CPU suite) for larger ones, and the same frames through the GPU one call each.  Every check
compares csize and every payload byte."""
import hashlib

import numpy as np
import pytest

import children as K
import hostlib as H
import lzss_cases as Z
from lzss_cases import gpu_batch, orc

pytestmark = pytest.mark.gpu

CHUNK = 1 << 24                 # LZ_CHUNK: positions per chunk
CHUNK_FRAMES = 256              # LZ_CHUNK_FRAMES: frames per chunk
WIN = 65535
PIECE = 512


@pytest.fixture(scope="module")
def hip():
    import torch
    from libagmv_amd import AgmvHip
    assert torch.cuda.is_available()
    h = AgmvHip(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def debruijn():
    return Z.de_bruijn3()


def same(got, exp, what):
    assert len(got) == len(exp), "%s: csize %d, expected %d" % (what, len(got), len(exp))
    if len(exp):
        d = np.nonzero(got != exp)[0]
        assert len(d) == 0, "%s: payload byte %d of %d differs" % (what, d[0], len(exp))


def check_brute(got, streams, what=""):
    cache = {}
    for i, x in enumerate(streams):
        key = x.tobytes()
        if key not in cache:
            cache[key] = orc(x)
        same(got[i], cache[key], "%s frame %d (%d bytes)" % (what, i, len(x)))


def check_host(got, streams, what=""):
    cache = {}
    for i, x in enumerate(streams):
        key = (len(x), hashlib.sha1(x.tobytes()).digest())
        if key not in cache:
            cache[key] = H.lzss(x)[0]
        same(got[i], cache[key], "%s frame %d (%d bytes)" % (what, i, len(x)))


def check_one_per_call(hip, got, streams, what=""):
    for i, x in enumerate(streams):
        same(got[i], hip.lzss_frames([x])[0], "%s frame %d alone" % (what, i))


def content(rng, n):
    """fuzz-like: noise, byte runs, copies from earlier, short periods, a 4-symbol alphabet"""
    parts, have = [], 0
    while have < n:
        kind, ln = int(rng.integers(0, 5)), int(rng.integers(1, 300))
        if kind == 0:
            p = rng.integers(0, 256, ln, dtype=np.uint8)
        elif kind == 1:
            p = np.full(ln, [0x5E, 0x4E, 0, 0xFF][int(rng.integers(0, 4))], np.uint8)
        elif kind == 2 and have:
            src = np.concatenate(parts)
            at = int(rng.integers(0, len(src)))
            p = src[at:at + ln].copy()
        elif kind == 3:
            p = np.tile(rng.integers(0, 256, int(rng.integers(1, 16)), dtype=np.uint8), ln // 2 + 1)[:ln]
        else:
            p = rng.integers(0x4C, 0x50, ln, dtype=np.uint8)
        parts.append(p)
        have += len(p)
    return np.concatenate(parts)[:n] if parts else np.zeros(0, np.uint8)


def chained_frames(n, max_size, seed, zero=()):
    """n frames: frame f starts with the last 64 bytes of frame f - 1, frame f + 256 equals frame f (in chunk keys they
    would alias if the frame index wrapped), frames in `zero` (and their copies 256 apart) are empty"""
    rng = np.random.default_rng(seed)
    base = []
    for f in range(min(n, CHUNK_FRAMES)):
        if f in zero:
            base.append(np.zeros(0, np.uint8))
            continue
        size = int(rng.integers(1, max_size + 1))
        head = base[-1][-64:] if base else np.zeros(0, np.uint8)
        base.append(np.concatenate([head, content(rng, size)])[:size])
    return [base[f % CHUNK_FRAMES] for f in range(n)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. chunks cut by the frame count
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 512, 513])
def test_frame_count_cuts_match_brute_force(hip, n):
    """0-3 KB frames, empty frames at 254..257 and first in every chunk (0, 256, 512)"""
    streams = chained_frames(n, 3072, n, zero={0, 1, 254, 255})      # 256, 257 and 512 are copies of 0 and 1
    check_brute(gpu_batch(hip, streams, stride_extra=7, out_extra=3), streams, "n=%d" % n)


def test_frame_count_cut_within_one_window(hip):
    """513 frames of <= 200 bytes: frame f + 256 (the next chunk) equals frame f and lies within 65535 chunk positions of it;
    a frame index that wrapped in the level-3 key would find it.  Also the same frames one call each."""
    streams = chained_frames(513, 200, 5, zero={1, 254, 255})       # 257 and 511 too
    assert len(streams[0]) and len(streams[256]) and (streams[256] == streams[0]).all()
    assert sum(len(x) for x in streams[:257]) < WIN
    got = gpu_batch(hip, streams)
    check_brute(got, streams, "513 x 200")
    check_one_per_call(hip, got, streams, "513 x 200")


def test_only_empty_frames_and_no_frames(hip):
    import torch
    got = gpu_batch(hip, [np.zeros(0, np.uint8)] * 600, stride_extra=5)
    assert all(len(g) == 0 for g in got)
    bits = torch.zeros((1, 16), dtype=torch.uint8, device="cuda")
    sizes = torch.full((1,), 9, dtype=torch.int32, device="cuda")
    out = torch.full((1, 32), Z.SENTINEL, dtype=torch.uint8, device="cuda")
    cs = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hip.lzss_frames_dev(bits, sizes, 0, out=out, csize=cs)               # n_frames = 0: rc 0, nothing written
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == Z.SENTINEL).all() and int(cs.item()) == -1


# ---------------------------------------------------------------------------------------------------------------------
# 2. chunks cut by the position count, at the exact limit
# ---------------------------------------------------------------------------------------------------------------------
def runs_and_noise(n, seed):
    """long period-1/2/15 runs (groups of > 65535 members in the window) between noise (group ranks close to N)"""
    rng = np.random.default_rng(seed)
    parts, have = [], 0
    while have < n:
        ln = int(rng.integers(70_000, 400_000))
        if len(parts) % 2:
            parts.append(rng.integers(0, 256, ln, dtype=np.uint8))
        else:
            p = [1, 2, 15][len(parts) // 2 % 3]
            parts.append(np.tile(rng.integers(0, 256, p, dtype=np.uint8), ln // p + 1)[:ln])
        have += ln
    return np.concatenate(parts)[:n]


def grams(x):
    x = np.asarray(x, np.uint32)
    return x[:-2] << 16 | x[1:-1] << 8 | x[2:]


def unique_tail(f):
    """f with its last 3 bytes chosen so that the keys of its last positions, two of which read the zero padding behind the
    chunk, are new in the frame"""
    used = np.bincount(grams(f[:-3]), minlength=1 << 24)
    rng = np.random.default_rng(0)
    for _ in range(100_000):
        tail = rng.integers(0, 256, 3, dtype=np.uint8)
        new = grams(np.concatenate([f[-5:-3], tail, [0, 0]]))
        if not used[new].any() and len(set(new.tolist())) == len(new):
            return np.concatenate([f[:-3], tail])
    raise AssertionError("no tail")


def distinct_gram_pair(db):
    """two frames of 2^23 and 2^23 + 1 bytes in which no (frame, 3-gram) key occurs twice: one chunk of them has 2^24 + 1
    level-3 groups.  The smallest key (frame 0, 000) lies 20 bytes before the end of frame 0, the largest (frame 1, FFFFFF)
    10 bytes into frame 1, both followed by the byte 7: a group rank that wrapped at 2^24 would join them.  Also frame 1's
    first 2^23 bytes: one chunk of 2^24 distinct keys, ranks up to 2^24 - 1."""
    h = 1 << 23
    p0, p1 = np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8)
    p0[[1, 7]] = [7, 1]
    p1[[0, 7, 200]] = [7, 200, 0]                                  # (the padding 0 stands for 200: its grams are rare here)
    f0 = p0[np.roll(db, -(h + 20))[:h]]                            # dB index 0 (000 then 1) at frame position h - 20
    f1 = p1[np.roll(db, 13)[:h + 1]]                               # dB index 2^24 - 3 (FFFFFF then 0) at position 10
    f1, f1_0 = unique_tail(f1), unique_tail(f1[:h])
    assert (f0[h - 20:h - 16] == [0, 0, 0, 7]).all() and (f1[10:14] == [255, 255, 255, 7]).all()
    for f, nxt in ((f0, f1[:2]), (f0, f1_0[:2]), (f1, [0, 0]), (f1_0, [0, 0])):   # keys read 2 bytes into the next frame
        assert np.bincount(grams(np.concatenate([f, nxt])), minlength=1 << 24).max() == 1
    return f0, f1, f1_0


@pytest.fixture(scope="module")
def big(debruijn):
    h = 1 << 23
    a, b = runs_and_noise(h, 1), runs_and_noise(h + 1, 2)
    g0, g1, g1_0 = distinct_gram_pair(debruijn)
    return {"a": a, "b": b, "b0": b[:h], "c": runs_and_noise(CHUNK - 1, 3), "g0": g0, "g1": g1, "g1_0": g1_0,
            "one": np.array([0x4E], np.uint8), "empty": np.zeros(0, np.uint8)}


@pytest.mark.parametrize("frames", [
    ("a", "b0"),                          # one chunk of exactly 2^24 positions
    ("a", "b0", "one"),                   # 2^24 | 1
    ("a", "b0", "empty", "one"),          # an empty frame at the cut
    ("a", "b"),                           # 2^23 | 2^23 + 1
    ("c",),                               # the largest frame, 2^24 - 1 bytes
    ("g0", "g1_0"),                       # 2^24 distinct level-3 keys in one chunk: ranks up to 2^24 - 1
    ("g0", "g1"),                         # 2^24 + 1 distinct keys: must be two chunks
    ("one", "g0", "g1_0", "a"),
], ids=lambda f: "+".join(f))
def test_position_cuts_at_the_limit_match_host(hip, big, frames):
    streams = [big[f] for f in frames]
    check_host(gpu_batch(hip, streams, stride_extra=1), streams, "+".join(frames))


# ---------------------------------------------------------------------------------------------------------------------
# 3. many tiny frames in one call
# ---------------------------------------------------------------------------------------------------------------------
def test_70000_tiny_frames_match_brute_force(hip):
    """~274 chunks in one call: chunk tables and d_csize + f0 far from 0"""
    rng = np.random.default_rng(70)
    sizes = rng.integers(0, 41, 70_000)
    streams = [rng.integers(0, 4, int(s), dtype=np.uint8) + np.uint8(0x61) for s in sizes]
    got = gpu_batch(hip, streams, out_extra=2)
    check_brute(got, streams, "70000 tiny")


# ---------------------------------------------------------------------------------------------------------------------
# 4. parse pieces
# ---------------------------------------------------------------------------------------------------------------------
def cyc(db, at, n):
    """n bytes of the cyclic de Bruijn sequence from `at`: no 3-gram twice, an all-literal parse"""
    return db[np.arange(at, at + n) % len(db)]


def planted(seed, n, at, ln):
    """noise without a repeated 3-gram, with a copy of ln bytes at `at` from 300 bytes before: the greedy parse takes a match
    of exactly ln bytes at `at` (the bytes before and after the copy differ from those around its source)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, n, dtype=np.uint8)
    while Z.has_repeated_3gram(x):
        x = rng.integers(0, 256, n, dtype=np.uint8)
    src = at - 300
    x[at:at + ln] = x[src:src + ln]
    if at + ln < n:
        x[at + ln] = x[src + ln] ^ 0x55
    x[at - 1] = x[src - 1] ^ 0x33
    return x


def brute_with_match_at(x, at, ln):
    """the brute-force payload, after checking that it has a match of ln bytes at `at`"""
    toks = {p: l for p, l, _ in Z.tokens(orc(x, flushed=True), len(x))}
    assert toks.get(at) == ln, (at, ln, sorted(toks.items())[:8])
    return orc(x)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_matches_across_piece_boundaries(hip, where):
    """for every c in 1..14, matches of 3..15 bytes that start c bytes before a piece boundary: the next piece is entered at
    every carry 1..14 (and at 0 when the match ends on the boundary)"""
    n = 4 * PIECE + 100
    bound = {"first": PIECE, "middle": 2 * PIECE, "last": 4 * PIECE}[where]
    streams, exp = [], []
    for c in range(1, 15):
        for ln in range(3, 16):
            streams.append(planted(len(streams) + 1, n, bound - c, ln))
            exp.append(brute_with_match_at(streams[-1], bound - c, ln))
    for i, g in enumerate(gpu_batch(hip, streams)):
        same(g, exp[i], "%s frame %d" % (where, i))


def test_matches_ending_at_the_frame_end(hip):
    """frames of 511, 512, 513 and 1024 + k bytes (k = 1..14) whose last token is a match that ends at the frame end: for
    1024 + k the last piece is entered at offset k, i.e. at its end"""
    streams, exp = [], []
    for n in [511, 512, 513] + [1024 + k for k in range(1, 15)]:
        for ln in range(3, 16):
            streams.append(planted(n * 16 + ln, n, n - ln, ln))
            exp.append(brute_with_match_at(streams[-1], n - ln, ln))
    for i, g in enumerate(gpu_batch(hip, streams, stride_extra=3)):
        same(g, exp[i], "frame end, frame %d (%d bytes)" % (i, len(streams[i])))


def test_runs_of_pieces_entered_off_zero(hip, debruijn):
    """period-15 content behind 0..14 bytes of noise: 15-byte matches cover the piece boundaries, runs of 14 consecutive
    pieces are entered at a non-zero offset"""
    streams = []
    for ph in range(15):
        pre = debruijn[1000 * ph:1000 * ph + ph]
        x = np.concatenate([pre, np.tile(debruijn[50_000 + ph * 15:50_015 + ph * 15], 24 * PIECE // 15 + 2)])[:24 * PIECE - ph]
        starts = np.array(sorted({p for p, _, _ in Z.tokens(orc(x, flushed=True), len(x))} | set(range(ph + 15)) | {len(x)}))
        bounds = PIECE * np.arange(1, (len(x) - 1) // PIECE + 1)
        entered = starts[np.searchsorted(starts, bounds)] > bounds
        run = max(len(r) for r in "".join("x" if e else " " for e in entered).split(" "))
        assert run >= 8, (ph, entered)
        streams.append(x)
    check_brute(gpu_batch(hip, streams), streams, "period 15")
    check_brute(gpu_batch(hip, streams[::-1] * 3), streams[::-1] * 3, "period 15, reversed x3")


# ---------------------------------------------------------------------------------------------------------------------
# 5. the window of a frame deep inside a chunk
# ---------------------------------------------------------------------------------------------------------------------
def window_frames(debruijn, dist, prev_block):
    """[P, A, B]: B starts 70000 chunk positions in.  B holds a 15-byte block at 0 and again at `dist`; with prev_block A ends
    with a copy of a block that B holds at 100 (13 + 100 chunk positions away, another frame: never a match)"""
    blk = cyc(debruijn, 12_345_678, 15)
    P = cyc(debruijn, 7_000_000, 40_000)
    A = cyc(debruijn, 9_000_000, 30_000)
    B = cyc(debruijn, 3_000_000, dist + 200)
    B[:15] = blk
    B[dist:dist + 15] = blk
    B[dist + 15] = B[15] ^ 0xA5
    if prev_block:
        A[-13:] = B[100:113]
    return [P, A, B]


@pytest.mark.parametrize("dist", [WIN, WIN + 1])
@pytest.mark.parametrize("prev_block", [False, True])
def test_window_of_a_frame_deep_in_a_chunk(hip, debruijn, dist, prev_block):
    streams = window_frames(debruijn, dist, prev_block)
    B = streams[2]
    exp = H.lzss(B)[0]
    toks = {p: (l, d) for p, l, d in Z.tokens(exp, len(B))}
    if dist == WIN:
        assert toks.get(dist) == (15, WIN)                           # a match at distance 65535
    else:
        assert dist not in toks                                      # 65536: out of the window
    assert 100 not in toks
    got = gpu_batch(hip, streams)
    check_host(got, streams, "window %d" % dist)
    for two in (streams[1:], [np.concatenate(streams[:2]), B]):      # B second in its call
        check_host(gpu_batch(hip, two), two, "B second")
    same(hip.lzss_frames([B])[0], got[2], "B alone")


def test_window_tie_prefers_the_earliest_start(hip, debruijn):
    """equal 15-byte matches at distances 65535 and 65534: the earliest start (65535) wins, in a frame 70000 positions in"""
    P = cyc(debruijn, 5_000_000, 70_000)
    B = cyc(debruijn, 11_000_000, WIN + 300)
    B[:16] = 0x3C                                                    # 15 x 0x3C at 0 and at 1
    B[16] = 0x11
    B[WIN:WIN + 15] = 0x3C
    B[WIN - 1] = 0x77
    B[WIN + 15] = 0x12
    exp = H.lzss(B)[0]
    toks = {p: (l, d) for p, l, d in Z.tokens(exp, len(B))}
    assert toks.get(WIN) == (15, WIN), toks.get(WIN)
    got = gpu_batch(hip, [P, B])
    check_host(got, [P, B], "tie")


# ---------------------------------------------------------------------------------------------------------------------
# 6. frames are isolated from their neighbours
# ---------------------------------------------------------------------------------------------------------------------
def test_identical_and_overlapping_neighbours(hip):
    rng = np.random.default_rng(6)
    x = content(rng, 2500)
    streams = [x] * 8                                                # identical consecutive frames
    for k in (1, 2, 3, 14, 15, 16, 100):
        streams += [x[k:], x[:-k], x[k:], np.concatenate([x[-k:], x])]  # suffixes and prefixes of the neighbours
    streams += [x[:n] for n in range(0, 40)]
    got = gpu_batch(hip, streams)
    check_brute(got, streams, "neighbours")


def test_matches_never_run_into_the_next_frame(hip, debruijn):
    """frame f ends with the first s bytes (s = 1..14) of a block it holds earlier, frame f + 1 starts with the rest: joined,
    they would form a 15-byte match; apart, the first is capped at s bytes and the second has no source"""
    streams = []
    for s in range(1, 15):
        blk = cyc(debruijn, 123_456 + 40 * s, 15)
        a = cyc(debruijn, s * 300_007, 600)
        a[100:115] = blk
        a[-s:] = blk[:s]
        b = cyc(debruijn, s * 500_009, 600)
        b[:15 - s] = blk[s:]
        b[200:215] = blk                                             # ... and later in its own frame
        streams += [a, b]
    got = gpu_batch(hip, streams)
    check_brute(got, streams, "joins")
    check_one_per_call(hip, got, streams[:6], "joins")


# ---------------------------------------------------------------------------------------------------------------------
# 7. the row contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride_extra,out_extra", [(0, 0), (1, 1), (333, 77), (4097, 4095)])
def test_rows_at_larger_and_odd_strides(hip, stride_extra, out_extra):
    rng = np.random.default_rng(stride_extra)
    streams = [content(rng, int(n)) for n in rng.integers(0, 3000, 40)] + [np.zeros(0, np.uint8)]
    check_brute(gpu_batch(hip, streams, stride_extra, out_extra), streams, "strides %d %d" % (stride_extra, out_extra))


def test_all_literal_rows_at_max_csize(hip, debruijn):
    """all-literal frames fill a row up to agmv_hip_lzss_max_csize, less one byte, at every residue of 9n mod 8"""
    streams = [debruijn[1000 * k:1000 * k + n] for k, n in enumerate(range(1000, 1016))]
    got = gpu_batch(hip, streams)
    for x, g in zip(streams, got):
        exp, ecs = Z.literal_payload(x)
        same(g, exp, "literal %d" % len(x))
        assert ecs == hip.lzss_max_csize(len(x)) - 1 - (1 if (9 * len(x)) % 8 else 0)


# ---------------------------------------------------------------------------------------------------------------------
# 8. error returns
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["size_2p24", "size_above_stride", "out_stride_small"])
def test_error_returns_write_nothing_and_leave_the_context_usable(hip, bad):
    import torch
    n, good = 4, 500
    stride = {"size_2p24": CHUNK, "size_above_stride": 1000, "out_stride_small": 1000}[bad]
    size = {"size_2p24": CHUNK, "size_above_stride": 1001, "out_stride_small": 1000}[bad]
    ostride = hip.lzss_max_csize(size) - (1 if bad == "out_stride_small" else 0)
    bits = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
    sizes = torch.tensor([good, 0, size, good], dtype=torch.int32, device="cuda")
    out = torch.full((n, ostride), Z.SENTINEL, dtype=torch.uint8, device="cuda")
    cs = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="frame 2"):
        hip.lzss_frames_dev(bits, sizes, n, out=out, csize=cs)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == Z.SENTINEL).all(), "an output byte was written"
    assert (cs.cpu().numpy() == -1).all(), "a csize was written"
    del bits, out
    rng = np.random.default_rng(8)
    streams = [content(rng, int(k)) for k in rng.integers(0, 2000, 30)]
    check_brute(gpu_batch(hip, streams), streams, "after %s" % bad)


def test_wrapper_rejects_what_it_would_misread(hip):
    import torch
    n = 3
    bits = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), 10, dtype=torch.int32, device="cuda")
    out = torch.zeros((n, 80), dtype=torch.uint8, device="cuda")
    cs = torch.zeros(n, dtype=torch.int32, device="cuda")
    bad = {
        "sizes int64": dict(sizes=sizes.to(torch.int64)),
        "sizes on the host": dict(sizes=sizes.cpu()),
        "sizes strided": dict(sizes=torch.full((2 * n,), 10, dtype=torch.int32, device="cuda")[::2]),
        "sizes short": dict(sizes=sizes[:2]),
        "bits int32": dict(bits=torch.zeros((n, 16), dtype=torch.int32, device="cuda")),
        "bits inner stride 2": dict(bits=torch.zeros((n, 128), dtype=torch.uint8, device="cuda")[:, ::2]),
        "bits transposed": dict(bits=torch.zeros((64, n), dtype=torch.uint8, device="cuda").t()),
        "bits on the host": dict(bits=bits.cpu()),
        "bits short": dict(bits=bits[:2]),
        "out int16": dict(out=torch.zeros((n, 80), dtype=torch.int16, device="cuda")),
        "out inner stride 2": dict(out=torch.zeros((n, 160), dtype=torch.uint8, device="cuda")[:, ::2]),
        "out short": dict(out=out[:2]),
        "csize int64": dict(csize=torch.zeros(n, dtype=torch.int64, device="cuda")),
    }
    for what, kw in bad.items():
        a = dict(bits=bits, sizes=sizes, out=out, csize=cs)
        a.update(kw)
        with pytest.raises(ValueError):
            hip.lzss_frames_dev(a["bits"], a["sizes"], n, out=a["out"], csize=a["csize"])
            pytest.fail(what)
    hip.lzss_frames_dev(bits, sizes, n, out=out, csize=cs)
    torch.cuda.synchronize()
    assert (cs.cpu().numpy() == len(orc(np.zeros(10, np.uint8)))).all()


# ---------------------------------------------------------------------------------------------------------------------
# 9. the context's work areas
# ---------------------------------------------------------------------------------------------------------------------
def fresh(streams):
    from libagmv_amd import AgmvHip
    h = AgmvHip(0)
    try:
        return gpu_batch(h, streams)
    finally:
        h.close()


def test_work_areas_reused_by_smaller_and_larger_calls(big):
    from libagmv_amd import AgmvHip
    rng = np.random.default_rng(9)
    calls = [[big["a"], big["b0"]], [content(rng, 1024)], chained_frames(300, 3000, 9), [big["g0"], big["g1_0"]]]
    calls.append(calls[0])
    h = AgmvHip(0)
    try:
        for k, streams in enumerate(calls):
            got = gpu_batch(h, streams)
            exp = fresh(streams)
            for i in range(len(streams)):
                same(got[i], exp[i], "call %d frame %d" % (k, i))
    finally:
        h.close()


def test_two_contexts_on_two_streams(big):
    import torch
    from libagmv_amd import AgmvHip
    rng = np.random.default_rng(10)
    jobs = [chained_frames(300, 3000, 10), [big["a"][:3_000_000], content(rng, 5000), big["c"][:2_000_000]]]
    serial = [fresh(j) for j in jobs]
    ctx = [AgmvHip(0), AgmvHip(0)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        inputs = []
        for j in jobs:
            stride = max(len(x) for x in j)
            b = np.zeros((len(j), stride), np.uint8)
            for i, x in enumerate(j):
                b[i, :len(x)] = x
            inputs.append((torch.from_numpy(b).cuda(), torch.tensor([len(x) for x in j], dtype=torch.int32).cuda()))
        torch.cuda.synchronize()
        results = []
        for rnd in range(3):
            for w in (0, 1):
                with torch.cuda.stream(streams[w]):
                    results.append((w, ctx[w].lzss_frames_dev(inputs[w][0], inputs[w][1], len(jobs[w]))))
        torch.cuda.synchronize()
        for w, (out, cs) in results:
            out, cs = out.cpu().numpy(), cs.cpu().numpy()
            for i in range(len(jobs[w])):
                same(out[i, :cs[i]], serial[w][i], "context %d frame %d" % (w, i))
    finally:
        for c in ctx:
            c.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. the file pipeline with batches of several chunks
# ---------------------------------------------------------------------------------------------------------------------
def test_pipeline_with_multi_chunk_batches(tmp_path):
    """28 source frames of 1080p noise through AGMV_EncodeAGMV (OPT_III, LZSS) in batches of 8: NORMAL-heavy frames of > 3 MB
    pre-LZ, so every batch of 8 is more than 2^24 positions.  LZSS on the GPU (one device, and two contexts on one card)
    must write the file the host stage writes."""
    H.lib()
    T, W, Hh = 28, 1920, 1080
    rng = np.random.default_rng(10)
    (tmp_path / "fr").mkdir()
    for t in range(1, T + 1):
        H.write_bmp(str(tmp_path / "fr" / ("f%d.bmp" % t)), rng.integers(0, 1 << 24, (Hh, W), dtype=np.uint32))
    files = {}
    for name, extra in [("host", {}), ("device", {"AGMV_LZ_DEVICE": "1"}),
                        ("device2", {"AGMV_LZ_DEVICE": "1", "AGMV_DEVICES": "2", "AGMV_DEVICES_OVERSUBSCRIBE": "1"})]:
        env = dict(dict.fromkeys(("AGMV_LZ_DEVICE", "AGMV_DEVICES", "AGMV_DEVICES_OVERSUBSCRIBE")), AGMV_TRACE="1", **extra)
        d = tmp_path / name
        d.mkdir()
        (d / "fr").symlink_to(tmp_path / "fr")
        r = K.drive_child(d, "agmv", T, W, Hh, 3, 3, 1, 8, decode=True, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert (b"LZ (host)" if name == "host" else b"LZ (device)") in r.stderr, r.stderr.decode()[-2000:]
        if name == "device2":
            assert b"4 GPU workers" in r.stderr, r.stderr.decode()[-2000:]
        files[name] = open(d / "out.agmv", "rb").read()
    data = files["host"]
    usize, c = [], data.find(b"AGFC")                                 # 'AGFC', frame number, usize, csize, payload, guard bytes
    while c >= 0:
        usize.append(int.from_bytes(data[c + 8:c + 12], "little"))
        c = data.find(b"AGFC", c + 16 + int.from_bytes(data[c + 12:c + 16], "little"))
    assert len(usize) >= 16 and all(sum(usize[k:k + 8]) > CHUNK for k in range(0, len(usize) - 7, 8)), usize
    assert files["device"] == data, "AGMV_LZ_DEVICE=1 wrote another file"
    assert files["device2"] == data, "AGMV_LZ_DEVICE=1 on two contexts wrote another file"
