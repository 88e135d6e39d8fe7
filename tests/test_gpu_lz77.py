"""The LZ77 stage on the GPU (agmv_hip_lz77_peek_dev / agmv_hip_lz77_frames_dev and their AgmvHip mirrors) against the
brute-force restatement (orc_lz77_compress), the host stage (agmv_lz77_mem) and the closed form of an all-zero stream.
Payloads are the csize = 4 * tokens bytes the reference's file holds for a frame."""
import os

import numpy as np
import pytest

import lz77_cases as Z
from lz77_cases import SEG, bitstream_like, gpu_batch77, host77, orc77, same, token_starting_at, tokens77, zeros_closed_form

pytestmark = pytest.mark.gpu

SEEDS = int(os.environ.get("AGMV_FUZZ_SEEDS", "24"))


@pytest.fixture(scope="module")
def hip():
    import torch
    from libagmv_amd import AgmvHip
    assert torch.cuda.is_available()
    h = AgmvHip(0)
    yield h
    h.close()


def small_cases():
    rng = np.random.default_rng(77)
    cases = []
    for n in (0, 1, 2, 3, 254, 255, 256, 257, 258):
        cases.append(rng.integers(0, 3, n, dtype=np.uint8))
        cases.append(np.zeros(n, np.uint8))
        cases.append(rng.integers(0, 256, n, dtype=np.uint8))
    for p in range(1, 17):                                           # self-overlapping runs of period 1..16
        cases.append(np.tile(rng.integers(0, 256, p, dtype=np.uint8), 2000 // p + 1)[:2000 + p])
    # a 1-byte match whose byte occurs at three places: the earliest one wins (distance 9 at position 9)
    cases.append(np.array([7, 1, 2, 7, 3, 4, 7, 5, 6, 7, 8], np.uint8))
    # equally long (5) matches at two distances for the copy at 80; a later longer match (7) beats an earlier shorter one
    blk = rng.integers(0, 100, 5, dtype=np.uint8)
    t = np.arange(100, 220, dtype=np.uint8)
    t[0:5] = blk; t[40:45] = blk; t[80:85] = blk
    cases.append(t.copy())
    t[60:67] = np.concatenate([blk, [7, 9]]); t[100:107] = np.concatenate([blk, [7, 9]])
    cases.append(t)
    # a 300-byte repeat: the cap of 255, then the next token
    r = rng.integers(0, 256, 300, dtype=np.uint8)
    cases.append(np.concatenate([r, [1, 2, 3], r, [4]]).astype(np.uint8))
    return cases


def test_hand_made_tokens(hip):
    """the tie rules, spelled out as tokens"""
    got = tokens77(hip.lz77_frames([np.array([7, 1, 2, 7, 3, 4, 7, 5, 6, 7, 8], np.uint8)])[0])
    assert got[-1] == (9, 1, 8) and got[3] == (3, 1, 3)
    rng = np.random.default_rng(1)
    r = rng.integers(0, 256, 300, dtype=np.uint8)
    x = np.concatenate([r, [1, 2, 3], r, [4]]).astype(np.uint8)
    got = hip.lz77_frames([x])[0]
    assert same(got, orc77(x))
    tk = tokens77(got)
    assert (303, 255, int(r[255])) in tk and tk[-1] == (303, 44, 4)


@pytest.mark.parametrize("case", range(len(small_cases())))
def test_small_cases_match_brute_force(hip, case):
    x = small_cases()[case]
    assert same(hip.lz77_frames([x])[0], orc77(x))


@pytest.mark.parametrize("seed", range(SEEDS))
def test_fuzz_matches_brute_force(hip, seed):
    x = bitstream_like(seed)
    assert same(hip.lz77_frames([x])[0], orc77(x)), seed


def ends_with_match(x):
    tk = tokens77(orc77(x))
    return tk[-1][1] > 0 and sum(t[1] + 1 for t in tk) == len(x) + 1


@pytest.mark.parametrize("peek", [0, 0x5A])
def test_byte_past_the_end(hip, peek):
    rng = np.random.default_rng(3)
    r = rng.integers(0, 256, 40, dtype=np.uint8)
    match_end = [np.concatenate([r, r]), np.zeros(600, np.uint8), np.concatenate([r, [9], r[:7]]).astype(np.uint8),
                 np.array([5, 5], np.uint8)]
    literal_end = [np.concatenate([r, r, [r[0] ^ 0xFF]]).astype(np.uint8), np.arange(50, dtype=np.uint8), np.array([5], np.uint8)]
    for x in match_end:
        assert ends_with_match(x)
    for x in literal_end:
        assert not ends_with_match(x)
    streams = match_end + literal_end
    got = gpu_batch77(hip, streams, peek=np.full(len(streams), peek, np.uint8))
    for i, x in enumerate(streams):
        assert same(got[i], orc77(x, peek)), i
        assert same(got[i], host77(x, peek)), i
    for i in range(len(match_end)):
        assert got[i][-1] == peek
    plain = gpu_batch77(hip, streams)                                # no peek array: zeros
    for i, x in enumerate(streams):
        assert same(plain[i], orc77(x, 0)), i
    for i in range(len(match_end), len(streams)):
        assert same(plain[i], got[i])                                # a literal at the end does not see the peek byte


@pytest.mark.parametrize("dist", [65535, 65536])
def test_window_edge_repeat(hip, dist):
    """a 40-byte repeat at distance 65535 is a match; at 65536 its first byte is out of the window"""
    rng = np.random.default_rng(dist)
    blk = rng.integers(0, 200, 40, dtype=np.uint8)
    x = np.concatenate([blk, rng.integers(0, 200, dist - 40, dtype=np.uint8), blk, [251, 252, 253]]).astype(np.uint8)
    x[dist - 1] = 250                                                # occurs nowhere before: the next byte starts a token
    got = hip.lz77_frames([x])[0]
    assert same(got, host77(x))
    hit = token_starting_at(got, dist)
    assert hit is not None, "position %d is not a token start" % dist
    if dist == 65535:
        assert hit == (65535, 40, 251)
    else:
        assert hit[1] < 40


@pytest.mark.parametrize("dist", [65535, 65536])
def test_window_edge_single_byte(hip, dist):
    """a byte whose only other occurrence lies at distance 65535 is a 1-byte match; at 65536 the token is (0, 0, byte)"""
    rng = np.random.default_rng(dist + 1)
    x = rng.integers(0, 200, dist + 3, dtype=np.uint8)
    x[dist - 1] = 250                                                # a token boundary: 250 occurs nowhere before
    x[0] = 222; x[dist] = 222; x[dist + 1] = 251; x[dist + 2] = 252
    x[1:dist][x[1:dist] == 222] = 0
    got = hip.lz77_frames([x])[0]
    assert same(got, host77(x))
    hit = token_starting_at(got, dist)
    assert hit is not None, "position %d is not a token start" % dist
    assert hit == ((65535, 1, 251) if dist == 65535 else (0, 0, 222))


def test_every_entry_offset_into_a_segment(hip):
    """k distinct bytes, then zeros: the true chain enters the segments of zeros at every offset"""
    streams = [np.concatenate([np.arange(1, k + 1, dtype=np.uint8), np.zeros(3 * SEG + 77, np.uint8)]) for k in range(256)]
    got = gpu_batch77(hip, streams)
    assert hip.lz77_reparsed_segments() > 0
    for k, x in enumerate(streams):
        assert same(got[k], host77(x)), k


def test_closed_form_of_zeros_is_the_host_stage():
    for n, peek in ((0, 0), (1, 9), (2, 9), (256, 9), (257, 9), (258, 9), (70000, 0x5A), (66049, 3)):
        assert same(zeros_closed_form(n, peek), host77(np.zeros(n, np.uint8), peek)), n


def test_all_zero_frame_never_merges(hip):
    n = 300_000
    got = gpu_batch77(hip, [np.zeros(n, np.uint8)], peek=np.array([0x5A], np.uint8))[0]
    assert hip.lz77_reparsed_segments() > 0
    assert same(got, zeros_closed_form(n, 0x5A))


@pytest.mark.parametrize("period", [2, 255, 256, 257])
def test_periodic_frames(hip, period):
    rng = np.random.default_rng(period)
    n = 300_000 + period
    x = np.tile(rng.permutation(256)[np.arange(period) % 256].astype(np.uint8), n // period + 1)[:n]
    assert same(hip.lz77_frames([x])[0], host77(x))


def test_sizes_around_the_segment_size(hip):
    streams = []
    for m in (1, 2, 17):
        for d in (-1, 0, 1):
            streams.append(bitstream_like(100 + len(streams), n=m * SEG + d))
            streams.append(np.zeros(m * SEG + d, np.uint8))
    got = gpu_batch77(hip, streams, peek=np.full(len(streams), 0x33, np.uint8), stride_extra=5)
    for i, x in enumerate(streams):
        assert same(got[i], host77(x, 0x33)), i


def test_one_batched_call_mixed_sizes(hip):
    streams = small_cases() + [bitstream_like(s) for s in range(SEEDS)]
    streams.insert(3, np.zeros(0, np.uint8))
    streams.append(np.zeros(0, np.uint8))
    got = gpu_batch77(hip, streams, stride_extra=333, out_extra=77)
    for i, x in enumerate(streams):
        assert same(got[i], orc77(x)), i


def test_many_tiny_frames(hip):
    rng = np.random.default_rng(8)
    n = 70_000
    sizes = rng.integers(0, 9, n)
    streams = [rng.integers(0, 3, int(s), dtype=np.uint8) for s in sizes]
    peek = rng.integers(0, 256, n, dtype=np.uint8)
    got = gpu_batch77(hip, streams, peek=peek)
    for i in range(n):
        assert same(got[i], host77(streams[i], int(peek[i]))), i


def test_largest_frame_and_the_error_beyond(hip):
    import torch
    n = (1 << 24) - 1
    bits = torch.zeros((1, 1 << 24), dtype=torch.uint8, device="cuda")
    sizes = torch.tensor([n], dtype=torch.int32, device="cuda")
    peek = torch.tensor([0x5A], dtype=torch.uint8, device="cuda")
    out, cs = hip.lz77_frames_dev(bits, sizes, 1, peek=peek)
    torch.cuda.synchronize()
    exp = zeros_closed_form(n, 0x5A)
    assert int(cs[0]) == len(exp)
    assert (out[0, :len(exp)].cpu().numpy() == exp).all()
    assert hip.lz77_reparsed_segments() > 0
    sizes[0] = 1 << 24
    with pytest.raises(RuntimeError, match="at most 16777215 bytes"):
        hip.lz77_frames_dev(bits, sizes, 1, peek=peek, out=out, csize=cs)
    # the work areas stay usable: a small call after the large one
    x = bitstream_like(5)
    assert same(hip.lz77_frames([x])[0], orc77(x))
    assert same(gpu_batch77(hip, [x, np.zeros(10, np.uint8)])[0], orc77(x))


def peek_dev(hip, rows, sizes, persist, stride):
    import torch
    n = len(sizes)
    bits = np.zeros((max(n, 1), stride), np.uint8)
    for f in range(n):
        bits[f, :len(rows[f])] = rows[f]
    d_persist = torch.from_numpy(persist.copy()).cuda()
    peek = hip.lz77_peek_dev(torch.from_numpy(bits).cuda(), torch.from_numpy(np.asarray(sizes, np.int32)).cuda(), n, d_persist)
    torch.cuda.synchronize()
    return peek.cpu().numpy()[:n], d_persist.cpu().numpy()


@pytest.mark.parametrize("shape", ["random", "equal", "long", "many"])
def test_peek_against_the_host_loop(hip, shape):
    rng = np.random.default_rng(len(shape))
    plen = 300
    if shape == "random":
        sizes = rng.integers(0, 280, 40); sizes[[3, 17]] = 0
    elif shape == "equal":
        sizes = np.full(12, 123)
    elif shape == "long":
        sizes = rng.integers(250, 400, 30); sizes[5] = 300; sizes[6] = 299
    else:
        sizes = rng.integers(0, 299, 5000)
    stride = int(max(sizes)) + 3
    rows = [rng.integers(1, 256, stride, dtype=np.uint8) for _ in sizes]          # bytes behind a size are there, as k_encode leaves them
    persist0 = rng.integers(1, 256, plen, dtype=np.uint8)
    exp_persist = persist0.copy()
    exp = Z.prepare_batch_peek(rows, sizes, exp_persist)
    got, got_persist = peek_dev(hip, rows, sizes, persist0, stride)
    assert (got == exp).all() and (got_persist == exp_persist).all()
    # the same frames in two calls with the buffer carried
    cut = len(sizes) // 3
    a, mid = peek_dev(hip, rows[:cut], sizes[:cut], persist0, stride)
    b, end = peek_dev(hip, rows[cut:], sizes[cut:], mid, stride)
    assert (np.concatenate([a, b]) == exp).all() and (end == exp_persist).all()


def test_real_1080p_frames_peek_compress_decode(hip):
    """8 frames of the synthetic 1080p clip through k_encode, then peek + LZ77 on the device against the host stage with the
    emulated peek bytes, and back through the GPU decoder"""
    import torch
    from test_gpu_lzss import encode_bitstreams
    W, H_, n = 1920, 1080, 8
    frames = hip.synth_dev(W, H_, 0, n)
    out, sizes = encode_bitstreams(hip, frames, n, W, H_)
    torch.cuda.synchronize()
    bits = out.cpu().numpy()
    sz = sizes.cpu().numpy().view(np.uint32)
    persist = torch.zeros(out.stride(0) + 64, dtype=torch.uint8, device="cuda")
    peek = hip.lz77_peek_dev(out, sizes, n, persist)
    pay, cs = hip.lz77_frames_dev(out, sizes, n, peek=peek)
    torch.cuda.synchronize()
    reparsed = hip.lz77_reparsed_segments()
    exp_persist = np.zeros(out.stride(0) + 64, np.uint8)
    exp_peek = Z.prepare_batch_peek([bits[f] for f in range(n)], sz, exp_persist)
    assert (peek.cpu().numpy()[:n] == exp_peek).all()
    assert (persist.cpu().numpy() == exp_persist).all()
    pay_h = pay.cpu().numpy()
    cs_h = cs.cpu().numpy().view(np.uint32)
    payloads = []
    for f in range(n):
        exp = host77(bits[f, :sz[f]], int(exp_peek[f]))
        assert cs_h[f] == len(exp), f
        assert (pay_h[f, :len(exp)] == exp).all(), f
        payloads.append(np.concatenate([exp, np.full(4, 0xFF, np.uint8)]))
    print("1080p: %d of %d segments re-parsed" % (reparsed, sum((int(s) + SEG - 1) // SEG for s in sz)))
    cap = int(out.stride(0)) + 64
    rows, bpos, used, _ = hip.lz_decode_frames(3, payloads, [int(s) for s in sz], [int(c) for c in cs_h], cap)
    for f in range(n):
        assert bpos[f] >= sz[f], f                                   # (the token at the end also writes its `next`)
        assert (rows[f, :sz[f]] == bits[f, :sz[f]]).all(), f
