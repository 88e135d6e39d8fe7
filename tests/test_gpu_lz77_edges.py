"""The LZ77 stage on the GPU (agmv_hip_lz77_frames_dev) at the edges its kernels and host driver are built around
(libagmv_amd/csrc/agmv_lz77_hip.hip, DESIGN.md section 4 "LZ77 stage"): the window's first byte strictly inside a segment, where
bytes below it lie in LDS and only the two range tests of lz77_search keep them out (pass A for matches of 4 bytes and more,
pass B for 1..3); windows past 65 535 bytes staged at all four byte offsets of a dword; 255-byte matches whose last byte or
`next` is the last byte a segment stages, or the stream's last, or the byte behind it; the ways a re-parse leaves or rejoins
its segment; and batches cut into chunks by the 2^26 positions a chunk holds, whose later chunks reuse the work areas.

References: the host stage (agmv_lz77_mem), which tests/test_lz77_cases_cpu.py pins against the brute force on these very
families, and the tokens the families state in closed form.  Every check compares csize and every payload byte, and batches
go through gpu_batch77, which checks the row contract of include/agmv_hip.h; the chunk test compares on the device."""
import numpy as np
import pytest

import lz77_cases as Z
from lz77_cases import SENTINEL, bitstream_like, gpu_batch77, host77, host77_many, orc77, same, token_starting_at

pytestmark = pytest.mark.gpu

CHUNK = 1 << 26                 # LZ77_CHUNK: positions per chunk


@pytest.fixture(scope="module")
def hip():
    import torch
    from libagmv_amd import AgmvHip
    assert torch.cuda.is_available()
    h = AgmvHip(0)
    yield h
    h.close()


def batch_at_every_alignment(hip, streams, peek=None):
    """each stream in four consecutive rows of one call, the rows a stride = 1 (mod 4) apart from an aligned base: copy r of a
    stream starts at byte offset r of a dword (in rotating order), so a window that starts at W0 = 1 (mod 4) is staged
    with every offset a = (r + 1) & 3.  Returns the payloads, four per stream."""
    rows = Z.at_every_alignment(streams)
    layout = {}
    got = gpu_batch77(hip, rows, peek=None if peek is None else np.full(len(rows), peek, np.uint8),
                      stride_extra=Z.stride_extra_for(streams, 1), layout=layout)
    assert layout["stride"] % 4 == 1 and layout["data_ptr"] % 4 == 0
    assert sorted((layout["data_ptr"] + r * layout["stride"]) % 4 for r in range(4)) == [0, 1, 2, 3]
    return got


@pytest.mark.parametrize("i", Z.EDGE_I)
def test_window_low_edge(hip, i):
    """68 streams per token start i = 17 * SEG + 1, 2, 3, 4, 2047, 4095: a copy of the L bytes at i starts 0..3 bytes below
    the window's first byte c0 (so c0 & 3 takes every value), with and without a shorter or an equal copy inside"""
    grid = Z.edge_grid([i])
    assert len(grid) == 68
    streams = [Z.edge_stream(*c) for c in grid]
    got = batch_at_every_alignment(hip, streams)
    exp = host77_many(streams)
    for s, c in enumerate(grid):
        for r in range(4):
            assert same(got[4 * s + r], exp[s]), (c, r)
            assert token_starting_at(got[4 * s + r], i) == Z.edge_token(*c), (c, r)


def test_lookahead_edge(hip):
    grid = Z.ahead_grid()
    assert len(grid) == 72
    streams = [Z.ahead_stream(*c) for c in grid]
    got = batch_at_every_alignment(hip, streams, peek=0x5A)
    exp = host77_many(streams, 0x5A)
    for s, (E, k, tail) in enumerate(grid):
        for r in range(4):
            assert same(got[4 * s + r], exp[s]), (E, k, tail, r)
            assert token_starting_at(got[4 * s + r], E - 1 - k) == Z.ahead_token(E, k, tail, 0x5A), (E, k, tail, r)


@pytest.mark.parametrize("m", Z.SHIFT_M)
def test_stitch_exits(hip, m):
    """one call per m: the shifted family, and the family whose second segment is parsed again from 4097 + k and left
    exactly at its end (m = 1) or rejoined at E - 1 (m = 2) or E - 63 (m = 64), as tests/test_lz77_cases_cpu.py shows"""
    streams = [Z.shifted_stream(k, m) for k in range(256)] + [Z.exit_stream(k, m) for k in range(256)]
    got = gpu_batch77(hip, streams)
    assert hip.lz77_reparsed_segments() >= 255                       # the second segment of every exit_stream with k < 255
    exp = host77_many(streams)
    for k in range(len(streams)):
        assert same(got[k], exp[k]), (k, m)


def test_deep_fuzz_at_every_alignment(hip):
    streams = [Z.deep_stream(s) for s in range(Z.DEEP_SEEDS)]
    got = batch_at_every_alignment(hip, streams, peek=0x33)
    exp = host77_many(streams, 0x33)
    for s in range(len(streams)):
        for r in range(4):
            assert same(got[4 * s + r], exp[s]), (s, r)
    # and back through the GPU decoder (the token at the end also writes its `next`)
    usizes = [len(x) for x in Z.at_every_alignment(streams)]
    payloads = [np.concatenate([p, np.full(4, 0xFF, np.uint8)]) for p in got]
    rows, bpos, used, _ = hip.lz_decode_frames(3, payloads, usizes, [len(p) for p in got], max(usizes) + 64)
    for f, x in enumerate(Z.at_every_alignment(streams)):
        assert bpos[f] >= len(x), f
        assert (rows[f, :len(x)] == x).all(), f


@pytest.fixture(scope="module")
def chunk_frames():
    """the distinct frames of the chunk batches with their expected payloads (peek 0x5A), computed once"""
    frames = {"A": bitstream_like(201, n=1 << 20), "B": bitstream_like(202, n=(1 << 20) - 1),
              "C": np.array([0x4E], np.uint8), "Z": np.zeros(0, np.uint8)}
    return {name: (x, host77(x, 0x5A)) for name, x in frames.items()}


CHUNK_BATCHES = {
    "a": ["A"] * 64 + ["C"],                                         # the first chunk is exactly full, C opens the second
    "b": ["A"] * 63 + ["B", "C", "C"],                               # the first C still fits (<=), the second opens chunk 2
    "c": ["A"] * 64 + ["Z", "B", "Z"] + ["A"] * 64 + ["C"],          # three chunks; an empty frame joins one that is full
}


def expected_chunks(sizes):
    """frames per chunk, as the driver cuts them: the next frame joins while the positions stay <= 2^26"""
    chunks, n = [0], 0
    for s in sizes:
        if n + s > CHUNK:
            chunks.append(0)
            n = 0
        n += s
        chunks[-1] += 1
    return chunks


@pytest.mark.parametrize("batch", sorted(CHUNK_BATCHES))
def test_chunks_cut_by_positions(hip, chunk_frames, batch):
    import torch
    names = CHUNK_BATCHES[batch]
    n = len(names)
    sizes = [len(chunk_frames[name][0]) for name in names]
    assert expected_chunks(sizes) == {"a": [64, 1], "b": [65, 1], "c": [65, 65, 2]}[batch]
    assert sum(sizes) == {"a": CHUNK + 1, "b": CHUNK + 1, "c": 2 * CHUNK + (1 << 20)}[batch]
    stride = (1 << 20) + 1
    ostride = hip.lz77_max_csize(1 << 20)
    bits = torch.full((n, stride), 0xEE, dtype=torch.uint8, device="cuda")
    expected = {}
    for name in set(names):
        x, exp = chunk_frames[name]
        rows = torch.tensor([f for f in range(n) if names[f] == name], device="cuda")
        if len(x):
            bits[rows, :len(x)] = torch.from_numpy(x).cuda()
        expected[name] = torch.from_numpy(exp).cuda()
    d_sizes = torch.tensor(sizes, dtype=torch.int32, device="cuda")
    peek = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((n, ostride), SENTINEL, dtype=torch.uint8, device="cuda")
    cs = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    hip.lz77_frames_dev(bits, d_sizes, n, peek=peek, out=out, csize=cs)
    torch.cuda.synchronize()
    cs = cs.cpu().numpy()
    for f, name in enumerate(names):
        exp = expected[name]
        assert cs[f] == exp.numel(), "frame %d (%s): csize %d, expected %d" % (f, name, cs[f], exp.numel())
        assert torch.equal(out[f, :exp.numel()], exp), "frame %d (%s): payload" % (f, name)
        assert bool((out[f, exp.numel():] == SENTINEL).all()), "frame %d (%s): a byte behind csize was written" % (f, name)
    # the work areas stay usable after growing: a small call on the same context
    x = bitstream_like(5)
    assert same(hip.lz77_frames([x])[0], orc77(x))


def test_chunk_opens_with_an_empty_frame(hip):
    """an empty frame always fits into a chunk by positions, so only the cut at LZ77_CHUNK_FRAMES = 65 536 frames puts one
    first: 65 536 one-byte frames, an empty one, a one-byte one"""
    rng = np.random.default_rng(9)
    streams = [rng.integers(0, 256, 1, dtype=np.uint8) for _ in range(1 << 16)] + [np.zeros(0, np.uint8), np.array([7], np.uint8)]
    got = gpu_batch77(hip, streams, peek=np.full(len(streams), 0x5A, np.uint8))
    for f, x in enumerate(streams):
        assert same(got[f], np.array([0, 0, 0, x[0]], np.uint8) if len(x) else np.zeros(0, np.uint8)), f
