"""Inputs, references and closed-form expectations for the LZ77 stage on the GPU (tests/test_gpu_lz77.py,
tests/test_gpu_lz77_edges.py, tests/test_gpu_lz77_files.py, tests/test_lz77_abi.py); tests/test_lz77_cases_cpu.py pins the
stream families and their stated tokens against the brute force without a GPU."""
import ctypes as C

import numpy as np

SEG = 4096                  # LZ77_SEG of libagmv_amd/csrc/agmv_lz77_hip.hip: bytes per speculative segment
WIN = 65535
CAP = 255
SENTINEL = 0xA5


def orc77(x, tail_byte=0):
    """the brute-force payload (oracle/agmv_oracle.c orc_lz77_compress); tail_byte is what lies behind the stream"""
    import oracles as O
    x = np.ascontiguousarray(x, np.uint8)
    out = np.zeros(4 * len(x) + 64, np.uint8)
    cs = C.c_uint32()
    n = O.oracle().orc_lz77_compress(np.concatenate([x, np.full(8, tail_byte, np.uint8)]), len(x), out, C.byref(cs))
    assert n == cs.value
    return out[:cs.value].copy()


def host77(x, tail_byte=0):
    import hostlib as H
    out, cs = H.lz77(x, tail_byte)
    assert len(out) == cs
    return out


def host77_many(streams, tail_byte=0):
    """host77 of every stream, on a few threads (the library call releases the interpreter lock)"""
    from concurrent.futures import ThreadPoolExecutor
    if not streams:
        return []
    first = host77(streams[0], tail_byte)                            # loads the library once, on this thread
    with ThreadPoolExecutor(8) as pool:
        return [first] + list(pool.map(lambda x: host77(x, tail_byte), streams[1:]))


def tokens77(payload):
    """(dist, len, next) per 4-byte token"""
    p = np.asarray(payload, np.uint8).reshape(-1, 4).astype(np.int64)
    return [(int(a | b << 8), int(l), int(c)) for a, b, l, c in p]


def zeros_closed_form(n, peek=0):
    """the payload of n zero bytes: (0, 0, 0) at 0, then at i = 1 + 256k the match (min(i, 65535), min(255, n - i), next);
    next is 0 while i + len < n, the token that ends exactly at n takes the byte behind the stream"""
    if n == 0:
        return np.zeros(0, np.uint8)
    i = 1 + 256 * np.arange((max(n - 1, 0) + 255) // 256, dtype=np.int64)
    i = i[i < n]
    dist = np.minimum(i, WIN)
    ln = np.minimum(CAP, n - i)
    nxt = np.where(i + ln < n, 0, peek)
    tok = np.zeros((1 + len(i), 4), np.uint8)
    tok[1:, 0] = dist & 255
    tok[1:, 1] = dist >> 8
    tok[1:, 2] = ln
    tok[1:, 3] = nxt
    return tok.reshape(-1)


def prepare_batch_peek(rows, sizes, persist):
    """restatement of the host pipeline's loop over the reference's one persistent bitstream buffer (prepare_batch,
    libagmv_amd/csrc/agmv_pipeline.c): returns the peek bytes; persist is updated in place"""
    peek = np.zeros(len(sizes), np.uint8)
    for f, n in enumerate(sizes):
        n = int(n)
        peek[f] = persist[n] if n < len(persist) else 0
        k = min(n, len(persist))
        persist[:k] = rows[f][:k]
    return peek


def gpu_batch77(hip, streams, peek=None, stride_extra=0, out_extra=0, layout=None):
    """one batched device call; rows at a stride larger than needed.  Checks the row contract of agmv_hip_lz77_frames_dev
    (include/agmv_hip.h): csize a multiple of 4 and <= 4 * size, 0 for an empty frame, every byte of a row behind csize
    keeps what it held (SENTINEL).  Returns the payloads; a dict given as layout receives the input's row stride and
    device address."""
    import torch
    n = len(streams)
    sizes = np.array([len(x) for x in streams], np.int64)
    stride = int(max([1] + sizes.tolist())) + stride_extra
    bits = np.full((n, stride), 0xEE, np.uint8)                      # what lies behind a stream must never be read
    for i, x in enumerate(streams):
        bits[i, :len(x)] = x
    ostride = hip.lz77_max_csize(int(max([1] + sizes.tolist()))) + out_extra
    d_bits = torch.from_numpy(bits).cuda()
    if layout is not None:
        layout["stride"] = int(d_bits.stride(0))
        layout["data_ptr"] = int(d_bits.data_ptr())
    d_sizes = torch.from_numpy(sizes.astype(np.int32)).cuda()
    d_peek = torch.from_numpy(np.ascontiguousarray(peek, np.uint8)).cuda() if peek is not None else None
    out = torch.full((n, ostride), SENTINEL, dtype=torch.uint8, device="cuda")
    cs = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    out, cs = hip.lz77_frames_dev(d_bits, d_sizes, n, peek=d_peek, out=out, csize=cs)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    cs = cs.cpu().numpy().view(np.uint32).astype(np.int64)
    assert (cs % 4 == 0).all() and (cs <= 4 * sizes).all(), "csize is not 4 * tokens <= 4 * size"
    assert (cs[sizes == 0] == 0).all(), "an empty frame with a payload"
    behind = np.arange(ostride)[None, :] >= cs[:, None]
    bad = np.nonzero(behind & (out != SENTINEL))
    assert len(bad[0]) == 0, "row %d byte %d behind csize %d was written" % (bad[0][0], bad[1][0], cs[bad[0][0]])
    return [out[i, :cs[i]].copy() for i in range(n)]


def same(got, exp):
    return len(got) == len(exp) and bool((np.asarray(got) == np.asarray(exp)).all())


def bitstream_like(seed, n=None, max_n=6000):
    """runs, copies of earlier parts, short periods, 4-symbol noise and noise, as pre-LZ bitstreams mix them"""
    rng = np.random.default_rng(7700 + seed)
    if n is None:
        n = int(rng.integers(1, max_n))
    parts, have = [], 0
    while have < n:
        kind = int(rng.integers(0, 5))
        ln = int(rng.integers(1, 400))
        if kind == 0:
            p = rng.integers(0, 256, ln, dtype=np.uint8)
        elif kind == 1:
            p = np.full(ln, [0x5E, 0x4E, 0x2F, 0, 0xFF][int(rng.integers(0, 5))], np.uint8)
        elif kind == 2 and parts:
            src = np.concatenate(parts)
            at = int(rng.integers(0, len(src)))
            p = src[at:at + ln].copy()
        elif kind == 3:
            p = np.tile(rng.integers(0, 256, int(rng.integers(1, 20)), dtype=np.uint8), ln // 4 + 1)[:ln]
        else:
            p = rng.integers(0, 4, ln, dtype=np.uint8) + np.uint8(0x4C)
        parts.append(p)
        have += len(p)
    return np.concatenate(parts)[:n]


def token_starting_at(payload, i):
    """the token of a payload that starts at byte i of the stream, None if i is not a token start"""
    at = 0
    for t in tokens77(payload):
        if at == i:
            return t
        if at > i:
            return None
        at += t[1] + 1
    return None


def token_at(x, i, win=WIN, tail_byte=0):
    """one token in numpy, under a window of `win` bytes: the longest common prefix of x[j:] and x[i:], at most
    min(255, n - i) bytes, over the starts j in [max(0, i - win), i); the earliest j among the longest.  Only there to
    show that a fixture decides: the same stream under another window gives another token."""
    x = np.asarray(x, np.uint8)
    n = len(x)
    cap = min(CAP, n - i)
    j = np.arange(max(0, i - win), i)
    ln = np.zeros(len(j), np.int64)
    alive = np.ones(len(j), bool)
    for k in range(cap):
        alive &= x[j + k] == x[i + k]
        if not alive.any():
            break
        ln[alive] = k + 1
    best = int(ln.max()) if len(j) else 0
    if best == 0:
        return (0, 0, int(x[i]))
    start = int(j[np.argmax(ln == best)])
    return (i - start, best, int(x[i + best]) if i + best < n else tail_byte)


# ---- the window's low edge --------------------------------------------------------------------------------------------
# Bytes 0..199 are filler, bytes >= 200 are placed: one that is placed once cannot lie inside a match.
EDGE_BASE = 17 * SEG
EDGE_I = tuple(EDGE_BASE + d for d in (1, 2, 3, 4, 2047, 4095))
EDGE_L = (1, 2, 3, 4, 5, 40)
EDGE_OUT = (0, 1, 2, 3)
EDGE_INSIDE = ("none", "shorter", "equal")
EDGE_NEAR = 30000


def edge_grid(i_values=EDGE_I):
    """(i, L, out, inside) of the family: 68 streams per i, 408 in all"""
    return [(i, L, out, inside) for i in i_values for L in EDGE_L for out in EDGE_OUT for inside in EDGE_INSIDE
            if not (inside == "shorter" and L < 2)]


def edge_pattern(L):
    return (200 + np.arange(L) % 40).astype(np.uint8)


def edge_stream(i, L, out, inside, seed=0):
    """A token starts at i (the byte before it, 250, occurs once).  The L bytes P there, ended by 251, have a copy that
    starts `out` bytes below the window's first byte i - 65535, and inside the window, at distance 30000, nothing, P
    without its last byte, or P.  With i strictly inside a segment and past 65535, the bytes below i - 65535 lie in the
    window the GPU stages for the segment."""
    assert i - WIN - out >= 0 and L <= 40
    rng = np.random.default_rng([seed, i, L, out, EDGE_INSIDE.index(inside)])
    x = rng.integers(0, 200, i + L + 40, dtype=np.uint8)
    P = edge_pattern(L)
    x[i - 1] = 250
    x[i:i + L] = P
    x[i + L] = 251
    s = i - WIN - out
    x[s:s + L] = P
    if inside == "shorter":
        assert L >= 2
        x[i - EDGE_NEAR:i - EDGE_NEAR + L - 1] = P[:L - 1]
        x[i - EDGE_NEAR + L - 1] = 252
    elif inside == "equal":
        x[i - EDGE_NEAR:i - EDGE_NEAR + L] = P
    else:
        assert inside == "none"
    return x


def edge_token(i, L, out, inside):
    """the token at i of edge_stream(i, L, out, inside)"""
    if out == 0:
        return (WIN, L, 251)
    if inside == "none":
        return (0, 0, 200)
    if inside == "shorter":
        return (EDGE_NEAR, L - 1, int(edge_pattern(L)[L - 1]))
    return (EDGE_NEAR, L, 251)


# ---- the look-ahead edge ----------------------------------------------------------------------------------------------
AHEAD_E = (2 * SEG, 17 * SEG, 18 * SEG)
AHEAD_K = (0, 1, 2, 3, 254, 255)
AHEAD_TAIL = (0, 1, 2, 300)
AHEAD_DIST = 5000


def ahead_grid():
    return [(E, k, tail) for E in AHEAD_E for k in AHEAD_K for tail in AHEAD_TAIL]


def ahead_stream(E, k, tail, seed=0):
    """a 255-byte match at distance 5000 whose token starts at i = E - 1 - k, E a segment boundary: for k = 0 its `next`
    is the last byte the segment's workgroup stages, for k = 254 it ends at E - 1 and `next` is E, for k = 255 the token
    leaves the segment exactly at E.  tail bytes follow the match (251 first); with tail = 0 the match ends at the stream's
    size and `next` is the byte behind the stream."""
    i = E - 1 - k
    rng = np.random.default_rng([seed, E, k, tail])
    x = rng.integers(0, 200, i + CAP + tail, dtype=np.uint8)
    B = rng.integers(200, 250, CAP, dtype=np.uint8)
    x[i - AHEAD_DIST:i - AHEAD_DIST + CAP] = B
    x[i:i + CAP] = B
    x[i - 1] = 250
    if tail > 0:
        x[i + CAP] = 251
    return x


def ahead_token(E, k, tail, peek=0):
    return (AHEAD_DIST, CAP, 251 if tail > 0 else peek)


# ---- the stitch's exits -----------------------------------------------------------------------------------------------
SHIFT_M = (1, 2, 64)


def shifted_stream(k, m, seed=0):
    """k distinct bytes, then three times SEG - m zeros and m bytes of noise without a zero: the pattern lies at every
    offset against the segments.  (The noise cuts the token that runs into it, so the chain through the zeros and the
    speculative parse of a segment meet again behind it: these streams seldom make the stitch parse anything again.
    exit_stream does.)"""
    rng = np.random.default_rng([seed, k, m])
    parts = [np.arange(1, k + 1, dtype=np.uint8)]
    for _ in range(3):
        parts += [np.zeros(SEG - m, np.uint8), rng.integers(1, 256, m, dtype=np.uint8)]
    return np.concatenate(parts)


def exit_stream(k, m, seed=0):
    """k distinct bytes, then zeros up to 3 * SEG bytes, with m bytes of noise without a zero at the end of the second
    segment.  The chain through the zeros (k, k + 1 + 256 j) enters the second segment at 4097 + k, which for k < 255 is
    no start of its speculative parse (4096 + 256 j): the stitch parses it again.  The noise cuts the last token of both
    parses, whose `next` is the first noise byte at 2 * SEG - m: for m = 1 the re-parse leaves its segment exactly at its end
    E without having met a recorded start, for m = 2 it meets one at E - 1, for larger m at E - m + 1."""
    rng = np.random.default_rng([seed, k, m, 1])
    x = np.zeros(3 * SEG, np.uint8)
    x[:k] = np.arange(1, k + 1)
    x[2 * SEG - m:2 * SEG] = rng.integers(1, 256, m, dtype=np.uint8)
    return x


def stitch_model(x, g):
    """what k_lz77_stitch does in segment g of stream x, from the definitions alone: (entry, where the parse from the entry
    ends, merged).  The true token starts come from the host stage, the speculative ones from token_at."""
    S, E = g * SEG, min((g + 1) * SEG, len(x))
    true, at = [], 0
    for t in tokens77(host77(x)):
        true.append(at)
        at += t[1] + 1
    spec, i = set(), S
    while i < E:
        spec.add(i)
        i += token_at(x, i)[1] + 1
    entry = min(t for t in true if t >= S)
    for t in true + [at]:
        if t >= entry and (t in spec or t >= E):
            return entry, t, t in spec and t < E
    raise AssertionError("the chain does not leave the segment")


# ---- deep windows -----------------------------------------------------------------------------------------------------
DEEP_SEEDS = 8


def deep_stream(seed):
    """bitstream_like of 70 000 .. 300 000 bytes, the size drawn from the seed"""
    n = int(np.random.default_rng(4100 + seed).integers(70_000, 300_001))
    return bitstream_like(300 + seed, n=n)


def window_limit_stream():
    """a 64-byte block, 70 000 bytes of noise, the block again: out of the window"""
    rng = np.random.default_rng(5)
    block = rng.integers(0, 256, 64, dtype=np.uint8)
    return np.concatenate([block, rng.integers(0, 256, 70000, dtype=np.uint8), block])


def stride_extra_for(streams, residue):
    """stride_extra of gpu_batch77 that makes the row stride = residue (mod 4)"""
    longest = max([1] + [len(x) for x in streams])
    return (residue - longest) % 4


def at_every_alignment(streams):
    """each stream in four consecutive rows: at a row stride = 1 (mod 4) from an aligned base, the four copies start at
    the four byte offsets of a dword"""
    return [x for x in streams for _ in range(4)]
