"""Inputs, references and closed-form expectations for the LZSS stage (tests/test_lz_csize_tail.py, tests/test_gpu_lzss.py,
tests/test_gpu_lzss_edges.py)."""
import ctypes as C

import numpy as np

TAIL_N = 1864143            # 9n = 16 777 287 bits: above 2^24, n = 7 (mod 8)


def all_literal_stream(n=TAIL_N, seed=3):
    """n bytes in which no 3-gram occurs twice (every LZSS token is a literal): a greedy walk over unused 3-grams"""
    rng = np.random.default_rng(seed)
    used = np.zeros(1 << 24, np.bool_)
    out = bytearray(n)
    starts = rng.integers(0, 256, n).tolist()
    a, b = 0, 1
    out[0], out[1] = a, b
    for i in range(2, n):
        base = (a << 16) | (b << 8)
        c0 = starts[i]
        for k in range(256):
            c = (c0 + k) & 255
            if not used[base | c]:
                break
        else:
            raise AssertionError("greedy walk stuck at %d" % i)
        used[base | c] = True
        out[i] = c
        a, b = b, c
    return np.frombuffer(bytes(out), np.uint8).copy()


def literal_payload(x):
    """the reference's payload for an all-literal stream: 9-bit tokens 1 | byte << 1, LSB-first, csize computed in float;
    when csize exceeds the full bytes the last payload byte is the partial one (unused high bits 0)"""
    x = np.asarray(x, np.uint8)
    n = len(x)
    tok = np.zeros((n, 16), np.uint8)
    tok[:, 0] = 1
    tok[:, 1:9] = np.unpackbits(x[:, None], axis=1, bitorder="little")
    bits = tok[:, :9].reshape(-1)
    flushed = np.packbits(bits, bitorder="little")                  # ceil(9n / 8) bytes, partial byte zero-padded
    csize = int(np.float32(9 * n) / np.float32(8))
    return flushed[:csize].copy(), csize


def has_repeated_3gram(x):
    x = np.asarray(x, np.uint32)
    g = (x[:-2] << 16) | (x[1:-1] << 8) | x[2:]
    return len(np.unique(g)) != len(g)


def orc(x, flushed=False):
    """the brute-force payload: csize bytes of the flushed stream, zero-padded (flushed: the whole flushed stream, whose
    last token the csize bytes can cut)"""
    import oracles as O
    x = np.ascontiguousarray(x, np.uint8)
    out = np.zeros(4 * len(x) + 64, np.uint8)
    cs = C.c_uint32()
    n = O.oracle().orc_lzss_compress(np.concatenate([x, np.zeros(8, np.uint8)]), len(x), out, C.byref(cs))
    if flushed:
        return out[:n].copy()
    p = np.zeros(cs.value, np.uint8)
    p[:min(n, cs.value)] = out[:min(n, cs.value)]
    return p


SENTINEL = 0xA5


def gpu_batch(hip, streams, stride_extra=0, out_extra=0):
    """one batched device call; rows at a stride larger than needed.  Checks the row contract of agmv_hip_lzss_frames_dev
    (include/agmv_hip.h): csize <= agmv_hip_lzss_max_csize(size), 0 for an empty frame, and every byte of a row behind
    csize keeps what it held (SENTINEL).  Returns the payloads."""
    import torch
    n = len(streams)
    sizes = np.array([len(x) for x in streams], np.int64)
    stride = int(max([1] + sizes.tolist())) + stride_extra
    bits = np.zeros((n, stride), np.uint8)
    for i, x in enumerate(streams):
        bits[i, :len(x)] = x
    ostride = hip.lzss_max_csize(stride) + out_extra
    d_bits = torch.from_numpy(bits).cuda()
    d_sizes = torch.from_numpy(sizes.astype(np.int32)).cuda()
    out = torch.full((n, ostride), SENTINEL, dtype=torch.uint8, device="cuda")
    cs = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    out, cs = hip.lzss_frames_dev(d_bits, d_sizes, n, out=out, csize=cs)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    cs = cs.cpu().numpy().view(np.uint32).astype(np.int64)
    cap = np.array([hip.lzss_max_csize(s) for s in np.unique(sizes)], np.int64)
    assert (cs <= cap[np.searchsorted(np.unique(sizes), sizes)]).all(), "csize above agmv_hip_lzss_max_csize"
    assert (cs[sizes == 0] == 0).all(), "an empty frame with a payload"
    behind = np.arange(ostride)[None, :] >= cs[:, None]
    bad = np.nonzero(behind & (out != SENTINEL))
    assert len(bad[0]) == 0, "row %d byte %d behind csize %d was written" % (bad[0][0], bad[1][0], cs[bad[0][0]])
    return [out[i, :cs[i]].copy() for i in range(n)]


def de_bruijn3():
    """the cyclic de Bruijn sequence B(256, 3) (2^24 bytes, every 3-gram once cyclically): the Lyndon words of length 1 and 3
    in lexicographic order.  A slice of it holds no 3-gram twice, so its LZSS parse is all literals."""
    parts = []
    for a in range(256):
        b, c = np.meshgrid(np.arange(a, 256), np.arange(a + 1, 256), indexing="ij")
        w = np.stack([np.full(b.size, a), b.reshape(-1), c.reshape(-1)], axis=1).reshape(-1)
        parts.append(np.concatenate([[a], w]).astype(np.uint8))
    s = np.concatenate(parts)
    assert len(s) == 1 << 24
    return s


def tokens(payload, n):
    """(position, length, distance) of the match tokens in a flushed LZSS stream of an n-byte input (literals are skipped)"""
    bits = np.unpackbits(np.concatenate([np.asarray(payload, np.uint8), np.zeros(4, np.uint8)]), bitorder="little")
    w = 1 << np.arange(16)
    out, b, i = [], 0, 0
    while i < n:
        if bits[b]:
            b += 9
            i += 1
        else:
            dist = int(bits[b + 1:b + 17] @ w)
            ln = int(bits[b + 17:b + 21] @ w[:4])
            out.append((i, ln, dist))
            b += 21
            i += ln
    return out
