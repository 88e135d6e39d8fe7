"""Inputs, references and closed-form expectations for the LZ77 stage on the GPU (tests/test_gpu_lz77.py,
tests/test_gpu_lz77_files.py, tests/test_lz77_abi.py)."""
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


def gpu_batch77(hip, streams, peek=None, stride_extra=0, out_extra=0):
    """one batched device call; rows at a stride larger than needed.  Checks the row contract of agmv_hip_lz77_frames_dev
    (include/agmv_hip.h): csize a multiple of 4 and <= 4 * size, 0 for an empty frame, every byte of a row behind csize
    keeps what it held (SENTINEL).  Returns the payloads."""
    import torch
    n = len(streams)
    sizes = np.array([len(x) for x in streams], np.int64)
    stride = int(max([1] + sizes.tolist())) + stride_extra
    bits = np.full((n, stride), 0xEE, np.uint8)                      # what lies behind a stream must never be read
    for i, x in enumerate(streams):
        bits[i, :len(x)] = x
    ostride = hip.lz77_max_csize(int(max([1] + sizes.tolist()))) + out_extra
    d_bits = torch.from_numpy(bits).cuda()
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
