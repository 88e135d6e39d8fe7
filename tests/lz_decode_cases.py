"""Inputs and the expected results for the decoder's LZ stage on the GPU (tests/test_gpu_lz_decode.py,
tests/test_lz_decode_abi.py).

Payloads always carry what follows them in a file (8 x 0xFF, then the next chunk's `AGFC` header): the reference stores
csize = floor(bits / 8), so the last LZSS token may read guard bits, and decode(lzss(x)) is not always x.  The expected
result is therefore always the host stage (agmv_lz_decode_mem) run on the same bytes, frame by frame over one persistent
buffer, as the sequence decoder does."""
import ctypes as C

import numpy as np

import hostlib as H

GUARD = bytes([0xFF] * 8) + b"AGFC" + bytes(12)


def lzss_tokens(tokens):
    """LSB-first LZSS stream of tokens ('L', byte) / ('M', offset, len); returns (bytes of the flushed stream, bits)"""
    acc, n = 0, 0
    for t in tokens:
        if t[0] == "L":
            acc |= (1 | (t[1] & 255) << 1) << n
            n += 9
        else:
            acc |= ((t[1] & 0xFFFF) << 1 | (t[2] & 15) << 17) << n
            n += 21
    return acc.to_bytes((n + 7) // 8, "little"), n


def lz77_tokens(tokens):
    """LZ77 stream of tokens (offset, len, byte)"""
    out = bytearray()
    for off, ln, b in tokens:
        out += bytes([off & 255, (off >> 8) & 255, ln & 255, b & 255])
    return bytes(out)


class Frame:
    """one chunk of a file image: payload bytes and the header's fields; avail (None = everything behind the header)"""

    def __init__(self, payload, usize, csize, avail=None, guard=GUARD):
        self.payload = bytes(payload)
        self.usize, self.csize, self.avail = int(usize), int(csize), avail
        self.guard = guard


def lzss_frame(tokens, usize=None, csize=None, guard=GUARD):
    b, nbits = lzss_tokens(tokens)
    cs = nbits // 8 if csize is None else csize
    out = sum(1 if t[0] == "L" else t[2] for t in tokens)
    return Frame(b[:min(cs, len(b))], out if usize is None else usize, cs, guard=guard)


def chain_frame(n_matches, lead=0x5A, offset=1, length=15):
    """a literal, then n_matches equal matches (offset, length), built with numpy (lzss_tokens is quadratic in the stream
    length); csize = floor(bits / 8), so the last match may read guard bits"""
    lit = np.array([1] + [(lead >> i) & 1 for i in range(8)], np.uint8)
    m = np.array([0] + [(offset >> i) & 1 for i in range(16)] + [(length >> i) & 1 for i in range(4)], np.uint8)
    bits = np.concatenate([lit, np.tile(m, n_matches)])
    cs = len(bits) // 8
    return Frame(np.packbits(bits, bitorder="little")[:cs].tobytes(), 1 + n_matches * length, cs)


def lz77_frame(tokens, usize=None, csize=None):
    b = lz77_tokens(tokens)
    out = sum(t[1] + 1 for t in tokens)
    return Frame(b, out if usize is None else usize, len(b) if csize is None else csize)


def image(frames):
    """a file image: per frame a 16-byte chunk header, the payload and its guard.  Returns (src, off, avail)"""
    src = bytearray()
    off, avail = [], []
    for k, fr in enumerate(frames):
        src += b"AGFC" + k.to_bytes(4, "little") + (fr.usize & 0xFFFFFFFF).to_bytes(4, "little") + \
            (fr.csize & 0xFFFFFFFF).to_bytes(4, "little")
        off.append(len(src))
        src += fr.payload + fr.guard
    for k, fr in enumerate(frames):
        avail.append(len(src) - off[k] if fr.avail is None else fr.avail)
    return np.frombuffer(bytes(src) + bytes(1), np.uint8)[:len(src)].copy(), np.array(off, np.int64), np.array(avail, np.int64)


def host_lz(version, src, off, avail, usize, csize, cap, stride):
    """agmv_lz_decode_mem per frame into fresh rows; returns (rows [n, stride], bpos, used)"""
    n = len(off)
    rows = np.zeros((n, stride), np.uint8)
    bpos = np.zeros(n, np.int64)
    used = np.zeros(n, np.int64)
    L = H.lib()
    for f in range(n):
        u = C.c_size_t(0)
        buf = np.ascontiguousarray(src[int(off[f]):int(off[f]) + int(avail[f])])
        if buf.size == 0:
            buf = np.zeros(1, np.uint8)
        row = np.zeros(max(cap, 1), np.uint8)
        bpos[f] = L.agmv_lz_decode_mem(version, buf, int(avail[f]), int(usize[f]), int(csize[f]), row, cap, C.byref(u))
        used[f] = u.value
        rows[f, :bpos[f]] = row[:bpos[f]]
    return rows, bpos, used


def commit(rows, bpos, persist, n=None):
    """numpy restatement of the sequence decoder's loop over the persistent buffer (agmv_decode_stream):
    memcpy(row + bp, persist + bp, 16) clipped to the stride (and the buffer); memcpy(persist, row, min(bp, cap))"""
    cap, stride = len(persist), rows.shape[1]
    for f in range(len(bpos) if n is None else n):
        bp = int(bpos[f])
        e = min(bp + 16, stride, cap)
        if e > bp:
            rows[f, bp:e] = persist[bp:e]
        persist[:min(bp, cap)] = rows[f, :min(bp, cap)]
    return rows, persist


def host_batch(version, frames, cap, persist=None, stride=None):
    """the expected result of lz_decode_frames_dev + lz_decode_commit_dev on image(frames)"""
    src, off, avail = image(frames)
    stride = cap if stride is None else stride
    rows, bpos, used = host_lz(version, src, off, avail, [f.usize for f in frames], [f.csize for f in frames], cap, stride)
    per = np.zeros(cap, np.uint8) if persist is None else np.array(persist, np.uint8, copy=True)
    before = rows.copy()
    rows, per = commit(rows, bpos, per)
    return before, rows, bpos, used, per


def splash_rng_cases(rng):
    """small pre-LZ inputs of several kinds: runs, repeats, noise, empty and 1-byte streams"""
    xs = [np.zeros(0, np.uint8), np.array([7], np.uint8), np.zeros(40, np.uint8), np.zeros(1000, np.uint8),
          rng.integers(0, 256, 300, dtype=np.uint8), np.tile(rng.integers(0, 256, 37, dtype=np.uint8), 80),
          rng.integers(0, 3, 5000, dtype=np.uint8), np.arange(256, dtype=np.uint8).repeat(7)]
    for n in (2, 3, 4, 5, 17, 18, 19, 30, 31, 33, 64, 65):
        xs.append(rng.integers(0, 4, n, dtype=np.uint8))
    return xs
