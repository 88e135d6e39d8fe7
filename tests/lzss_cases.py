"""Inputs and closed-form expectations for the LZSS stage (tests/test_lz_csize_tail.py, tests/test_gpu_lzss.py)."""
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
