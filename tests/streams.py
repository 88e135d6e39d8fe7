"""Seeded stream generators and oracle decodes from a given decoder state, shared by the prior-state tests
(tests/test_prior_state.py on the CPU, tests/test_prior_state_gpu.py on the GPU).  Test infrastructure only."""
import numpy as np

import oracles as O
import synth as S

FLAGS = [0x4E, 0x2F, 0x5E, 0x7F, 0xFF]         # FILL, NORMAL, COPY flags and the two escape-code bytes


def clip(rng, W, H, n):
    """n frames (H, W) of mixed content: noise, flat, synthetic, repeats, small changes, 8x8 tiles -- so that I, COPY,
    FILL and NORMAL blocks all occur (the content mix of test_fuzz_encode_decode_vs_oracle)"""
    frames, prevf = [], None
    for _ in range(n):
        kind = int(rng.integers(0, 6))
        if kind == 0 or prevf is None and kind == 3:
            f = rng.integers(0, 1 << 24, size=(H, W), dtype=np.uint32)
        elif kind == 1:
            f = np.full((H, W), int(rng.integers(0, 1 << 24)), np.uint32)
        elif kind == 2:
            f = S.synth_frame(max(W, 8), max(H, 8), int(rng.integers(0, 50)))[:H, :W].copy()
        elif kind == 3:
            f = prevf.copy()
        elif kind == 4:
            base = prevf if prevf is not None else np.zeros((H, W), np.uint32)
            f = base ^ rng.integers(0, 4, size=(H, W), dtype=np.uint32) * np.uint32(0x010101)
        else:
            f = np.repeat(np.repeat(rng.integers(0, 1 << 24, size=((H + 7) // 8, (W + 7) // 8), dtype=np.uint32), 8, 0), 8, 1)[:H, :W].copy()
        frames.append(f.astype(np.uint32))
        prevf = frames[-1]
    return np.stack(frames)


def palettes(rng, frames):
    return S.content_palettes(frames[:4]) if rng.integers(0, 2) else S.random_palettes(int(rng.integers(0, 1 << 30)))


def encode(W, H, mode512, p0, p1, frames, first_fc=0):
    """oracle encoder output of `frames`, frame f at frame_count first_fc + f (a batch that starts inside a GOP sees the
    fresh encoder's zeroed I-frame entries: the streams are valid input all the same)"""
    enc = O.OracleEncoder(W, H, mode512, p0, p1, first_fc)
    return [enc.encode(f) for f in frames]


def damage(rng, b, W, H, rate=3):
    """about one stream in `rate`: cut short, bytes overwritten with flag values, or random bytes spliced in (kept within the
    oracle decoder's persistent buffer of w*h*3+64 bytes)"""
    b = b.copy()
    hurt = int(rng.integers(0, 3 * rate))
    if hurt == 0 and len(b) > 1:
        b = b[:int(rng.integers(1, len(b)))]
    elif hurt == 1 and len(b):
        for _ in range(int(rng.integers(1, 6))):
            b[int(rng.integers(0, len(b)))] = FLAGS[int(rng.integers(0, len(FLAGS)))]
    elif hurt == 2:
        room = W * H * 3 + 64 - 16 - len(b)
        if room >= 1:
            at = int(rng.integers(0, len(b) + 1))
            b = np.concatenate([b[:at], rng.integers(0, 256, int(rng.integers(1, min(70, room) + 1)), dtype=np.uint8), b[at:]])
    return b


def block_soup(rng, W, H, n, mode512):
    """n streams that are sequences of blocks -- clean runs, FILL bodies holding flag values, escape codes, NORMAL blocks
    with flag-valued codes, stray bytes between blocks -- cut at every kind of length (test_fuzz_parser_block_sequences)"""
    nblk = W * H // 16
    cap = min(33 * nblk + 64, W * H * 3 + 64 - 16)
    p_copy, p_fill, p_norm, _ = rng.dirichlet([4, 4, 1, 0.3])
    spicy = np.array([0x4E, 0x5E, 0x2F, 0x7F, 0xFF, 0x7E, 0x00], np.uint8)

    def code():
        c = int(rng.choice(spicy)) if rng.random() < 0.25 else int(rng.integers(0, 256))
        if mode512 and (c & 0x7F) == 127:
            return [c, int(rng.integers(127, 256))]
        return [c]

    out = []
    for _ in range(n):
        buf = []
        for _ in range(int(nblk * rng.choice([0.3, 1.0, 1.0, 1.2])) + 1):
            r = rng.random()
            if r < p_copy:
                buf.append(0x5E)
            elif r < p_copy + p_fill:
                buf.append(0x4E)
                buf += code()
            elif r < p_copy + p_fill + p_norm:
                buf.append(0x2F)
                for _ in range(16):
                    buf += code()
            else:
                buf += [int(x) for x in rng.integers(0, 256, int(rng.integers(1, 4)))]
            if len(buf) >= cap:
                break
        buf = np.array(buf[:cap], np.uint8)
        cut = int(rng.choice([len(buf), len(buf), max(0, len(buf) - int(rng.integers(0, 70))), int(rng.integers(0, len(buf) + 1))]))
        out.append(buf[:cut].copy())
    return out


def prior_states(rng, W, H):
    """the three decoder states a range is decoded from: the fresh one (zeroed), S_A (random 24-bit img / iframe) and
    S_B = S_A ^ 0xFFFFFF, which differs from S_A at every pixel of both planes"""
    a = rng.integers(0, 1 << 24, size=(H, W), dtype=np.uint32)
    ai = rng.integers(0, 1 << 24, size=(H, W), dtype=np.uint32)
    m = np.uint32(0xFFFFFF)
    return {"zero": (None, None), "A": (a, ai), "B": (a ^ m, ai ^ m)}


def oracle_range(W, H, mode512, p0, p1, bits, first_fc, prev=None, prev_iframe=None):
    """decode the streams `bits` serially with the oracle started from (prev, prev_iframe, frame_count = first_fc) and a
    fresh bitstream buffer.  Returns (pixels [n, w*h], pads [n][16] = the stale bytes behind each stream, entry offsets
    [n, nblk], nentered [n]); the last three are functions of the streams alone."""
    dec = O.OracleDecoder(W, H, mode512, p0, p1)
    dec.set_state(prev, prev_iframe, first_fc)
    pix, pads, offs, nent = [], [], [], []
    for b in bits:
        p, padded, o, ne = dec.decode(b, want_tables=True)
        pix.append(p)
        pads.append(padded[len(b):len(b) + 16])
        offs.append(o)
        nent.append(ne)
    dec.close()
    return np.stack(pix), pads, np.stack(offs), np.array(nent, np.int64)


def slab(bits, pads, stride=None):
    """per-frame streams + their stale bytes -> ([n, stride] uint8 rows, bpos int32 [n]) as the GPU decoders take them"""
    n = len(bits)
    need = (max(len(b) for b in bits) + 16 + 255) & ~255
    stride = max(stride or 0, need)
    out = np.zeros((n, stride), np.uint8)
    bpos = np.zeros(n, np.int32)
    for i, b in enumerate(bits):
        out[i, :len(b)] = b
        out[i, len(b):len(b) + 16] = pads[i]
        bpos[i] = len(b)
    return out, bpos
