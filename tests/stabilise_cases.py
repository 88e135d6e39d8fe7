"""The temporal stabilisation of include/agmv.h ("temporal stabilisation") stated in numpy, the crafted blocks, the random clips
and the noisy still clip the tests share (tests/test_stabilise_cpu.py on the CPU, tests/test_gpu_stabilise*.py on the GPU).  The
statement follows the header's wording frame by frame; nothing here calls a GPU."""
import functools

import numpy as np

import dither_cases as D

STRENGTHS = (1, 16, 64)                          # of the crafted blocks: the ends of the range and one between
NOISY_SIGMA, NOISY_STRENGTH, NOISY_FRAMES = 3, 32, 8     # the noisy still clip, and a strength at which every block of it is still


def anchors(n, first_fc):
    """-> (k, a): the frames k of a batch of n frames from frame count first_fc on that have their anchor a = k - (fc & 3) in the
    batch, both int64 arrays"""
    k = np.arange(n, dtype=np.int64)
    phase = (first_fc + k) & 3
    ok = (phase != 0) & (k - phase >= 0)
    return k[ok], (k - phase)[ok]


def still_blocks(frame, anchor, s):
    """bool [..., h // 4, w // 4]: max(d) <= s and sum(d) <= 12 * s over the 48 differences of each block, bits 0 .. 23 only"""
    d = np.abs(D.channels(np.asarray(frame, np.uint32) & np.uint32(0xFFFFFF)) - D.channels(np.asarray(anchor, np.uint32) & np.uint32(0xFFFFFF)))
    h, w = d.shape[-3:-1]
    b = d.reshape(d.shape[:-3] + (h // 4, 4, w // 4, 4, 3))
    return (b.max(axis=(-4, -2, -1)) <= s) & (b.sum(axis=(-4, -2, -1)) <= 12 * s)


def stabilise(frames, s, first_fc=0):
    """frames uint32 [n, h, w] with frame counts first_fc + k -> (the stabilised clip, examined, replaced): the blocks of the
    P-frames that have their anchor in the batch, and those of them that were replaced"""
    frames = np.asarray(frames, np.uint32)
    n, h, w = frames.shape
    assert h % 4 == 0 and w % 4 == 0 and 1 <= s <= 64
    out = frames.copy()
    k, a = anchors(n, first_fc)
    if len(k) == 0:
        return out, 0, 0
    anchor = frames[a]                               # (an anchor has fc & 3 == 0 and is never changed itself)
    still = still_blocks(frames[k], anchor, s)
    mask = np.repeat(np.repeat(still, 4, axis=1), 4, axis=2)
    out[k] = np.where(mask, anchor & np.uint32(0xFFFFFF), frames[k])
    return out, int(still.size), int(still.sum())


# ---- crafted blocks: per strength a list of (what it is, the 48 signed differences [4, 4, 3] (R, G, B), the XOR of bits 24 .. 31
# of the P-frame's pixels against the anchor's, whether the block is still)
def crafted_blocks(s):
    zero = np.zeros((4, 4, 3), np.int64)
    cases = []

    def add(name, d, high, still):
        cases.append((name, d, high, still))
    for v, still in ((s, True), (s + 1, False)):
        d = zero.copy()
        d[2, 1, 1] = v
        add("max(d) = %d" % v, d, 0, still)
    twelve = zero.copy().reshape(-1)
    twelve[np.arange(12) * 4] = s * np.where(np.arange(12) & 1, -1, 1)       # 12 differences of s, both signs, spread over the block
    add("sum(d) = 12 s", twelve.reshape(4, 4, 3), 0, True)
    more = twelve.copy()
    more[47] = -1
    add("sum(d) = 12 s + 1, every difference <= s", more.reshape(4, 4, 3), 0, False)
    for place in range(48):
        for sign in (1, -1):
            for v, still in ((s + 1, False), (s, True)):
                d = zero.copy().reshape(-1)
                d[place] = sign * v
                add("one difference of %+d at place %d" % (sign * v, place), d.reshape(4, 4, 3), 0, still)
    add("differences in bits 24 .. 31 only", zero, 0xFF, True)
    d = zero.copy()
    d[0, 0, 0] = -(s + 1)
    add("bits 24 .. 31 of a block that is not still", d, 0x81, False)
    return cases


BLOCKS_PER_ROW = 16


@functools.lru_cache(maxsize=None)
def crafted_clip(s):
    """-> (frames uint32 [2, h, 64]: an I-frame and one P-frame, frame counts 0 and 1, one crafted block per 4x4 place in row-major
    order; still bool [h // 4, 16]; the names).  Places behind the last case hold equal blocks (still)."""
    cases = crafted_blocks(s)
    rows = -(-len(cases) // BLOCKS_PER_ROW)
    rng = np.random.default_rng(900 + s)
    base = rng.integers(70, 186, (rows * 4, BLOCKS_PER_ROW * 4, 3)).astype(np.int64)       # +-65 stays inside 0 .. 255
    high = rng.integers(0, 256, (rows * 4, BLOCKS_PER_ROW * 4)).astype(np.int64)
    p, phigh = base.copy(), high.copy()
    still = np.ones((rows, BLOCKS_PER_ROW), bool)
    for i, (_, d, hx, st) in enumerate(cases):
        y, x = i // BLOCKS_PER_ROW * 4, i % BLOCKS_PER_ROW * 4
        p[y:y + 4, x:x + 4] += d
        phigh[y:y + 4, x:x + 4] ^= hx
        still[i // BLOCKS_PER_ROW, i % BLOCKS_PER_ROW] = st
    assert p.min() >= 0 and p.max() <= 255
    pack = lambda c, hi: (hi << 24 | c[..., 0] << 16 | c[..., 1] << 8 | c[..., 2]).astype(np.uint32)
    return np.stack([pack(base, high), pack(p, phigh)]), still, [c[0] for c in cases]


def random_clip(n, h, w, s, seed):
    """a clip whose blocks differ from frame 0's by noise of an amplitude drawn per frame and block from 0, s/4, s/2, s and 2s, with
    random bits 24 .. 31: some blocks pass both tests, some fail the sum, some the maximum"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (1, h, w, 3)).astype(np.int64)
    amp = rng.choice(np.array([0, max(s // 4, 1), max(s // 2, 1), s, 2 * s]), (n, h // 4, w // 4))
    amp = np.repeat(np.repeat(amp, 4, axis=1), 4, axis=2)[..., None]
    c = np.clip(base + np.rint((rng.random((n, h, w, 3)) * 2 - 1) * amp).astype(np.int64), 0, 255)
    hi = rng.integers(0, 256, (n, h, w)).astype(np.int64)
    return (hi << 24 | c[..., 0] << 16 | c[..., 1] << 8 | c[..., 2]).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def noisy_still_clip(sigma=NOISY_SIGMA, n=NOISY_FRAMES):
    """frame 5 of the golden clip held for n frames, Gaussian noise of sigma levels added per frame and channel (default_rng(7)),
    rounded and clipped -> (noisy uint32 [n, 240, 320], the clean clip)"""
    still = D.fox()[0][D.FOX_FRAME]
    clean = np.broadcast_to(still, (n,) + still.shape).copy()
    c = np.clip(D.channels(clean) + np.rint(np.random.default_rng(7).normal(0.0, sigma, clean.shape + (3,))).astype(np.int64), 0, 255)
    return (c[..., 0] << 16 | c[..., 1] << 8 | c[..., 2]).astype(np.uint32), clean
