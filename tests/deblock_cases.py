"""The deblocking rule of include/agmv.h ("deblocking") stated in numpy, and the crafted lines and clips the tests share
(tests/test_deblock_cpu.py on the CPU, tests/test_gpu_deblock*.py on the GPU).  The statement follows the header's wording: two
stages, each a function of its input only, and the two counters.  deblock_cells evaluates the same rule cell by cell, the way the
kernel does.  Nothing here calls a GPU."""
import functools

import numpy as np

STRENGTHS = (1, 3, 4, 16, 64)                    # the ends of the range, s >> 2 == 0 (1, 3), its first non-zero value (4), one between


def channels(x):
    """uint32 [...] -> int64 [..., 3]: R, G, B"""
    x = np.asarray(x, np.uint32).astype(np.int64)
    return np.stack([(x >> 16) & 255, (x >> 8) & 255, x & 255], axis=-1)


def pack(c, top=0):
    """int64 [..., 3] R, G, B and the top bytes -> uint32"""
    c = np.asarray(c, np.int64)
    return (np.asarray(top, np.int64) << 24 | c[..., 0] << 16 | c[..., 1] << 8 | c[..., 2]).astype(np.uint32)


def filter_lines(p1, p0, q0, q1, s):
    """the decision and both filters on arrays of lines, int64 [..., 3] each -> (p1', p0', q0', q1', weak, strong), the last two
    bool [...]"""
    step = np.abs(p0 - q0).max(-1)
    side = np.maximum(np.abs(p1 - p0), np.abs(q1 - q0)).max(-1)
    on = (step >= 1) & (step <= s)
    strong = on & (side <= (s >> 2))
    weak = on & ~strong
    a, b = p1 + p0, q0 + q1
    st, wk = strong[..., None], weak[..., None]
    o1 = np.where(st, (7 * a + b + 8) >> 4, p1)
    o0 = np.where(st, (5 * a + 3 * b + 8) >> 4, np.where(wk, (p1 + 2 * p0 + q0 + 2) >> 2, p0))
    r0 = np.where(st, (3 * a + 5 * b + 8) >> 4, np.where(wk, (p0 + 2 * q0 + q1 + 2) >> 2, q0))
    r1 = np.where(st, (a + 7 * b + 8) >> 4, q1)
    return o1, o0, r0, r1, weak, strong


def stage(c, s):
    """one stage along the last pixel axis: c int64 [..., L, 3] with L a multiple of 4, the edges at 4, 8, ..., L - 4, all at once
    -> (the result, weak, strong)"""
    L = c.shape[-2]
    b = c.reshape(c.shape[:-2] + (L // 4, 4, 3)).copy()
    if L == 4:
        return c.copy(), 0, 0
    o1, o0, r0, r1, weak, strong = filter_lines(b[..., :-1, 2, :], b[..., :-1, 3, :], b[..., 1:, 0, :], b[..., 1:, 1, :], s)
    b[..., :-1, 2, :], b[..., :-1, 3, :], b[..., 1:, 0, :], b[..., 1:, 1, :] = o1, o0, r0, r1
    return b.reshape(c.shape), int(weak.sum()), int(strong.sum())


def deblock(frames, s):
    """frames uint32 [n, h, w] -> (the deblocked clip uint32, weak, strong): vertical edges of the decoded frame, then horizontal
    edges of that result; the top byte of every pixel is the source's"""
    frames = np.asarray(frames, np.uint32)
    n, h, w = frames.shape
    assert h % 4 == 0 and w % 4 == 0 and h and w and 1 <= s <= 64
    c1, w1, s1 = stage(channels(frames), s)                                  # lines along x
    c2, w2, s2 = stage(np.ascontiguousarray(c1.transpose(0, 2, 1, 3)), s)     # lines along y
    out = c2.transpose(0, 2, 1, 3)
    assert out.min() >= 0 and out.max() <= 255
    return pack(out) | (frames & np.uint32(0xFF000000)), w1 + w2, s1 + s2


def lines_examined(n, h, w):
    return n * ((w // 4 - 1) * h + (h // 4 - 1) * w)


def deblock_cells(frames, s):
    """the same rule cell by cell: the frame padded by 2 pixels all round falls into (w / 4 + 1) x (h / 4 + 1) cells of 4 x 4, each
    evaluated from its own 16 pixels -- its rows, then its columns, a line only where all four of its pixels lie in the frame"""
    frames = np.asarray(frames, np.uint32)
    n, h, w = frames.shape
    c = np.zeros((n, h + 4, w + 4, 3), np.int64)
    c[:, 2:-2, 2:-2] = channels(frames)
    inside = np.zeros((h + 4, w + 4), bool)
    inside[2:-2, 2:-2] = True
    ch, cw = h // 4 + 1, w // 4 + 1
    cells = c.reshape(n, ch, 4, cw, 4, 3).transpose(0, 1, 3, 2, 4, 5).copy()       # [n, cy, cx, row, column, 3]
    valid = inside.reshape(ch, 4, cw, 4).transpose(0, 2, 1, 3)                        # [cy, cx, row, column]
    weak = strong = 0
    for axis in (0, 1):                                                               # rows of the cell, then its columns
        x = cells if axis == 0 else cells.swapaxes(3, 4)
        v = valid if axis == 0 else valid.swapaxes(2, 3)
        o1, o0, r0, r1, wk, st = filter_lines(x[..., 0, :], x[..., 1, :], x[..., 2, :], x[..., 3, :], s)
        on = v.all(-1)[None]                                                          # [1, cy, cx, line]
        new = np.stack([o1, o0, r0, r1], axis=-2)
        x = np.where(on[..., None, None], new, x)
        weak += int((wk & on).sum())
        strong += int((st & on).sum())
        cells = x if axis == 0 else x.swapaxes(3, 4)
    out = cells.transpose(0, 1, 3, 2, 4, 5).reshape(n, h + 4, w + 4, 3)[:, 2:-2, 2:-2]
    return pack(out) | (frames & np.uint32(0xFF000000)), weak, strong


# ---- crafted lines: per strength a list of (what it is, [4, 3] R, G, B of p1 p0 q0 q1, "none" | "weak" | "strong")
def crafted_lines(s):
    q = s >> 2
    cases = []

    def add(name, p1, p0, q0, q1, kind):
        line = np.array([p1, p0, q0, q1], np.int64)
        assert line.min() >= 0 and line.max() <= 255, name
        cases.append((name, line, kind))
    g = 100
    flat = lambda v: (v, v, v)
    for c in range(3):
        one = lambda v, c=c: tuple(v if k == c else g for k in range(3))
        for sign in (1, -1):
            add("step == s in channel %d, sign %+d" % (c, sign), flat(g), flat(g), one(g + sign * s), one(g + sign * s), "strong")
            add("step == s + 1 in channel %d, sign %+d" % (c, sign), flat(g), flat(g), one(g + sign * (s + 1)), one(g + sign * (s + 1)), "none")
            # one channel alone over the limit vetoes a line that the two others would filter
            add("channel %d alone over the limit, sign %+d" % (c, sign), flat(g), flat(g),
                tuple(g + sign * (s + 1) if k == c else g + 1 for k in range(3)), tuple(g + sign * (s + 1) if k == c else g + 1 for k in range(3)), "none")
            add("side == s >> 2 on the p side, channel %d, sign %+d" % (c, sign), one(g + sign * q), flat(g), flat(g + 1), flat(g + 1), "strong")
            add("side == (s >> 2) + 1 on the p side, channel %d, sign %+d" % (c, sign), one(g + sign * (q + 1)), flat(g), flat(g + 1), flat(g + 1), "weak")
            add("side == s >> 2 on the q side, channel %d, sign %+d" % (c, sign), flat(g), flat(g), flat(g + 1), tuple(g + 1 + (sign * q if k == c else 0) for k in range(3)), "strong")
            add("side == (s >> 2) + 1 on the q side, channel %d, sign %+d" % (c, sign), flat(g), flat(g), flat(g + 1), tuple(g + 1 + (sign * (q + 1) if k == c else 0) for k in range(3)), "weak")
    add("step == 0 with busy sides", flat(40), flat(g), flat(g), flat(200), "none")
    add("0 | s, flat", flat(0), flat(0), flat(s), flat(s), "strong")
    add("255 | 255 - s, flat", flat(255), flat(255), flat(255 - s), flat(255 - s), "strong")
    add("0 255 | 255 - s .., weak at the ends of the range", flat(0), flat(255), flat(255 - s), flat(0), "weak")
    add("255 0 | s 255, weak at the ends of the range", flat(255), flat(0), flat(s), flat(255), "weak")
    add("a large side with a step of 1", flat(255), flat(0), flat(1), flat(255), "weak")
    return cases


@functools.lru_cache(maxsize=None)
def crafted_clip(s):
    """-> uint32 [2, h, w]: frame 0 has every crafted line of strength s as a row across the one vertical edge of an 8-pixel-wide
    frame (columns 0 1 hold p1, columns 6 7 hold q1); frame 1 has them as columns 2 .. 5 of an 8-wide pair of blocks across the edge
    y = 4 of an 8-row band, transposed, so that stage 1 leaves those columns alone and stage 2 meets the crafted values.  Both frames
    have the size of the larger, the rest filled with a flat colour; random top bytes."""
    cases = crafted_lines(s)
    k = len(cases)
    h, w = max(-(-k // 4) * 4, 8), 8 * k
    rng = np.random.default_rng(40 + s)
    c = np.full((2, h, w, 3), 100, np.int64)
    for i, (_, line, _) in enumerate(cases):
        c[0, i, 0:2], c[0, i, 2:6], c[0, i, 6:8] = line[0], line, line[3]
        c[1, 0:2, 8 * i:8 * i + 8], c[1, 2:6, 8 * i:8 * i + 8], c[1, 6:8, 8 * i:8 * i + 8] = line[0], line[:, None, :], line[3]
    return pack(c, rng.integers(0, 256, (2, h, w)))


def flat_blocks(a, b, h=8, w=8):
    """one frame of flat 4x4 blocks in a checkerboard of the grey levels a and b"""
    yy, xx = np.mgrid[0:h, 0:w]
    v = np.where(((yy // 4) + (xx // 4)) & 1, b, a).astype(np.int64)
    return pack(np.stack([v, v, v], -1))[None]


def staircase_clip(n, h, w, seed, levels=8, noise=2, gain=1):
    """what a decoder of flat FILL blocks gives: a gradient (its slope divided by `gain`) quantised per 4x4 block to levels `levels`
    apart, plus noise of a per-block amplitude drawn from 0, 1 and `noise` (some lines strong, some weak, some busy beyond the
    strength), random top bytes"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 3 + yy, 255 * gain - xx * 2 - yy, xx + yy * 3], -1) // gain % 256
    blk = base.reshape(h // 4, 4, w // 4, 4, 3).mean((1, 3)).round().astype(np.int64) // levels * levels
    c = np.repeat(np.repeat(blk, 4, 0), 4, 1)[None] + np.zeros((n, 1, 1, 1), np.int64)
    amp = rng.choice(np.array([0, 1, noise]), (n, h // 4, w // 4))
    amp = np.repeat(np.repeat(amp, 4, 1), 4, 2)[..., None]
    c = np.clip(c + np.rint((rng.random((n, h, w, 3)) * 2 - 1) * amp).astype(np.int64), 0, 255)
    return pack(c, rng.integers(0, 256, (n, h, w)))
