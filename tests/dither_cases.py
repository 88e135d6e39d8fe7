"""The pattern dithering of include/agmv.h ("pattern dithering") stated in numpy, a brute-force nearest entry by the rules of
AGMV_FindNearestColor / AGMV_FindNearestEntry, the crafted palettes and the measure the tests share (tests/test_dither_cpu.py on
the CPU, tests/test_gpu_dither*.py on the GPU).  The statement takes `nearest` as an argument: the CPU tests pass the brute
force, the GPU tests the context's own exact table, which the existing suite proves."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B4 = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.int64)
FOX_FRAME = 5                                   # the frame of tests/golden/foxlogo.npz the measurements are made on


def channels(pix):
    """uint32 0x??RRGGBB [...] -> int64 [..., 3]"""
    p = np.asarray(pix).astype(np.int64)
    return np.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], axis=-1)


def rgb(r, g, b):
    return (r << 16) | (g << 8) | b


def pal512_of(p0, p1=None):
    p1 = np.zeros(256, np.uint32) if p1 is None else p1
    return np.concatenate([np.asarray(p0, np.uint32), np.asarray(p1, np.uint32)])


def brute_nearest(pal512, mode512):
    """-> nearest(colours uint32 [...]) -> entries int64 [...]: the argmin of the squared distance over palette 0 (and palette 1),
    the lowest index on a tie inside a palette and palette 0 on a tie between the two.  Every distinct colour is searched once."""
    pc = channels(np.asarray(pal512, np.uint32)[:512 if mode512 else 256])
    memo = {}

    def nearest(colours):
        c = np.asarray(colours, np.uint32) & np.uint32(0xFFFFFF)
        uniq, inv = np.unique(c, return_inverse=True)
        new = np.array([u for u in uniq.tolist() if u not in memo], np.uint32)
        for lo in range(0, len(new), 4096):
            part = new[lo:lo + 4096]
            d = ((channels(part)[:, None, :] - pc[None, :, :]) ** 2).sum(axis=2)
            for u, e in zip(part.tolist(), d.argmin(axis=1).tolist()):      # (argmin: the first minimum in the order p0 | p1)
                memo[u] = e
        return np.array([memo[u] for u in uniq.tolist()], np.int64)[inv].reshape(c.shape)
    return nearest


def table_nearest(table):
    """-> nearest from a table of all 2^24 entries, table[0xRRGGBB]"""
    return lambda colours: table[np.asarray(colours, np.uint32) & np.uint32(0xFFFFFF)].astype(np.int64)


_tables = {}


def use_palette(torch, hip, pal512, mode512):
    """GPU: sets the palette on the context `hip`; -> nearest() of the statement from the context's own exact table, downloaded
    once per palette with quantise_dev over all 2^24 colours"""
    pal512 = np.ascontiguousarray(pal512, np.uint32)
    hip.set_palette(pal512[:256], pal512[256:], mode512)
    key = (pal512.tobytes(), bool(mode512))
    if key not in _tables:
        every = torch.arange(1 << 24, dtype=torch.int32, device="cuda")
        _tables[key] = hip.quantise_dev(every).cpu().numpy().view(np.uint16)
        assert int(_tables[key].max()) < (512 if mode512 else 256)
    return table_nearest(_tables[key])


def candidates(pix, pal512, mode512, s, nearest):
    """the 16 entries e_0 .. e_15 of every pixel, int64 [16, ...], in the order the definition finds them"""
    pal = np.asarray(pal512, np.uint32) & np.uint32(0xFFFFFF)
    assert pal.shape == (512,) and 1 <= s <= 64
    pc, px = channels(pal), channels(np.asarray(pix, np.uint32) & np.uint32(0xFFFFFF))
    acc = np.zeros_like(px)
    out = np.empty((16,) + px.shape[:-1], np.int64)
    for i in range(16):
        a = np.clip(px + ((acc * s) >> 6), 0, 255)                          # (>> on negative int64 rounds down)
        e = nearest((a[..., 0] << 16 | a[..., 1] << 8 | a[..., 2]).astype(np.uint32))
        assert ((e >= 0) & (e < (512 if mode512 else 256))).all()
        acc += px - pc[e]
        assert np.abs(acc).max() <= 16 * 255
        out[i] = e
    return out


def dither(frames, pal512, mode512, s, nearest):
    """frames uint32 [n, h, w] -> the dithered frames, uint32 [n, h, w]"""
    frames = np.asarray(frames, np.uint32)
    n, h, w = frames.shape
    pal = np.asarray(pal512, np.uint32) & np.uint32(0xFFFFFF)
    pc = channels(pal)
    e = candidates(frames, pal512, mode512, s, nearest)
    keys = np.sort((299 * pc[e, 0] + 587 * pc[e, 1] + 114 * pc[e, 2]) * 512 + e, axis=0)
    assert keys.max() < 1 << 27
    t = B4[np.arange(h)[:, None] & 3, np.arange(w)[None, :] & 3]
    pick = np.take_along_axis(keys, np.broadcast_to(t, (1, n, h, w)), axis=0)[0]
    return pal[pick & 511]


def quantised(frames, pal512, nearest):
    """every pixel as its nearest palette colour: what the encoder makes of an undithered clip"""
    return (np.asarray(pal512, np.uint32) & np.uint32(0xFFFFFF))[nearest(frames)]


def block_sums(frames):
    """int64 [n, h // 4, w // 4, 3]: the channel sums of the whole 4x4 blocks"""
    c = channels(np.asarray(frames, np.uint32))
    n, h, w, _ = c.shape
    return c[:, :h // 4 * 4, :w // 4 * 4].reshape(n, h // 4, 4, w // 4, 4, 3).sum(axis=(2, 4))


def block_sum_error(out, src):
    """the sum over 4x4 blocks and channels of (sum of out - sum of src)^2: 256 times the squared error of the box means"""
    return int(((block_sums(out) - block_sums(src)) ** 2).sum())


def uniform_blocks(frames):
    c = channels(np.asarray(frames, np.uint32))
    n, h, w, _ = c.shape
    b = c.reshape(n, h // 4, 4, w // 4, 4, 3)
    return int((b == b[:, :, :1, :, :1, :]).all(axis=(2, 4, 5)).sum())


@functools.lru_cache(maxsize=None)
def fox():
    """-> (the 24 golden frames uint32 [24, 240, 320], p0, p1)"""
    z = np.load(os.path.join(GOLDEN, "foxlogo.npz"))
    return z["frames"].astype(np.uint32), z["p0"].astype(np.uint32), z["p1"].astype(np.uint32)


def fox_palette(mode512):
    _, p0, p1 = fox()
    return pal512_of(p0, p1 if mode512 else None)


# ---- crafted palettes: name -> (pal512, mode512, frames uint32 [n, h, w], what the case is there for)
GREY = rgb(200, 200, 200)


@functools.lru_cache(maxsize=None)
def crafted():
    rng = np.random.default_rng(2024)
    cases = {}
    # 128 colours, each in two slots of palette 0 and again in palette 1: the lowest slot must win everywhere
    c128 = rng.integers(0, 1 << 24, 128).astype(np.uint32)
    dup = np.concatenate([c128, c128])
    cases["duplicate_colours"] = (pal512_of(dup, dup[::-1].copy()), True, rng.integers(0, 1 << 24, (2, 5, 7)).astype(np.uint32))
    cases["all_black"] = (np.zeros(512, np.uint32), True, rng.integers(0, 1 << 24, (1, 4, 8)).astype(np.uint32))
    # two colours, the pixel exactly midway: slot 0 black, every other slot one grey
    two = np.full(256, GREY, np.uint32)
    two[0] = 0
    mid = np.full((1, 8, 8), rgb(100, 100, 100), np.uint32)
    cases["two_colours_midway"] = (pal512_of(two), False, mid)
    # a palette of mid greys, pixels far outside it: the clamps at 0 and at 255
    greys = np.array([rgb(v, v, v) for v in 120 + (np.arange(256) % 16)], np.uint32)
    ends = np.zeros((1, 4, 8), np.uint32)
    ends[0, :, 4:] = 0xFFFFFF
    ends[0, 2:, :] |= 0xA5000000                                             # (bits >= 24 are ignored)
    cases["clamps_at_both_ends"] = (pal512_of(greys), False, ends)
    return cases
