"""The palette refinement of include/agmv.h ("palette refinement") stated in numpy, and the cases the tests share.

refine() is the definition: weighted k-means over the occupied bins of a histogram of AGMV_QuantizeColor codes, in exact
integers.  The distances go through a float64 matrix product, which is exact here: every term is an integer below 2^20.
The sums are uint64 and wrap modulo 2^64 like the library's."""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HIGH, MID, LOW = 1, 2, 3
BITS = {HIGH: (6, 6, 7), MID: (5, 6, 6), LOW: (5, 6, 5)}      # bits of R, G, B in a code (AGMV_QuantizeColor)
NCODES = {q: 1 << sum(b) for q, b in BITS.items()}            # 2^19, 2^17, 2^16: the all-ones code is the last
OPT_II, OPT_III = 2, 3                                        # a 256-colour and a 512-colour opt
SHAPES = ((512, 511), (256, 256))                             # (k, n_free) of the drivers


def quantize(pix, quality):
    """AGMV_QuantizeColor over an array of 0x00RRGGBB"""
    rb, gb, bb = BITS[quality]
    p = np.asarray(pix).astype(np.uint32)
    return (((p >> 16) & 255) >> (8 - rb)) << (gb + bb) | (((p >> 8) & 255) >> (8 - gb)) << bb | ((p & 255) >> (8 - bb))


def histogram(frames, quality):
    """what agmv_hip_histogram_dev fills: 2^19 u32 bins"""
    return np.bincount(quantize(frames, quality).reshape(-1), minlength=1 << 19).astype(np.uint32)


def centres(codes, quality):
    """[n, 3] int64: the centre of each code's bin, AGMV_ReverseQuantizeColor plus half a step per channel"""
    rb, gb, bb = BITS[quality]
    c = np.asarray(codes).astype(np.int64)
    ch = [(c >> (gb + bb)) & ((1 << rb) - 1), (c >> bb) & ((1 << gb) - 1), c & ((1 << bb) - 1)]
    return np.stack([(v << (8 - n)) + (1 << (7 - n)) for v, n in zip(ch, (rb, gb, bb))], axis=1)


def code_at(r, g, b, quality):
    return int(quantize(np.uint32(r << 16 | g << 8 | b), quality))


def unpack(pal):
    p = np.asarray(pal).astype(np.int64)
    return np.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], axis=1)


def assign(P, C):
    """nearest centroid of every point (lowest index on a tie) and its squared distance"""
    a = np.empty(len(P), np.int64)
    d = np.empty(len(P), np.uint64)
    Cf, cc = C.astype(np.float64), (C * C).sum(1).astype(np.float64)
    for i in range(0, len(P), 8192):
        p = P[i:i + 8192]
        m = (p * p).sum(1).astype(np.float64)[:, None] - 2.0 * (p.astype(np.float64) @ Cf.T) + cc[None, :]
        j = m.argmin(1)                                       # the first minimum: the lowest index
        a[i:i + 8192] = j
        d[i:i + 8192] = m[np.arange(len(p)), j].astype(np.uint64)
    return a, d


def refine(hist, quality, pal, n_free, iterations):
    """-> dict: pal (u32 [k]), rounds, sse (before, after), and per pass the distortion (`trace`) and the centroids (`history`)"""
    hist = np.asarray(hist, np.uint32)
    codes = np.flatnonzero(hist[:NCODES[quality]])
    w, P = hist[codes].astype(np.uint64), centres(codes, quality)
    c = np.array(pal, np.uint32)
    k, rounds, trace, history = len(c), 0, [], [c.copy()]
    for it in range(iterations + 1):
        a, d = assign(P, unpack(c))
        trace.append(int(np.sum(w * d, dtype=np.uint64)))
        if it == iterations:
            break
        W = np.zeros(k, np.uint64)
        np.add.at(W, a, w)
        new = np.zeros(k, np.uint64)
        for ch in range(3):
            S = np.zeros(k, np.uint64)
            np.add.at(S, a, w * P[:, ch].astype(np.uint64))
            new = new << np.uint64(8) | (S + W // np.uint64(2)) // np.maximum(W, np.uint64(1))
        moves = (np.arange(k) < n_free) & (W > 0)
        new = np.where(moves, new.astype(np.uint32), c)
        if (new == c).all():
            break
        c, rounds = new, rounds + 1
        history.append(c.copy())
    return {"pal": c, "rounds": rounds, "sse": (trace[0], trace[-1]), "trace": trace, "history": history}


def at(run, iterations):
    """the result of refine() with fewer iterations, read off a longer run: a run that changed centroids in R rounds is also the
    run of any limit >= R (pass R measures the centroids returned either way); below that the first `iterations` rounds all moved"""
    if iterations >= run["rounds"]:
        return run
    return {"pal": run["history"][iterations], "rounds": iterations, "sse": (run["trace"][0], run["trace"][iterations])}


# ---- the slot map of AGMV_BuildPalette and its inverse ------------------------------------------
def slots(c, mode512):
    """512 (256) colours -> palette0, palette1"""
    c = np.asarray(c, np.uint32)
    p0, p1 = np.zeros(256, np.uint32), np.zeros(256, np.uint32)
    if not mode512:
        p0[:] = c[:256]
        return p0, p1
    p0[:126], p1[:127], p0[127:], p1[127:] = c[:126], c[126:253], c[253:382], c[382:511]
    return p0, p1


def start_of(p0, p1, mode512):
    """the centroids the drivers start from, out of AGMV_BuildPalette's palettes: its pick list as colours, with centroid 511 = 0"""
    if not mode512:
        return np.array(p0, np.uint32)
    return np.concatenate([p0[:126], p1[:127], p0[127:], p1[127:], np.zeros(1, np.uint32)]).astype(np.uint32)


def build_palette(hist, quality, opt):
    """AGMV_BuildPalette of the host library -> (p0, p1) as uint32"""
    import hostlib as H
    p0, p1 = np.zeros(256, np.uint64), np.zeros(256, np.uint64)
    H.lib().AGMV_BuildPalette(np.ascontiguousarray(hist, np.uint32), quality, opt, p0, p1)
    return p0.astype(np.uint32), p1.astype(np.uint32)


def refined_palettes(hist, quality, opt, iterations):
    """the statement of AGMV_BuildPaletteRefined: pick, refinement, slot map -> (p0, p1, run)"""
    mode512 = opt not in (2, 4, 6)
    run = refine(hist, quality, start_of(*build_palette(hist, quality, opt), mode512), 511 if mode512 else 256, iterations)
    return slots(run["pal"], mode512) + (run,)


@functools.lru_cache(maxsize=None)
def fox_frames():
    f = np.load(os.path.join(HERE, "golden", "foxlogo.npz"))["frames"]
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def fox_hist(quality):
    h = histogram(fox_frames(), quality)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def fox_run(quality, k):
    """16 rounds over the golden clip's histogram from the drivers' start; computed once, at() gives the shorter runs"""
    mode512 = k == 512
    start = start_of(*build_palette(fox_hist(quality), quality, OPT_III if mode512 else OPT_II), mode512)
    start.setflags(write=False)
    return start, refine(fox_hist(quality), quality, start, 511 if mode512 else 256, 16)


def sparse_hist():
    """a crafted sparse histogram: few colours, far fewer than the palette has slots"""
    h = np.zeros(1 << 19, np.uint32)
    rng = np.random.default_rng(11)
    h[rng.integers(0, 1 << 16, 40)] = rng.integers(1, 5000, 40)
    return h


# ---- crafted histograms: where a kernel can go wrong -------------------------------------------
def rgb(r, g, b):
    return r << 16 | g << 8 | b


def crafted():
    """name -> (quality, hist, pal, n_free, iterations)"""
    cases = {}

    def hist_of(quality, points):
        h = np.zeros(1 << 19, np.uint32)
        for (r, g, b), w in points:
            code = code_at(r, g, b, quality)
            assert tuple(centres([code], quality)[0]) == (r, g, b), "not a bin centre: %r" % ((r, g, b),)
            h[code] = w
        return h

    # a point exactly between three centroids (distance 100 to each): index 0 takes it, index 2 stays empty
    cases["tie_lowest_index_wins"] = (HIGH, hist_of(HIGH, [((102, 102, 101), 5), ((90, 102, 101), 3)]),
                                      [rgb(112, 102, 101), rgb(92, 102, 101), rgb(102, 112, 101)], 3, 4)
    # two identical centroids: the second never receives a point in round 1 and keeps its colour
    cases["identical_centroids"] = (HIGH, hist_of(HIGH, [((98, 102, 101), 7), ((110, 98, 103), 2), ((30, 30, 31), 4)]),
                                    [rgb(100, 100, 100), rgb(100, 100, 100), rgb(20, 20, 20)], 3, 1)
    # a pinned centroid next to the heaviest cluster: it attracts the points and must not move
    cases["pinned_attracts"] = (HIGH, hist_of(HIGH, [((202, 198, 201), 900), ((206, 202, 203), 800), ((50, 50, 51), 10), ((58, 54, 51), 12)]),
                                [rgb(40, 40, 40), rgb(120, 120, 120), rgb(200, 200, 200)], 2, 8)
    rng = np.random.default_rng(3)
    blob = np.zeros(1 << 19, np.uint32)
    blob[rng.integers(0, 1 << 17, 3000)] = rng.integers(1, 1 << 20, 3000)
    cases["n_free_0"] = (MID, blob, list(rng.integers(0, 1 << 24, 5)), 0, 6)
    cases["k_1"] = (MID, blob, [rgb(1, 2, 3)], 1, 5)
    cases["single_bin"] = (LOW, hist_of(LOW, [((132, 62, 12), 77)]), [rgb(0, 0, 0), rgb(140, 60, 10), rgb(255, 255, 255)], 3, 3)
    cases["all_zero"] = (HIGH, np.zeros(1 << 19, np.uint32), list(rng.integers(0, 1 << 24, 9)), 9, 3)
    ones = hist_of(HIGH, [((22, 22, 21), 50), ((30, 26, 23), 60)])
    ones[NCODES[HIGH] - 1] = 1234                              # the all-ones code is a point like any other
    ones[NCODES[HIGH] - 2] = 99
    cases["all_ones_code"] = (HIGH, ones, [rgb(0, 0, 0), rgb(250, 250, 250)], 2, 4)
    for q, name in ((MID, "mid"), (LOW, "low")):
        top = blob.copy()
        top[NCODES[q]:] = 0
        top[NCODES[q] - 1] = 4000                              # the top code of the quality ...
        top[NCODES[q] - 300] = 17
        top[NCODES[q]:NCODES[q] + 64] = 0xFFFF                 # ... and bins behind it, which are not read
        cases["top_code_" + name] = (q, top, list(rng.integers(0, 1 << 24, 37)), 30, 6)
    # four bins of 0xFFFFFFFF in one cluster: W = 4 * (2^32 - 1) needs 64 bits, and B = (1 + 1 + 1 + 3) / 4 = 1.5 rounds up to 2
    F = 0xFFFFFFFF
    cases["full_bins_round_half_up"] = (HIGH, hist_of(HIGH, [((2, 2, 1), F), ((6, 2, 1), F), ((2, 6, 1), F), ((2, 2, 3), F), ((250, 250, 251), F), ((254, 250, 251), 7)]),
                                        [rgb(10, 10, 10), rgb(240, 240, 240)], 2, 3)
    # converges well before 64 rounds: the launches behind the round that changes nothing must do nothing
    cases["early_stop"] = (MID, blob, list(rng.integers(0, 1 << 24, 6)), 6, 64)
    return {n: (q, h, np.array(p, np.uint32), nf, it) for n, (q, h, p, nf, it) in cases.items()}
