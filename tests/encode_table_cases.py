"""Crafted palettes and entry planes for k_encode's block decisions and byte emission (tests/test_gpu_encode_table.py), built
and proved on the CPU (tests/test_encode_table_cpu.py).  Nothing here needs a GPU.

Every case is a plane of ENTRIES (pal_num << 8 | index) under a palette of 512 pairwise distinct colours, so the pixel frame
pal[entries] quantises back to exactly those entries (distance 0, no tie) and both of the library's paths -- pixels and
entries -- have to give the bytes the oracle assembles from the plane.

Lattice palette: the 8 x 8 x 8 lattice 16 + 32 i, permuted over the 512 slots: no two colours are within +-2, the predicate holds
for equal entries only.  Cluster palette: eight clusters, 60 or more apart, of the 64 colours base + {0, 2, 3, 5}^3: inside a
cluster every signed channel difference 0, +-1, +-2, +-3, +-5 occurs.  Clusters 0 .. 3 are spread over slots 0 .. 255 and clusters
4 .. 7 over slots 256 .. 511 by a fixed permutation, so palette 0 alone (the 256-colour cases) holds whole clusters.

A block's 16 entries are listed in the order of the stream: row by row, pixel i = 4 * row + column."""
import functools

import numpy as np

import oracles as O

COPY, FILL, NORMAL = 0x5E, 0x4E, 0x2F
KINDS = (COPY, FILL, NORMAL)
COPY_COUNT, FILL_COUNT = 13, 14
ENC_T, WAVE = 512, 64                                          # blocks per tile and per wave of k_encode
LO, HI = np.array([0, 1, 125, 126]), np.array([127, 128, 254, 255])     # indices without / with an escape byte
SPECIAL = (0, 126, 127, 128, 255)


def _frozen(a):
    a.setflags(write=False)
    return a


def mix(x):
    """a 32-bit hash of integers (numpy, element-wise)"""
    x = np.asarray(x).astype(np.uint64)
    x = (x * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    return x.astype(np.int64)


# ---- palettes ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice_palette():
    """u32 [512]: slot s = pal_num << 8 | index"""
    v = 16 + 32 * np.arange(8)
    col = (v[:, None, None] << 16 | v[None, :, None] << 8 | v[None, None, :]).reshape(-1).astype(np.uint32)
    return _frozen(col[np.random.default_rng(0x1A77).permutation(512)])


V = np.array([0, 2, 3, 5])
BASES = np.array([(0, 0, 0), (250, 250, 250), (0, 120, 250), (250, 0, 120), (120, 250, 0), (60, 180, 60), (180, 60, 180), (120, 120, 120)])
COORDS = np.array([(V[m >> 4], V[(m >> 2) & 3], V[m & 3]) for m in range(64)])      # member m of a cluster -> (dr, dg, db)


class ClusterPalette:
    """pal u32 [512]; g = cluster * 64 + member; slot_of[g], g_of[slot]"""


@functools.lru_cache(maxsize=None)
def cluster_palette():
    c = ClusterPalette()
    rng = np.random.default_rng(0xC1A5)
    c.g_of = _frozen(np.concatenate([rng.permutation(256), 256 + rng.permutation(256)]))
    c.slot_of = np.zeros(512, np.int64)
    c.slot_of[c.g_of] = np.arange(512)
    _frozen(c.slot_of)
    rgb = BASES[c.g_of >> 6] + COORDS[c.g_of & 63]
    c.pal = _frozen((rgb[:, 0] << 16 | rgb[:, 1] << 8 | rgb[:, 2]).astype(np.uint32))
    return c


def halves(pal):
    return pal[:256], pal[256:]


def rgb_of(col):
    col = np.asarray(col).astype(np.int64)
    return np.stack([(col >> 16) & 255, (col >> 8) & 255, col & 255], axis=-1)


def within2_np(a, b):
    """the predicate in numpy: all three |channel differences| <= 2 (colours a, b, broadcast)"""
    return (np.abs(rgb_of(a) - rgb_of(b)) <= 2).all(axis=-1)


def matrix_np(pal, n=512):
    """bit (a, b) of the +-2 matrix, rows and columns 0 .. n-1"""
    return within2_np(pal[:n, None], pal[None, :n])


def edge_census(da):
    """da: signed channel differences [..., 3] of compared colour pairs -> the set of (channel, sign, 2 | 3) for which a pair
    differs by exactly sign * 2 (inside) or sign * 3 (outside) on that channel with the other two inside +-2"""
    da = np.asarray(da).reshape(-1, 3)
    got = set()
    for ch in range(3):
        others = (np.abs(np.delete(da, ch, axis=1)) <= 2).all(axis=1)
        for sign in (-1, 1):
            for dist in (2, 3):
                if (others & (da[:, ch] == sign * dist)).any():
                    got.add((ch, sign, dist))
    return got


ALL_EDGES = {(ch, sign, dist) for ch in range(3) for sign in (-1, 1) for dist in (2, 3)}


# ---- planes, streams --------------------------------------------------------------------------------------------------
def plane_of_blocks(blk, w, h):
    """blk [nblk, 16] in block raster order -> plane [h, w]"""
    bw, bh = w // 4, h // 4
    return np.ascontiguousarray(np.asarray(blk).reshape(bh, bw, 4, 4).transpose(0, 2, 1, 3).reshape(h, w))


def blocks_of_plane(plane, w, h):
    return np.asarray(plane).reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3).reshape(-1, 16)


def block_lengths(flags, blk, mode512):
    """bytes of every block given its flag and its entries [nblk, 16]"""
    flags, blk = np.asarray(flags), np.asarray(blk)
    esc = ((blk & 0xFF) >= 127) if mode512 else np.zeros(blk.shape, bool)
    return np.where(flags == COPY, 1, np.where(flags == FILL, 2 + esc[:, 0], 17 + esc.sum(axis=1)))


def stream_has_flags(stream, flags, blk, mode512):
    """does the stream hold exactly these flags?  By induction over the blocks: a block whose flag is the predicted one at the
    predicted offset has the predicted length (its entries are the plane's), so the next one starts where predicted"""
    ln = block_lengths(flags, blk, mode512)
    off = np.concatenate([[0], np.cumsum(ln)])
    return off[-1] == len(stream) and bool((np.asarray(stream)[off[:-1]] == flags).all())


def walk(stream, nblk, mode512):
    """parse a frame's bytes: flags [nblk], offsets [nblk + 1], the top-left entry of every FILL block (-1 elsewhere)"""
    s = np.asarray(stream)
    flags, off, first = np.zeros(nblk, np.int64), np.zeros(nblk + 1, np.int64), np.full(nblk, -1, np.int64)
    pos = 0

    def code(pos):
        b = int(s[pos])
        if not mode512:
            return b, pos + 1
        if b & 0x7F < 127:
            return (b >> 7) << 8 | (b & 0x7F), pos + 1
        return (b >> 7) << 8 | int(s[pos + 1]), pos + 2
    for k in range(nblk):
        off[k] = pos
        flags[k] = fl = int(s[pos])
        pos += 1
        if fl == FILL:
            first[k], pos = code(pos)
        elif fl == NORMAL:
            for _ in range(16):
                _, pos = code(pos)
        else:
            assert fl == COPY, "block %d: flag %#x at %d" % (k, fl, pos - 1)
    off[nblk] = pos
    assert pos == len(s)
    return flags, off, first


class Case:
    """name, w, h, mode512, pal u32 [512], entries u16 [n, h, w], first_fc, iplane (u16 [h, w] or None: the entries of the GOP's
    I-frame when the clip starts inside a GOP), bytes: what the oracle assembles from the planes, frame by frame"""

    def __init__(self, name, w, h, mode512, pal, entries, first_fc=0, iplane=None):
        self.name, self.w, self.h, self.mode512, self.pal, self.first_fc = name, w, h, mode512, pal, first_fc
        self.entries = _frozen(np.ascontiguousarray(entries, np.uint16).reshape(-1, h, w))
        self.iplane = None if iplane is None else _frozen(np.ascontiguousarray(iplane, np.uint16).reshape(h, w))
        self.n, self.nblk = len(self.entries), (w // 4) * (h // 4)
        assert int(self.entries.max()) < (512 if mode512 else 256)
        self.bytes = [_frozen(b) for b in assemble_clip(pal, mode512, self.entries, first_fc, self.iplane)]

    def pixels(self):
        """u32 [n, h, w]: the colours of the entries"""
        return self.pal[self.entries]

    def blocks(self, f):
        return blocks_of_plane(self.entries[f], self.w, self.h)


def assemble_clip(pal, mode512, entries, first_fc=0, iplane=None):
    """orc_assemble_iframe / _pframe over a clip of entry planes [n, h, w], with the encoder's I-frame rule (frame_count % 4)"""
    p0, p1 = halves(pal)
    n, h, w = entries.shape
    out = []
    for f in range(n):
        if (first_fc + f) & 3 == 0:
            iplane = entries[f]
            out.append(O.assemble_iframe(p0, p1, mode512, w, h, entries[f]))
        else:
            assert iplane is not None
            out.append(O.assemble_pframe(p0, p1, mode512, w, h, entries[f], iplane))
    return out


def counts_np(pal, blk, iblk=None):
    """count1 [nblk] (against the top-left entry's colour) and count2 [nblk] (against the I-frame's entries; None without),
    by the numpy statement of the predicate"""
    col = pal[np.asarray(blk)]
    c1 = within2_np(col[:, :1], col).sum(axis=1)
    c2 = None if iblk is None else within2_np(col, pal[np.asarray(iblk)]).sum(axis=1)
    return c1, c2


def flags_of_counts(c1, c2):
    """COPY has priority"""
    fl = np.where(c1 >= FILL_COUNT, FILL, NORMAL)
    return fl if c2 is None else np.where(c2 >= COPY_COUNT, COPY, fl)


# ---- group 1: every escape pattern --------------------------------------------------------------------------------------
def p_pattern(k):
    return (np.asarray(k) * 40503 + 12345) & 0xFFFF


@functools.lru_cache(maxsize=None)
def escape_patterns(mode512):
    """1024 x 1024, an I- and a P-frame, every block NORMAL: block k of the I-frame has escape pattern k (bit i: the index of
    pixel i is >= 127), block k of the P-frame pattern p_pattern(k).  Pixel i takes index LO[s] or HI[s], s = (i + hash(k)) & 3
    in the I-frame and one more in the P-frame (the indices of a pixel in the two frames differ, and so do the four of a block's
    row), from the palette a hash of (k, i) names in the I-frame and from the other one in the P-frame.  The 256-colour control
    keeps the indices"""
    k, i = np.arange(65536)[:, None], np.arange(16)[None, :]
    hk = mix(k)
    pal_i = (mix(k * 16 + i + 0x51ED) >> 7) & 1
    frames = []
    for pat, s, pn in ((k, (i + hk) & 3, pal_i), (p_pattern(k), (i + hk + 1) & 3, 1 - pal_i)):
        idx = np.where((pat >> i) & 1, HI[s], LO[s])
        frames.append(plane_of_blocks(pn << 8 | idx if mode512 else idx, 1024, 1024))
    return Case("escape-patterns-%d" % (512 if mode512 else 256), 1024, 1024, mode512, lattice_palette(), np.stack(frames))


# ---- group 2: the matrix, one bit per block -------------------------------------------------------------------------------
def _foreign(cp, a, step, member_xor):
    """for entries a: an entry of another cluster of the same palette half (clusters 4h .. 4h+3)"""
    g = cp.g_of[a]
    c, m = g >> 6, g & 63
    return cp.slot_of[((c & 4) | ((c + step) & 3)) << 6 | (m ^ member_xor)]


@functools.lru_cache(maxsize=None)
def matrix_bits(mode512, pframe):
    """block (a, b), row a and column b of the block grid, probes matrix bit (a, b); n = 512 or 256 rows and columns.
    I: top-left entry a, the pixel at 1 + (a + b) % 15 holds b, two pixels entries of two other clusters, twelve more a:
       count1 = 13 + bit, FILL exactly when the bit is set.
    P: the same with three foreign pixels; the I plane holds a where the P plane holds a or b, and entries of a third cluster
       under the foreign pixels: count2 = 12 + bit and count1 = 12 + bit: COPY exactly when the bit is set, NORMAL otherwise.
       The P-frame is encoded alone, at frame_count 1, with the I plane handed over.
    Returns (case, n)"""
    cp = cluster_palette()
    n = 512 if mode512 else 256
    a, b = np.broadcast_arrays(np.arange(n)[:, None], np.arange(n)[None, :])
    blk = np.repeat(a[:, :, None], 16, axis=2)
    pos = (a + b) % 15
    put = lambda arr, off, val: np.put_along_axis(arr, (1 + (pos + off) % 15)[:, :, None], val[:, :, None], axis=2)
    put(blk, 0, b)
    put(blk, 5, _foreign(cp, a, 1, 0))
    put(blk, 10, _foreign(cp, a, 2, 63))
    iplane, fc = None, 0
    if pframe:
        put(blk, 3, _foreign(cp, a, 1, 21))
        iblk = np.repeat(a[:, :, None], 16, axis=2)
        for off in (5, 10, 3):
            put(iblk, off, _foreign(cp, a, 3, 42))
        iplane, fc = plane_of_blocks(iblk.reshape(-1, 16), 4 * n, 4 * n), 1
    name = "matrix-%s-%d" % ("P" if pframe else "I", n)
    return Case(name, 4 * n, 4 * n, mode512, cp.pal, plane_of_blocks(blk.reshape(-1, 16), 4 * n, 4 * n)[None], fc, iplane), n


# ---- group 3: the decision table on the edge of the predicate -------------------------------------------------------------
_AD = np.abs(COORDS[:, None, :] - COORDS[None, :, :])
REL = {True: _frozen(_AD.max(-1) == 2),                                            # a matching pixel: 2 on a channel, none above
       False: _frozen((_AD.max(-1) == 3) & ((_AD == 3).sum(-1) == 1))}              # a non-matching one: 3 on ONE channel, the others <= 2
EDGE_W, EDGE_H, EDGE_GOPS = 272, 64, 3
EDGE_NBLK = (EDGE_W // 4) * (EDGE_H // 4)
PAIRS9 = [(x, y) for x in KINDS for y in KINDS]
PAIRS4 = [(x, y) for x in (FILL, NORMAL) for y in (FILL, NORMAL)]
BOUNDARIES = list(range(WAVE - 1, EDGE_NBLK - 1, WAVE))        # lane 63 -> 0, 16 per frame; 511 -> 512 is also the tile boundary


def kind_of(c1, c2=0):
    return COPY if c2 >= COPY_COUNT else (FILL if c1 >= FILL_COUNT else NORMAL)


def _order_targets(targets, kinds, rng, want_pairs):
    """shuffle, then swap blocks so that the boundary after block BOUNDARIES[j] has the kinds want_pairs[j]"""
    order = rng.permutation(len(targets))
    reserved = {p for k in BOUNDARIES for p in (k, k + 1)}
    free = [p for p in rng.permutation(len(targets)) if p not in reserved]
    for k, pair in zip(BOUNDARIES, want_pairs):
        for p, want in zip((k, k + 1), pair):
            if kinds[order[p]] != want:
                t = next(t for t in free if kinds[order[t]] == want)
                free.remove(t)
                order[p], order[t] = order[t], order[p]
    return [targets[o] for o in order]


def _pick(cands, want, e_from, seed):
    """one of the candidate members; the one whose difference from member e_from is `want` = (channel, sign) if there is one"""
    ch, sign = want
    d = COORDS[cands, ch] - COORDS[e_from, ch]
    good = cands[(np.abs(d) >= 2) & (np.sign(d) == sign)]
    pool = good if len(good) else cands
    return int(pool[seed % len(pool)])


# FEASIBLE[k1][k2][e0, q]: is there a member on the edge k1 of member e0 and on the edge k2 of member q?
FEASIBLE = {k1: {k2: _frozen((REL[k1].astype(np.int64).T @ REL[k2].astype(np.int64)) > 0) for k2 in (True, False)} for k1 in (True, False)}


def _want(i, rot):
    """the (channel, sign) pixel i prefers: both rotate"""
    return (i + rot) % 3, 1 - 2 * (((i + rot) // 3) & 1)


def _position(q0, c1_i, ptargets, rng, rot, forced):
    """the I block and the three P blocks of one block position as members of one cluster, or None.  ptargets: (count1, count2)
    of the three P blocks; forced: {P block number: its top-left member}.  The top-left members come first; then every pixel's
    I-frame member is taken among those on the right edge of the I block's top-left that leave each P block a member on the right
    edges of its own top-left and of that I-frame member"""
    mi = set(rng.permutation(np.arange(1, 16))[:c1_i - 1].tolist())
    m1 = [set(rng.permutation(np.arange(1, 16))[:c1 - 1].tolist()) for c1, _ in ptargets]
    m2 = [set(rng.permutation(16)[:c2].tolist()) for _, c2 in ptargets]
    e0 = []
    for f in range(3):
        c = np.nonzero(REL[0 in m2[f]][:, q0])[0]
        if f in forced and forced[f] not in c:
            return None
        e0.append(forced[f] if f in forced else int(c[rng.integers(len(c))]))
    q, e = [q0], [[x] for x in e0]
    for i in range(1, 16):
        ok = REL[i in mi][:, q0].copy()
        for f in range(3):
            ok &= FEASIBLE[i in m1[f]][i in m2[f]][e0[f], :]
        if not ok.any():
            return None
        q.append(_pick(np.nonzero(ok)[0], _want(i, rot), q0, int(rng.integers(64))))
        for f in range(3):
            cands = np.nonzero(REL[i in m1[f]][:, e0[f]] & REL[i in m2[f]][:, q[i]])[0]
            e[f].append(_pick(cands, _want(i, rot + f + 1), q[i] if (i + f) & 1 else e0[f], int(rng.integers(64))))
    return [q] + e


@functools.lru_cache(maxsize=None)
def edge_decisions(mode512):
    """272 x 64 (1088 blocks, 3 tiles: 512, 512 and 64 blocks), EDGE_GOPS GOPs of I, P, P, P.  A P-frame holds every pair
    (count1 1 .. 16, count2 0 .. 16) four times, an I-frame every count1 68 times; every compared pixel is on the edge of the
    predicate (REL), all the colours of a block position of a GOP come from one cluster.  The blocks are shuffled and then swapped
    so that the 17 wave boundaries of a frame hold the nine (kind, next kind) pairs in rotation -- and the tile boundary
    511 -> 512 of P-frame p of the clip holds pair p: one GOP has three P-frames, nine pairs take three GOPs.  FILL blocks take
    their top-left entries from SPECIAL x the palettes, as far as the block position's cluster is still free.
    Returns (case, targets): targets[f][k] = (count1, count2 or None) as built"""
    cp = cluster_palette()
    nclu = 8 if mode512 else 4
    specials = [pn << 8 | ix for pn in range(2 if mode512 else 1) for ix in SPECIAL]
    rng = np.random.default_rng(0xED6E + mode512)
    planes, targets = [], []
    for gop in range(EDGE_GOPS):
        it = [(c1, None) for c1 in range(1, 17)] * (EDGE_NBLK // 16)
        tg = [_order_targets(it, [kind_of(c1) for c1, _ in it], rng, [PAIRS4[(j + gop) % 4] for j in range(len(BOUNDARIES))])]
        for p in range(3):
            pt = [(c1, c2) for c1 in range(1, 17) for c2 in range(17)] * 4
            pn = 3 * gop + p                                   # P-frame number in the clip
            want = [PAIRS9[pn] if k == ENC_T - 1 else PAIRS9[(j + 2 * pn + 1) % 9] for j, k in enumerate(BOUNDARIES)]
            tg.append(_order_targets(pt, [kind_of(c1, c2) for c1, c2 in pt], rng, want))
        # which block positions have a FILL block with a SPECIAL top-left entry, and in which frame of the GOP
        claim = {}
        for f in range(4):
            todo = specials * 2
            for k in range(EDGE_NBLK):
                if todo and k not in claim and kind_of(tg[f][k][0], tg[f][k][1] or 0) == FILL:
                    claim[k] = (f, todo.pop(0))
        blk = np.zeros((4, EDGE_NBLK, 16), np.int64)
        for k in range(EDGE_NBLK):
            cf, cslot = claim.get(k, (None, None))
            clu = int(mix(k + 1088 * gop) % nclu) if cslot is None else int(cp.g_of[cslot] >> 6)
            forced = None if cslot is None else int(cp.g_of[cslot] & 63)
            for attempt in range(256):
                r = np.random.default_rng([0xB10C, mode512, gop, k, attempt])
                if cf == 0:
                    q0 = forced
                elif cf is not None:                           # the I block's top-left must suit the P block's forced one
                    c = np.nonzero(REL[bool(r.integers(2))][:, forced])[0]
                    q0 = int(c[r.integers(len(c))])
                else:
                    q0 = int(r.integers(64))
                members = _position(q0, tg[0][k][0], [tg[f][k] for f in (1, 2, 3)], r, k + attempt, {cf - 1: forced} if cf else {})
                if members is not None:
                    break
            else:
                raise AssertionError("no blocks for position %d of GOP %d" % (k, gop))
            blk[:, k, :] = cp.slot_of[clu * 64 + np.array(members)]
        planes += [plane_of_blocks(b, EDGE_W, EDGE_H) for b in blk]
        targets += tg
    return Case("edge-decisions-%d" % (512 if mode512 else 256), EDGE_W, EDGE_H, mode512, cp.pal, np.stack(planes)), targets


# ---- group 4: waves of one to three bytes ---------------------------------------------------------------------------------
TAIL_SHAPES = [(20, 52), (8, 132), (268, 4), (2052, 4), (8, 1028), (20, 412)]       # 65, 66, 67, 513, 514, 515 blocks
TAIL_GOPS = 4
TAIL_STRIDE_EXTRA = (0, 1)                                     # out_stride = agmv_hip_max_usize + extra
# last waves by their blocks' lengths (P-frames): one block 1, 2 or 3 bytes; two blocks; three COPY
TAIL_COMBOS = {1: [(1,), (2,), (3,)], 2: [(1, 1), (1, 2), (2, 1)], 3: [(1, 1, 1)]}


def hip_max_usize(w, h, mode512):
    """agmv_hip_max_usize: 33 or 17 bytes per block and 64, rounded up to 256"""
    return ((w // 4) * (h // 4) * (33 if mode512 else 17) + 64 + 255) & ~255


def _fill_entry(length, seed, avoid):
    """an entry whose FILL block has `length` bytes (2: index < 127, 3: >= 127) and differs from every entry in `avoid`"""
    for t in range(8):
        e = int((seed + t) >> 2 & 1) << 8 | int((HI if length == 3 else LO)[(seed + t) & 3])
        if e not in avoid:
            return e
    raise AssertionError


@functools.lru_cache(maxsize=None)
def short_tails(shape, stride_extra):
    """lattice palette, 512 colours, TAIL_GOPS GOPs.  Every block is flat (one entry): FILL, or COPY in a P-frame where it
    repeats the I-frame's block.  The r = nblk % 64 blocks of the last wave have the lengths of a TAIL_COMBO; the blocks before
    them are a hashed mix of COPY, 2- and 3-byte FILL whose first two are then chosen so that the last wave's destination
    (frame * out_stride + bytes before it) has the residue mod 4 the frame is to have.  I-frames: the last wave of one block
    is a 2- or 3-byte FILL; with two or three blocks an I-frame's last wave has four bytes or more"""
    w, h = shape
    nblk = (w // 4) * (h // 4)
    r, pre = nblk % WAVE, nblk - nblk % WAVE
    stride = hip_max_usize(w, h, True) + stride_extra
    combos = TAIL_COMBOS[r]
    ent = np.zeros((4 * TAIL_GOPS, nblk), np.int64)
    plan = []
    for f in range(4 * TAIL_GOPS):
        g, p = f >> 2, f & 3
        if p == 0:                                             # the two shapes with r == 1 together: (2 | 3 bytes) x (residue 0 .. 3)
            lens, res, iblk = [2 + ((g + (nblk > ENC_T) + j) & 1) for j in range(r)], g, None
        else:                                                  # P-frame q of the clip: every combination x every residue
            q = 3 * g + p - 1
            lens, res, iblk = list(combos[q % len(combos)]), q // len(combos) % 4, ent[f - p]
        shortest = 2 if p == 0 else 1
        hh = mix(np.arange(pre) + 977 * f + 31 * nblk) >> 3
        pl = [int(x) for x in hh % (4 - shortest) + shortest]  # lengths of the blocks before the last wave
        head = next(t for t in np.ndindex(4, 4, 4) if min(t) >= shortest and (f * stride + sum(t) + sum(pl[3:])) % 4 == res)
        pl[:3] = head                                          # ... the first three make the residue
        for k, ln in enumerate(pl + lens):
            ent[f, k] = iblk[k] if ln == 1 else _fill_entry(ln, int(mix(k + 4099 * f) >> 5), () if iblk is None else (int(iblk[k]),))
        plan.append((sum(lens), res))
    c = Case("short-tails-%dx%d+%d" % (w, h, stride_extra), w, h, True, lattice_palette(),
             np.stack([plane_of_blocks(np.repeat(e[:, None], 16, axis=1), w, h) for e in ent]))
    c.stride, c.plan = stride, plan
    return c


def tail_census(c):
    """from the oracle's bytes: per frame (is I-frame, bytes of the last wave, destination of the last wave mod 4)"""
    out = []
    for f in range(c.n):
        _, off, _ = walk(c.bytes[f], c.nblk, True)
        base = int(off[c.nblk - c.nblk % WAVE])
        out.append((f & 3 == 0, len(c.bytes[f]) - base, (f * c.stride + base) & 3))
    return out


# ---- group 5: a frame at its maximum --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def full_frames(shape):
    """an I- and a P-frame, every block NORMAL with 16 escapes: 16 different indices >= 127 per block, the P-frame's from the
    other palette"""
    w, h = shape
    nblk = (w // 4) * (h // 4)
    k, i = np.arange(nblk)[:, None], np.arange(16)[None, :]
    idx = 127 + (mix(k) + 37 * i) % 129
    pn = (mix(k * 16 + i + 0xF011) >> 9) & 1
    planes = [plane_of_blocks(pn << 8 | idx, w, h), plane_of_blocks((1 - pn) << 8 | (127 + (mix(k + 7) + 37 * i) % 129), w, h)]
    return Case("full-%dx%d" % (w, h), w, h, True, lattice_palette(), np.stack(planes))


# ---- group 6: the exported predicate --------------------------------------------------------------------------------------
PRED_BASES = (0x000000, 0xFFFFFF, 0x808080)


@functools.lru_cache(maxsize=None)
def predicate_calls():
    """a [calls, 16], b [calls, 16] u32: around each base the 729 differences in [-4, 4]^3 (clipped to valid colours), 16 pairs
    per call (the last call of a base repeats its last pair), then per base and per n = 0 .. 16 a call with n pairs at exactly
    2 on a channel and 16 - n at exactly 3"""
    d = np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    a, b = [], []
    pack = lambda rgb: (rgb[:, 0] << 16 | rgb[:, 1] << 8 | rgb[:, 2]).astype(np.uint32)
    for base in PRED_BASES:
        other = pack(np.clip(rgb_of(base)[None, :] + d, 0, 255))
        other = np.concatenate([other, np.repeat(other[-1:], -len(other) % 16)])
        b.append(other.reshape(-1, 16))
        inward = np.where(rgb_of(base) >= 128, -1, 1)           # a direction that stays inside [0, 255]
        for n in range(17):
            dd = np.zeros((16, 3), np.int64)
            for j in range(16):
                dd[j, (j + n) % 3] = inward[(j + n) % 3] * (2 if (j * 7 + n) % 16 < n else 3)
            b.append(pack(rgb_of(base)[None, :] + dd)[None, :])
        a.append(np.full((len(other) // 16 + 17, 16), base, np.uint32))
    return _frozen(np.concatenate(a)), _frozen(np.concatenate(b))
