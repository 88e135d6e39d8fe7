"""The crafted cases of tests/encode_table_cases.py proved on the CPU: each census below is what a group of
tests/test_gpu_encode_table.py claims to reach, asserted against the oracle's own bytes, entries and block counts."""
import numpy as np
import pytest

import encode_table_cases as TC
import oracles as O

MODES = pytest.mark.parametrize("mode512", [True, False], ids=["m512", "m256"])


def oracle_entries_and_bytes(c):
    """the clip's PIXELS through OracleEncoder: the entries it finds must be the plane's, its bytes those assembled from the plane"""
    enc = O.OracleEncoder(c.w, c.h, c.mode512, *TC.halves(c.pal), first_frame_count=c.first_fc & ~3)
    if c.first_fc & 3:
        enc.encode(c.pal[c.iplane])
        for _ in range((c.first_fc & 3) - 1):
            enc.encode(c.pal[c.iplane])
    for f, pix in enumerate(c.pixels()):
        b, e = enc.encode(pix, want_entries=True)
        assert (e.reshape(c.h, c.w) == c.entries[f]).all(), "%s: frame %d does not quantise back to its entries" % (c.name, f)
        assert len(b) == len(c.bytes[f]) and (b == c.bytes[f]).all(), "%s: frame %d" % (c.name, f)
    enc.close()


# ---- palettes -----------------------------------------------------------------------------------------------------------
def test_lattice_palette_matches_only_itself():
    pal = TC.lattice_palette()
    assert len(np.unique(pal)) == 512 and len(np.unique(pal[:256])) == 256
    d = np.abs(TC.rgb_of(pal[:, None]) - TC.rgb_of(pal[None, :])).max(axis=-1)
    assert (d[~np.eye(512, dtype=bool)] >= 8).all()
    assert (TC.matrix_np(pal) == np.eye(512, dtype=bool)).all()


def test_cluster_palette_has_every_edge_inside_every_cluster():
    cp = TC.cluster_palette()
    assert len(np.unique(cp.pal)) == 512 and (cp.g_of[cp.slot_of] == np.arange(512)).all()
    assert sorted(set((cp.g_of[:256] >> 6).tolist())) == [0, 1, 2, 3], "palette 0 holds whole clusters"
    rgb = TC.rgb_of(cp.pal)
    clu = cp.g_of >> 6
    d = rgb[:, None, :] - rgb[None, :, :]
    across = clu[:, None] != clu[None, :]
    assert (np.abs(d).max(axis=-1)[across] >= 40).all()
    assert (np.abs(TC.BASES[:, None] - TC.BASES[None, :]).max(axis=-1)[~np.eye(8, dtype=bool)] >= 40).all()
    for c in range(8):
        inside = d[np.ix_(clu == c, clu == c)]
        assert set(np.unique(inside).tolist()) == {0, 1, 2, 3, 5, -1, -2, -3, -5}
        assert TC.edge_census(inside) == TC.ALL_EDGES
    spread = np.diff(np.sort(np.nonzero(clu == 0)[0]))
    assert (spread > 1).sum() > 16, "a cluster is spread over its palette, not a run of slots"


# ---- group 1 --------------------------------------------------------------------------------------------------------------
@MODES
def test_escape_patterns_are_complete_and_every_block_is_normal(mode512):
    c = TC.escape_patterns(mode512)
    oracle_entries_and_bytes(c)
    for f, pat_of in enumerate((lambda k: k, TC.p_pattern)):
        blk = c.blocks(f)
        assert TC.stream_has_flags(c.bytes[f], np.full(c.nblk, TC.NORMAL), blk, mode512), "frame %d: a block that is not NORMAL" % f
        if mode512:
            pat = (((blk & 0xFF) >= 127) << np.arange(16)).sum(axis=1)
            assert (pat == pat_of(np.arange(65536))).all()
            assert len(np.unique(pat)) == 65536, "every escape pattern once"
            assert len(c.bytes[f]) == 65536 * 25 == 1638400
            assert set(np.unique(blk & 0xFF).tolist()) == set(TC.LO.tolist() + TC.HI.tolist()) and set(np.unique(blk >> 8).tolist()) == {0, 1}
        else:
            assert len(c.bytes[f]) == 65536 * 17 and int(blk.max()) < 256
    if mode512:
        pi, pp = np.arange(65536), TC.p_pattern(np.arange(65536))
        assert sorted(pp.tolist()) == pi.tolist() and (pi % 64 != pp % 64).sum() > 60000, "pattern and lane are not tied together"
        assert ((c.entries[0] ^ c.entries[1]) >> 8 == 1).all(), "the P-frame's palette number is the complement"


# ---- group 2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pframe", [False, True], ids=["I", "P"])
@MODES
def test_matrix_blocks_turn_on_their_bit(mode512, pframe):
    c, n = TC.matrix_bits(mode512, pframe)
    cp = TC.cluster_palette()
    M = TC.matrix_np(cp.pal, n)
    assert (c.w, c.h, c.nblk) == (4 * n, 4 * n, n * n) and 2 * c.entries.nbytes <= 16 << 20
    blk = c.blocks(0)
    a, b = np.divmod(np.arange(n * n), n)
    assert (blk[:, 0] == a).all() and (blk[np.arange(n * n), 1 + (a + b) % 15] == b).all()
    iblk = TC.blocks_of_plane(c.iplane, c.w, c.h) if pframe else None
    c1, c2 = TC.counts_np(cp.pal, blk, iblk)
    if pframe:
        assert (iblk[np.arange(n * n), 1 + (a + b) % 15] == a).all(), "the probed pixel: row a (the I-frame's entry), column b"
        assert (c2 == 12 + M.reshape(-1)).all() and (c1 == 12 + M.reshape(-1)).all() and (c1 < TC.FILL_COUNT).all()
        flags = np.where(M.reshape(-1), TC.COPY, TC.NORMAL)
    else:
        assert (c1 == 13 + M.reshape(-1)).all()
        flags = np.where(M.reshape(-1), TC.FILL, TC.NORMAL)
    assert TC.stream_has_flags(c.bytes[0], flags, blk, mode512), "the numpy matrix does not predict the oracle's flags"
    moved = 1 + (a + b) % 15
    assert all(len(np.unique(moved[a == r])) == 15 for r in (0, 1, n - 1)), "the probed pixel takes every position in a row"
    clu = cp.g_of[:n] >> 6
    for k in np.unique(clu):
        inside = M[np.ix_(clu == k, clu == k)]
        assert inside.any() and not inside.all(), "cluster %d: both flag values" % k
        assert not M[np.ix_(clu == k, clu != k)].any()
    d = TC.rgb_of(cp.pal[:n, None]) - TC.rgb_of(cp.pal[None, :n])
    assert TC.edge_census(d) == TC.ALL_EDGES, "12 of 12 signed edges among the probed pairs"
    inside2 = (np.abs(d).max(axis=-1) == 2)
    assert M[inside2].all() and not M[np.abs(d).max(axis=-1) == 3].any()
    # every word and every bit position of a row is probed both ways
    words = M.reshape(n, n // 32, 32)
    assert words.any(axis=(0, 1)).all() and words.any(axis=(0, 2)).all() and (~words).any(axis=(0, 1)).all()


@pytest.mark.parametrize("pframe", [False, True], ids=["I", "P"])
def test_matrix_cases_through_the_stateful_encoder(pframe):
    """256 colours, 1024 x 1024: the case as pixels through OracleEncoder (for P: the I plane's pixels first) quantises back to
    its entries and gives the same bytes.  The 2048 x 2048 cases of the 512-colour mode stand on the same palette -- 512 distinct
    colours -- and are left out for their 2 x 10^9 distance computations per plane"""
    c, _ = TC.matrix_bits(False, pframe)
    oracle_entries_and_bytes(c)


# ---- group 3 --------------------------------------------------------------------------------------------------------------
@MODES
def test_edge_decisions_census(mode512):
    c, targets = TC.edge_decisions(mode512)
    cp = TC.cluster_palette()
    oracle_entries_and_bytes(c)
    assert c.n == 4 * TC.EDGE_GOPS and c.nblk == 1088 and len(TC.BOUNDARIES) == 16 and TC.ENC_T - 1 in TC.BOUNDARIES
    at_wave, at_tile = set(), set()
    fill_first = {True: set(), False: set()}
    edges1, edges2 = {True: [], False: []}, []
    for f in range(c.n):
        is_i = f & 3 == 0
        blk = c.blocks(f)
        iblk = None if is_i else c.blocks(f & ~3)
        c1, c2 = TC.counts_np(cp.pal, blk, iblk)
        assert (c1 == [t[0] for t in targets[f]]).all(), "frame %d: count1 as built" % f
        census = sorted(zip(c1.tolist(), [0] * c.nblk if is_i else c2.tolist()))
        if is_i:
            assert census == sorted((k, 0) for k in range(1, 17) for _ in range(68))
        else:
            assert (c2 == [t[1] for t in targets[f]]).all(), "frame %d: count2 as built" % f
            assert census == sorted((k, m) for k in range(1, 17) for m in range(17) for _ in range(4)), "every pair four times"
        want = TC.flags_of_counts(c1, c2)
        flags, _, first = TC.walk(c.bytes[f], c.nblk, mode512)
        assert (flags == want).all(), "frame %d: the counts dictate the flags, COPY first" % f
        fill_first[is_i] |= set(first[flags == TC.FILL].tolist())
        for k in TC.BOUNDARIES:
            at_wave.add((flags[k], flags[k + 1]))
            if k == TC.ENC_T - 1:
                at_tile.add((flags[k], flags[k + 1]))
        # the edge rule: against the top-left colour (but for the top-left pixel itself) and against the I-frame's entry
        rgb = TC.rgb_of(cp.pal[blk])
        d1 = rgb[:, 1:, :] - rgb[:, :1, :]
        m1 = np.abs(d1).max(axis=-1)
        assert ((m1 == 2) | ((m1 == 3) & ((np.abs(d1) == 3).sum(axis=-1) == 1))).all(), "frame %d: a pixel off the edge (count1)" % f
        edges1[is_i].append(d1)
        if not is_i:
            d2 = rgb - TC.rgb_of(cp.pal[iblk])
            m2 = np.abs(d2).max(axis=-1)
            assert ((m2 == 2) | ((m2 == 3) & ((np.abs(d2) == 3).sum(axis=-1) == 1))).all(), "frame %d: a pixel off the edge (count2)" % f
            edges2.append(d2)
    assert at_wave == set(TC.PAIRS9) and at_tile == set(TC.PAIRS9), "every (kind, next kind) at a wave boundary and at 511 -> 512"
    specials = {pn << 8 | ix for pn in range(2 if mode512 else 1) for ix in TC.SPECIAL}
    assert specials <= fill_first[True] and specials <= fill_first[False], "FILL top-left entries in I- and in P-frames"
    for e in (edges1[True], edges1[False], edges2):
        assert TC.edge_census(np.concatenate([x.reshape(-1, 3) for x in e])) == TC.ALL_EDGES
    # the four placings of a pair in a P-frame: at least three different sets of matching pixels
    blk, iblk = c.blocks(1), c.blocks(0)
    col = cp.pal[blk]
    masks = {}
    for k, t in enumerate(targets[1]):
        masks.setdefault(t, set()).add((tuple(TC.within2_np(col[k, :1], col[k]).tolist()), tuple(TC.within2_np(col[k], cp.pal[iblk[k]]).tolist())))
    assert all(len(v) >= 3 for t, v in masks.items() if 2 <= t[0] <= 15 or 1 <= t[1] <= 15)


# ---- group 4 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", TC.TAIL_STRIDE_EXTRA)
def test_short_tails_reach_every_total_and_alignment(extra):
    seen = {True: set(), False: set()}
    kinds = set()
    for shape in TC.TAIL_SHAPES:
        c = TC.short_tails(shape, extra)
        r = c.nblk % TC.WAVE
        assert r in (1, 2, 3) and c.nblk // TC.WAVE in (1, 8) and c.n == 4 * TC.TAIL_GOPS
        assert c.stride == TC.hip_max_usize(c.w, c.h, True) + extra and c.stride >= O.max_usize(c.w, c.h)
        oracle_entries_and_bytes(c)
        for f, (is_i, total, res) in enumerate(TC.tail_census(c)):
            assert (total, res) == c.plan[f], "%s frame %d" % (c.name, f)
            if total <= 3:
                seen[is_i].add((total, res))
            flags, off, _ = TC.walk(c.bytes[f], c.nblk, True)
            assert set(flags.tolist()) <= ({TC.FILL} if is_i else {TC.COPY, TC.FILL})
            kinds |= set(np.diff(off)[:c.nblk - r].tolist())
            assert len(c.bytes[f]) < c.stride
    assert seen[False] == {(t, a) for t in (1, 2, 3) for a in range(4)}, "P-frames: 12 of 12"
    assert seen[True] == {(t, a) for t in (2, 3) for a in range(4)}, "I-frames: 8 of 8"
    assert kinds == {1, 2, 3}


# ---- group 5 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2052, 4), (300, 40)], ids=lambda s: "%dx%d" % s)
def test_full_frames_are_at_the_maximum(shape):
    c = TC.full_frames(shape)
    oracle_entries_and_bytes(c)
    for f in range(2):
        assert len(c.bytes[f]) == 33 * c.nblk == O.max_usize(c.w, c.h) - 64 <= TC.hip_max_usize(c.w, c.h, True) - 64
        assert TC.stream_has_flags(c.bytes[f], np.full(c.nblk, TC.NORMAL), c.blocks(f), True)
        assert ((c.blocks(f) & 0xFF) >= 127).all()
    assert len(TC.full_frames((2052, 4)).bytes[0]) == 16929


# ---- group 6 --------------------------------------------------------------------------------------------------------------
def test_predicate_calls_against_the_oracle():
    a, b = TC.predicate_calls()
    want = TC.within2_np(a, b).sum(axis=1)
    assert a.shape == b.shape == (3 * (46 + 17), 16)
    for base, lo in zip(TC.PRED_BASES, range(0, len(a), 63)):
        assert (a[lo:lo + 63] == base).all()
        assert want[lo + 46:lo + 63].tolist() == list(range(17)), "every count 0 .. 16"
        d = TC.rgb_of(b[lo:lo + 46]) - TC.rgb_of(base)
        if base == 0x808080:
            assert len({tuple(x) for x in d.reshape(-1, 3).tolist()}) == 729 and TC.edge_census(d) == TC.ALL_EDGES
    ent, ient = np.arange(16, dtype=np.uint16), np.arange(16, dtype=np.uint16) | 0x100
    for k in range(len(a)):
        p0, p1 = np.zeros(256, np.uint32), np.zeros(256, np.uint32)
        p0[:16], p1[:16] = b[k], a[k]
        assert O.compare_pframe_block(p0, p1, 4, 0, 0, ent, ient) == want[k], k
        assert O.compare_iframe_block(p0, p1, 4, 0, 0, int(a[k, 0]), ent) == want[k], k
