"""k_encode as ONE software pipeline per workgroup that runs across tile switches (agmv_hip.hip): a workgroup that takes many
tiles one after the other -- tickets handed over through LDS slots, the cursors `cur` and `pf` crossing tile boundaries, eight
recycled control slots with 16-bit tags, geometry and load path recomputed at every switch, I-frame entries taken from the
caller's plane away from item 0 -- must give the oracle's bytes.  On an MI355X the default grid is 512 workgroups, so at a
small shape a workgroup runs one tile, or the few it draws before the others have started: which, is a matter of timing.
AGMV_ENC_GRID=n caps the grid, and every workgroup runs total_tiles / n of them (tests/encode_cases.py builds the clips):

  a  the cap is honoured (the grid encode_dev reports with AGMV_HIP_DEBUG), and values that are no cap change nothing
  b  grids 1, 2, 3, 8 on five ragged shapes, both modes, the 27 adversarial frames
  c  batches that start inside a GOP (phases 1, 2, 3), the entry plane handed from call to call
  d  the ENTRIES variant
  e  the default grid with at least eight tiles per workgroup: the periodic clip with marker GOPs, every frame compared
  g  one GOP of 68 tiles: chains of unfinished aggregates in the look-back
  h  1080p: capped grids equal the default one
  f  one workgroup past 65 536 items: the 16-bit tags wrap (0.2 s at 8x8 and 0.5 s at 2052x4 on an MI355X, clip and comparison included)

Expected bytes come from OracleEncoder, never from the GPU, except in h."""
import re

import numpy as np
import pytest

import encode_cases as EC
import oracles as O
import synth as S

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (68, 36), (2052, 4), (300, 40), (516, 64)]   # tiles per frame 1, 1, 2 (the second: one block), 2, 5 (the last: 16 blocks)
GRIDS = [1, 2, 3, 8]
ids_shape = lambda s: "%dx%d" % s


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    return torch


@pytest.fixture(scope="module")
def hip(torch):
    from libagmv_amd import AgmvHip
    h = AgmvHip(0)
    yield h
    h.close()


def set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("AGMV_ENC_GRID", raising=False)
    else:
        monkeypatch.setenv("AGMV_ENC_GRID", str(grid))


def dev_i32(torch, a):
    return torch.from_numpy(np.array(a, np.uint32).view(np.int32)).cuda()       # (a copy: the cached clips are read-only)


def encode(torch, hip, frames, first_fc=0, ientries=None):
    """frames: uint32 [n, h, w] on the host -> the bytes of every frame"""
    n, h, w = frames.shape
    out, sizes = hip.encode_dev(dev_i32(torch, frames), n, w, h, first_fc, ientries=ientries)
    hip.check()
    sizes, out = sizes.cpu().numpy(), out.cpu().numpy()
    return [out[i, :sizes[i]] for i in range(n)]


def assert_same(got, exp, what):
    assert len(got) == len(exp), what
    for t in range(len(exp)):
        n = min(len(got[t]), len(exp[t]))
        d = np.nonzero(got[t][:n] != exp[t][:n])[0]
        assert len(got[t]) == len(exp[t]) and d.size == 0, "%s: frame %d has %d bytes for %d, first difference at %s" % (
            what, t, len(got[t]), len(exp[t]), d[0] if d.size else n)


# ---- a ------------------------------------------------------------------------------------------------------------------
def test_cap_is_honoured(torch, monkeypatch, capfd):
    """300x40, 27 frames: 7 GOPs x 2 tiles.  The grid is read from the line encode_dev writes per launch under AGMV_HIP_DEBUG;
    the resident count from the line agmv_hip_create writes"""
    from libagmv_amd import AgmvHip
    c = EC.oracle_clip(300, 40, True)
    monkeypatch.setenv("AGMV_HIP_DEBUG", "1")
    monkeypatch.delenv("AGMV_ENC_GRID", raising=False)
    capfd.readouterr()
    h = AgmvHip(0)
    try:
        m = re.search(r"k_encode: (\d+) workgroup\(s\) of \d+ lanes resident per CU \(\d+ B of LDS each\), (\d+) CUs", capfd.readouterr().err)
        assert m, "no line from agmv_hip_create"
        resident = int(m.group(1)) * int(m.group(2))
        assert resident >= 1
        h.set_palette(*c.pal, True)
        for cap, want in ((None, min(resident, 14)), ("1", 1), ("3", 3), ("0", min(resident, 14)), ("-2", min(resident, 14)),
                          ("x", min(resident, 14)), ("1000000000", min(resident, 14)), ("14", min(resident, 14))):
            set_grid(monkeypatch, cap)
            capfd.readouterr()
            got = encode(torch, h, c.frames)
            lines = re.findall(r"k_encode: grid of (\d+) workgroup\(s\) for (\d+) tile\(s\)", capfd.readouterr().err)
            assert lines == [(str(want), "14")], "AGMV_ENC_GRID=%s: %s" % (cap, lines)
            assert_same(got, c.bytes, "AGMV_ENC_GRID=%s" % cap)
    finally:
        h.close()


# ---- b ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("mode512", [True, False], ids=["m512", "m256"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids_shape)
def test_capped_grids_vs_oracle(torch, hip, monkeypatch, shape, mode512, grid):
    c = EC.oracle_clip(shape[0], shape[1], mode512)
    set_grid(monkeypatch, grid)
    hip.set_palette(*c.pal, mode512)
    assert_same(encode(torch, hip, c.frames), c.bytes, "grid %d" % grid)


# ---- c ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("split", [(5, 9, 13), (3, 8, 16)], ids=["5+9+13", "3+8+16"])
@pytest.mark.parametrize("mode512", [True, False], ids=["m512", "m256"])
@pytest.mark.parametrize("shape", [(2052, 4), (300, 40)], ids=ids_shape)
def test_batches_inside_a_gop_capped(torch, hip, monkeypatch, shape, mode512, split, grid):
    """first_fc 5 and 14 (phases 1, 2), 3 and 11 (phase 3).  Tickets are tile-major, so with one or two workgroups GOP 0 of
    tile 1 comes to a workgroup that has run other tiles: the I-frame entries of the caller's plane are loaded at a tile
    switch, and a batch that also holds an I-frame writes the new plane to scratch first (ient_both)"""
    w, h = shape
    c = EC.oracle_clip(w, h, mode512)
    set_grid(monkeypatch, grid)
    hip.set_palette(*c.pal, mode512)
    ient = torch.zeros(w * h, dtype=torch.int16, device="cuda")
    fc = 0
    for n in split:
        got = encode(torch, hip, c.frames[fc:fc + n], first_fc=fc, ientries=ient)
        assert_same(got, c.bytes[fc:fc + n], "batch of %d from %d" % (n, fc))
        last_i = (fc + n - 1) & ~3
        assert last_i >= fc, "every batch of the splits holds an I-frame"
        assert (ient.cpu().numpy().view(np.uint16) == c.entries[last_i]).all(), "entry plane after the batch of %d from %d" % (n, fc)
        fc += n
    assert fc == c.n


# ---- d ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("mode512", [True, False], ids=["m512", "m256"])
def test_entries_variant_capped(hip, monkeypatch, mode512, grid):
    w, h = 300, 40
    c = EC.oracle_clip(w, h, mode512)
    set_grid(monkeypatch, grid)
    hip.set_palette(*c.pal, mode512)
    got = hip.encode_entries_host(c.entries.astype(np.uint32).reshape(c.n, h, w))
    hip.check()
    assert_same(got, c.bytes, "entries, grid %d" % grid)


# ---- e, f: the periodic clip ----------------------------------------------------------------------------------------------
def run_periodic(torch, hip, w, h, mode512, n_frames, marker_groups, twice):
    hip.set_palette(*EC.oracle_clip(w, h, mode512, EC.P).pal, mode512)
    p = EC.Periodic(w, h, mode512, n_frames, marker_groups, stride=hip.max_usize(w, h))     # (the stride is the palette mode's)
    pix = p.pixels(torch, "cuda")
    rows, row_sizes, row_of = torch.from_numpy(p.rows).cuda(), torch.from_numpy(p.row_sizes).cuda(), torch.from_numpy(p.row_of).cuda()
    out, sizes = hip.encode_dev(pix, n_frames, w, h)
    hip.check()
    bad = EC.mismatched_frames(torch, out, sizes, rows, row_sizes, row_of)
    assert not bad, "%d of %d frames differ from the oracle: %s" % (len(bad), n_frames, bad[:16])
    if twice:
        out2, sizes2 = hip.encode_dev(pix, n_frames, w, h)
        hip.check()
        assert torch.equal(sizes, sizes2)
        bad = EC.mismatched_frames(torch, out2, sizes2, out, sizes, torch.arange(n_frames, device="cuda"))
        assert not bad, "second run: frames %s differ from the first" % bad[:16]


@pytest.mark.parametrize("shape,mode512", [((68, 36), True), ((300, 40), True), ((300, 40), False)], ids=["68x36-m512", "300x40-m512", "300x40-m256"])
def test_default_grid_many_tiles_per_workgroup(torch, hip, monkeypatch, shape, mode512):
    """total_tiles >= 16 x CUs and at most two workgroups (69 KB of LDS) per CU: every workgroup runs at least eight tiles.
    Markers on groups 0, 1, the middle, the last but one and the last (three frames)"""
    set_grid(monkeypatch, None)
    w, h = shape
    tpf = EC.tiles_per_frame(w, h)
    want = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    ng = (want + tpf - 1) // tpf
    assert ng * tpf >= want and ng >= 8
    run_periodic(torch, hip, w, h, mode512, 4 * ng - 1, [0, 1, ng // 2, ng - 2, ng - 1], twice=True)


# ---- g ------------------------------------------------------------------------------------------------------------------
_one_gop = {}


def one_gop_clip():
    """2048x272: 34 816 blocks, 68 tiles.  Noise (every block NORMAL with escapes), flat (FILL), synthetic, and a frame of three
    bands of them, so that the tiles of one frame differ in size by a factor of ten"""
    if not _one_gop:
        w, h = 2048, 272
        rng = np.random.default_rng(2048272)
        noise = rng.integers(0, 1 << 24, size=(h, w), dtype=np.uint32)
        synth = S.synth_frame(w, h, 1)
        flat = np.full((h, w), 0x808181, np.uint32)
        bands = np.concatenate([noise[:92], flat[92:180], synth[180:]])
        frames = np.stack([bands, flat, noise, synth])
        pal = S.content_palettes(frames[2:])
        enc = O.OracleEncoder(w, h, True, *pal)
        _one_gop.update(frames=frames, pal=pal, bytes=[enc.encode(f) for f in frames])
        enc.close()
    return _one_gop


@pytest.mark.parametrize("n_frames", [4, 1])
@pytest.mark.parametrize("grid", [None, 2, 67])
def test_one_gop_of_68_tiles(torch, hip, monkeypatch, grid, n_frames):
    """n_groups == 1: consecutive tickets are consecutive tiles of the same frames, so a look-back meets predecessors that are
    still running.  With more than 65 tiles it CAN go on to its second window of 64 status words; whether it does depends on
    timing (it needs a chain of 64 unfinished aggregates) and cannot be asserted here -- what is asserted is every byte"""
    c = one_gop_clip()
    set_grid(monkeypatch, grid)
    hip.set_palette(*c["pal"], True)
    assert EC.tiles_per_frame(2048, 272) == 68 and EC.n_groups(n_frames) == 1
    assert_same(encode(torch, hip, c["frames"][:n_frames]), c["bytes"][:n_frames], "grid %s, %d frame(s)" % (grid, n_frames))


# ---- h ------------------------------------------------------------------------------------------------------------------
def test_capped_equals_default_at_1080p(torch, hip, monkeypatch):
    """8 synthetic frames, 254 tiles each (waves inside one block row, across one boundary, past the frame's end); frames 0 and 1
    of the default grid's output are pinned to the oracle by test_encode_1080p_vs_oracle"""
    w, h, n = 1920, 1080, 8
    frames = hip.synth_dev(w, h, 0, n)
    hip.set_palette(*S.content_palettes([S.synth_frame(w, h, t) for t in range(2)]), True)
    set_grid(monkeypatch, None)
    ref, ref_sizes = hip.encode_dev(frames, n, w, h)
    hip.check()
    assert int(ref_sizes.min()) > 0
    every = torch.arange(n, device="cuda")
    for grid in (1, 5, 64):
        set_grid(monkeypatch, grid)
        out, sizes = hip.encode_dev(frames, n, w, h)
        hip.check()
        assert torch.equal(sizes, ref_sizes), "grid %d" % grid
        bad = EC.mismatched_frames(torch, out, sizes, ref, ref_sizes, every)
        assert not bad, "grid %d: frames %s differ from the default grid's" % (grid, bad)


# ---- f ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n_frames", [((8, 8), 66002), ((2052, 4), 33202)], ids=["8x8", "2052x4"])
def test_item_counter_past_65536_in_one_workgroup(torch, hip, monkeypatch, shape, n_frames):
    """grid 1: the tags (it + 1) & 0xffff of the control slots wrap at item 65 535.  8x8: one tile, no look-back.  2052x4: two
    tiles, 66 404 items, a look-back on every item of tile 1 -- nothing smaller reaches the wrap with a look-back, since the
    case is one workgroup's.  Markers on the groups that hold items 65 534 .. 65 537, on the first and on the last group"""
    set_grid(monkeypatch, 1)
    w, h = shape
    tpf = EC.tiles_per_frame(w, h)
    assert n_frames * tpf > 65537
    run_periodic(torch, hip, w, h, True, n_frames, EC.wrap_marker_groups(n_frames, tpf), twice=False)
