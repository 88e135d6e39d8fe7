"""k_encode's block decisions and byte emission under crafted tables (tests/encode_table_cases.py builds the cases,
tests/test_encode_table_cpu.py proves on the CPU what they reach):

  1  every escape pattern of a NORMAL block in 512-colour mode, as an I- and as a P-frame; the 256-colour control
  2  every bit of the +-2 matrix decides one block: FILL (acc1, I-frame) and COPY (acc2, P-frame)
  3  every (count1, count2) with every compared pixel on the edge of the predicate; every kind of block behind every kind
     across wave and tile boundaries; the GOPs in batches with the entry plane handed over
  4  last waves of one, two and three bytes at every destination alignment
  5  frames of 33 bytes per block
  6  agmv_hip_within2_count on every difference in [-4, 4]^3

Expected bytes are the oracle's, assembled from the entry planes.  Every case goes down both paths, agmv_hip_encode_frames_dev
on the pixels pal[entries] and agmv_hip_encode_entries_dev on the entries.  The output rows are filled with 0xA5 before the
call and compared WHOLE: k_encode copies out exactly the bytes of each wave (wave_copy_own_u: head bytes, dwords, tail bytes of
`total` bytes), so a frame's row keeps the fill from its size on."""
import numpy as np
import pytest

import encode_table_cases as TC

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("mode512", [True, False], ids=["m512", "m256"])
PATHS = pytest.mark.parametrize("path", ["pixels", "entries"])
FILLER = 0xA5


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


@pytest.fixture(autouse=True)
def default_grid(monkeypatch):
    monkeypatch.delenv("AGMV_ENC_GRID", raising=False)


def encode(torch, hip, c, path, lo=0, hi=None, stride=None, ient=None):
    """frames lo .. hi-1 of the case in one call -> (out u8 [n, stride], sizes i32 [n]) on the device; ient: the i16 device plane
    handed from call to call (the case's own I plane when it starts inside a GOP)"""
    hi = c.n if hi is None else hi
    n, stride = hi - lo, stride or hip.max_usize(c.w, c.h)
    src = c.pal[c.entries[lo:hi]] if path == "pixels" else c.entries[lo:hi].astype(np.uint32)
    src = torch.from_numpy(src.view(np.int32)).cuda()
    if ient is None and c.iplane is not None:
        ient = torch.from_numpy(c.iplane.view(np.int16).copy()).cuda()
    out = torch.full((n, stride), FILLER, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    f = hip.L.agmv_hip_encode_frames_dev if path == "pixels" else hip.L.agmv_hip_encode_entries_dev
    hip._ck(f(hip.ctx, src.data_ptr(), n, c.w, c.h, c.first_fc + lo, out.data_ptr(), stride, sizes.data_ptr(),
              ient.data_ptr() if ient is not None else None, hip._stream()))
    hip.check()
    return out, sizes


def assert_rows(torch, c, out, sizes, lo=0, what=""):
    """sizes, bytes, and the fill behind them"""
    n, stride = out.shape
    exp = np.full((n, stride), FILLER, np.uint8)
    for f in range(n):
        exp[f, :len(c.bytes[lo + f])] = c.bytes[lo + f]
    got_sizes = sizes.cpu().numpy()
    exp_sizes = np.array([len(b) for b in c.bytes[lo:lo + n]], np.int32)
    assert (got_sizes == exp_sizes).all(), "%s %s: sizes %s for %s" % (c.name, what, got_sizes[:16], exp_sizes[:16])
    if not torch.equal(out, torch.from_numpy(exp).cuda()):
        f, b = np.argwhere(out.cpu().numpy() != exp)[0]
        raise AssertionError("%s %s: frame %d differs first at byte %d of %d (%s the frame's size)" % (
            c.name, what, lo + f, b, exp_sizes[f], "below" if b < exp_sizes[f] else "AT OR ABOVE"))


def set_palette(hip, c):
    hip.set_palette(*TC.halves(c.pal), c.mode512)


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@PATHS
@MODES
def test_every_escape_pattern(torch, hip, mode512, path):
    c = TC.escape_patterns(mode512)
    set_palette(hip, c)
    assert_rows(torch, c, *encode(torch, hip, c, path), what=path)


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@PATHS
@pytest.mark.parametrize("pframe", [False, True], ids=["I", "P"])
@MODES
def test_every_matrix_bit_decides_a_block(torch, hip, mode512, pframe, path):
    """I: row = the block's top-left entry, FILL when the bit is set.  P (encoded alone at frame_count 1, its I plane handed
    over): row = the I-frame's entry, COPY when the bit is set"""
    c, _ = TC.matrix_bits(mode512, pframe)
    set_palette(hip, c)
    assert_rows(torch, c, *encode(torch, hip, c, path), what=path)


# ---- 3 ------------------------------------------------------------------------------------------------------------------
@PATHS
@MODES
def test_decisions_on_the_edge_of_the_predicate(torch, hip, mode512, path):
    c, _ = TC.edge_decisions(mode512)
    set_palette(hip, c)
    assert_rows(torch, c, *encode(torch, hip, c, path), what=path)


@PATHS
@MODES
def test_decisions_on_the_edge_in_batches(torch, hip, mode512, path):
    """batches of 1, 3, 2, 2 and 4 frames: the second and the fourth start inside a GOP, at phases 1 and 2"""
    c, _ = TC.edge_decisions(mode512)
    set_palette(hip, c)
    ient = torch.zeros(c.w * c.h, dtype=torch.int16, device="cuda")
    lo = 0
    for n in (1, 3, 2, 2, 4):
        assert_rows(torch, c, *encode(torch, hip, c, path, lo, lo + n, ient=ient), lo=lo, what="%s, batch of %d from %d" % (path, n, lo))
        last_i = (lo + n - 1) & ~3
        assert (ient.cpu().numpy().view(np.uint16).reshape(c.h, c.w) == c.entries[last_i]).all(), "entry plane after the batch from %d" % lo
        lo += n
    assert lo == c.n


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@PATHS
@pytest.mark.parametrize("extra", TC.TAIL_STRIDE_EXTRA)
@pytest.mark.parametrize("shape", TC.TAIL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_last_wave_of_one_to_three_bytes(torch, hip, shape, extra, path):
    c = TC.short_tails(shape, extra)
    set_palette(hip, c)
    assert c.stride == hip.max_usize(c.w, c.h) + extra
    out, sizes = encode(torch, hip, c, path, stride=c.stride)
    assert out.data_ptr() % 4 == 0, "the residues of the case count from a 4-byte aligned slab"
    assert_rows(torch, c, out, sizes, what=path)


# ---- 5 ------------------------------------------------------------------------------------------------------------------
@PATHS
@pytest.mark.parametrize("grid", [None, 1])
@pytest.mark.parametrize("shape", [(2052, 4), (300, 40)], ids=lambda s: "%dx%d" % s)
def test_frames_at_their_maximum(torch, hip, monkeypatch, shape, grid, path):
    c = TC.full_frames(shape)
    if grid:
        monkeypatch.setenv("AGMV_ENC_GRID", str(grid))
    set_palette(hip, c)
    out, sizes = encode(torch, hip, c, path)
    assert sizes.cpu().tolist() == [33 * c.nblk] * 2 and 33 * c.nblk + 64 <= out.shape[1] == hip.max_usize(c.w, c.h)
    assert_rows(torch, c, out, sizes, what="%s, grid %s" % (path, grid))


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_within2_count_against_numpy(hip):
    a, b = TC.predicate_calls()
    want = TC.within2_np(a, b).sum(axis=1)
    got = [hip.L.agmv_hip_within2_count(hip.ctx, a[k].ctypes.data, b[k].ctypes.data) for k in range(len(a))]
    bad = [k for k in range(len(a)) if got[k] != want[k]]
    assert not bad, "calls %s: got %s, numpy has %s" % (bad[:8], [got[k] for k in bad[:8]], want[bad[:8]].tolist())
