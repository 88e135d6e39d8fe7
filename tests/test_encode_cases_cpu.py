"""The case builders of tests/encode_cases.py checked on the CPU: what the periodic clip's expectations rest on (the oracle
encoder's state does not outlive a GOP), the arithmetic of the ticket-order model for the two cases that take one workgroup's
item counter past 65 536, and that the comparison helper leaves out no frame and no byte below a frame's size."""
import numpy as np
import pytest
import torch

import encode_cases as EC
import oracles as O

PERIODIC_SHAPES = [(8, 8), (68, 36), (2052, 4), (300, 40)]     # every shape a periodic clip is built for
WRAP_CASES = [((8, 8), 66002), ((2052, 4), 33202)]


def test_adversarial_clip_has_seven_gops_and_the_known_head():
    w, h = 300, 40
    f = EC.adversarial_frames(w, h)
    assert f.shape == (27, h, w) and EC.n_groups(27) == 7 and EC.group_frames(6, 27) == (24, 27)
    rng = np.random.default_rng(w * 1000 + h)                  # the head: test_encode_vs_oracle_shapes_and_content's frames
    for t in range(3):
        assert (f[t] == rng.integers(0, 1 << 24, size=(h, w), dtype=np.uint32)).all()
    assert (f[3] == 0x808080).all() and (f[4] == 0x808181).all() and (f[5] == f[0]).all() and (f[6] == f[0] ^ 0x010101).all()
    assert (f[14] == f[12]).all() and (f[15] == f[12] ^ 0x010101).all()    # second round: P-frames 14, 15 repeat I-frame 12
    assert (f[11][:, :w // 4] == f[8][:, :w // 4]).all() and (f[11] != f[8]).any()      # P-frame 11: static left quarter of I-frame 8
    kinds = {len(np.unique(x)) == 1 for x in f}
    assert kinds == {True, False}
    assert (EC.adversarial_frames(w, h, 28)[:27] == f).all()


@pytest.mark.parametrize("mode512", [True, False])
@pytest.mark.parametrize("shape", PERIODIC_SHAPES, ids=lambda s: "%dx%d" % s)
def test_encoder_state_does_not_outlive_a_gop(shape, mode512):
    """the base clip encoded a second time by the same encoder, and by fresh encoders started at later frame counts, gives the
    same bytes; a marker GOP inside a running clip gives the bytes of a fresh encoder started at its frame count"""
    w, h = shape
    base = EC.oracle_clip(w, h, mode512, EC.P)
    enc = O.OracleEncoder(w, h, mode512, *base.pal)
    first = [enc.encode(f) for f in base.frames]
    mark = EC.marker_frames(w, h, 7, 4)
    running = [enc.encode(f) for f in mark]                    # GOP 7 of a running clip
    again = [enc.encode(f) for f in base.frames[4:]]           # GOPs 8 ..: the base from its GOP 1
    enc.close()
    for t in range(EC.P):
        assert (first[t].shape == base.bytes[t].shape) and (first[t] == base.bytes[t]).all(), t
    for t in range(4, EC.P):
        assert again[t - 4].shape == base.bytes[t].shape and (again[t - 4] == base.bytes[t]).all(), t
    for fc in (16, EC.P, 4 * 16383):
        e = O.OracleEncoder(w, h, mode512, *base.pal, first_frame_count=fc)
        for t in range(fc % EC.P, EC.P):
            b = e.encode(base.frames[t])
            assert b.shape == base.bytes[t].shape and (b == base.bytes[t]).all(), (fc, t)
        e.close()
    p = EC.Periodic(w, h, mode512, 35, [7])
    for j in range(4):                                         # frames 28 .. 31 of 35
        r = p.row_of[28 + j]
        assert r == EC.P + j and p.row_sizes[r] == len(running[j]) and (p.rows[r, :len(running[j])] == running[j]).all()


def test_periodic_clip_rows_and_pixels():
    w, h = 68, 36
    n = 4 * 40 - 1
    p = EC.Periodic(w, h, True, n, [0, 1, 20, 38, 39])
    assert p.rows.shape == (EC.P + 4 * 4 + 3, O.max_usize(w, h)) and p.row_of.shape == (n,)
    assert sorted(set(p.row_of.tolist())) == list(range(len(p.rows))), "a row no frame expects, or a frame without a row"
    pix = p.pixels(torch, "cpu").numpy().view(np.uint32)
    assert pix.shape == (n, h, w)
    for t in range(n):
        assert (pix[t] == p.frame(t)).all(), t
        marked = t // 4 in (0, 1, 20, 38, 39)
        assert (p.row_of[t] >= EC.P) == marked and (marked or p.row_of[t] == t % EC.P), t
    enc = O.OracleEncoder(w, h, True, *p.pal)                  # the whole clip through ONE encoder gives the rows
    for t in range(n):
        b, r = enc.encode(pix[t]), p.row_of[t]
        assert len(b) == p.row_sizes[r] and (p.rows[r, :len(b)] == b).all(), t
    enc.close()
    m = [p.markers[g] for g in (0, 1, 20, 38, 39)]
    assert len(m[-1]) == 3 and all(len(x) == 4 for x in m[:-1])
    for a in range(5):
        for b in range(a):
            assert (m[a][0] != m[b][0]).any(), "two markers with the same noise"
    sz = p.row_sizes
    assert (sz > 0).all() and (p.rows[np.arange(len(sz)), sz - 1] != 0).any()
    assert not (p.rows[np.arange(p.rows.shape[1])[None, :] >= sz[:, None]]).any(), "padding is zero"


@pytest.mark.parametrize("shape,n_frames", WRAP_CASES, ids=["8x8", "2052x4"])
def test_ticket_order_model_at_the_tag_wrap(shape, n_frames):
    tpf = EC.tiles_per_frame(*shape)
    assert tpf == {(8, 8): 1, (2052, 4): 2}[shape]
    items = list(EC.items_in_ticket_order(n_frames, tpf))
    assert len(items) == n_frames * tpf > 65537
    assert all(items[k] == EC.item_tile_frame(k, n_frames) for k in range(len(items)))
    assert sorted(items) == [(t, f) for t in range(tpf) for f in range(n_frames)], "every item once"
    ng = EC.n_groups(n_frames)
    lo, hi = EC.group_frames(ng - 1, n_frames)
    assert hi == n_frames and hi - lo == 2, "both clips end in a GOP of two frames"
    gs = EC.wrap_marker_groups(n_frames, tpf)
    held = {items[k][1] // 4 for k in range(65534, 65538)}
    assert set(gs) == held | {0, ng - 1}
    if shape == (8, 8):
        assert gs == [0, 16383, 16384, 16500] and [items[k] for k in (65535, 65536)] == [(0, 65535), (0, 65536)]
    else:
        assert gs == [0, 8083, 8300] and [items[k] for k in (65534, 65537)] == [(1, 32332), (1, 32335)]


@pytest.mark.parametrize("first_fc", [0, 1, 2, 3])
@pytest.mark.parametrize("n_frames", [1, 3, 4, 5, 9, 13, 16])
def test_ticket_order_model_with_short_first_and_last_gops(n_frames, first_fc):
    tpf = 3
    ng = EC.n_groups(n_frames, first_fc)
    spans = [EC.group_frames(g, n_frames, first_fc) for g in range(ng)]
    assert spans[0][0] == 0 and spans[-1][1] == n_frames and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert all(0 < hi - lo <= 4 for lo, hi in spans)
    for g, (lo, hi) in enumerate(spans):
        assert all(EC.group_of_frame(f, first_fc) == g for f in range(lo, hi))
        assert all(((first_fc + f) & 3 == 0) == (f == lo) for f in range(lo, hi) if g or not first_fc & 3), "a group starts at its I-frame"
    items = list(EC.items_in_ticket_order(n_frames, tpf, first_fc))
    assert items == [EC.item_tile_frame(k, n_frames) for k in range(n_frames * tpf)]
    assert [EC.ticket_tile_group(t, n_frames, first_fc) for t in range(ng * tpf)] == [(t, g) for t in range(tpf) for g in range(ng)]


def test_comparison_helper_sees_every_frame_and_every_byte_below_the_size():
    rng = np.random.default_rng(3)
    stride, n = 40, 23
    rows = rng.integers(1, 256, (5, stride), dtype=np.uint8)
    row_sizes = np.array([0, 1, 17, 39, 40], np.int32)
    row_of = rng.integers(0, 5, n)
    row_of[:5] = np.arange(5)
    out = rows[row_of].copy()
    keep = np.arange(stride)[None, :] < row_sizes[row_of][:, None]
    out[~keep] = rng.integers(0, 256, int((~keep).sum()), dtype=np.uint8)      # unspecified bytes: anything
    sizes = row_sizes[row_of].copy()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    run = lambda o, s, chunk: EC.mismatched_frames(torch, t(o), t(s), t(rows), t(row_sizes), t(row_of), chunk_bytes=chunk)
    for chunk in (1, 3 * stride, 1 << 20):                     # one frame per chunk, an odd number, all at once
        assert run(out, sizes, chunk) == []
        for f in range(n):
            for b in sorted({0, int(sizes[f]) // 2, int(sizes[f]) - 1} - {-1}):
                if b < sizes[f]:
                    o = out.copy()
                    o[f, b] ^= 1
                    assert run(o, sizes, chunk) == [f], (f, b)
            s = sizes.copy()
            s[f] += 1
            assert run(out, s, chunk) == [f]
        o = out.copy()
        o[0, 5] ^= 1
        o[n - 1, :] ^= 1
        exp = [f for f in (0, n - 1) if sizes[f] > (5 if f == 0 else 0)]
        assert run(o, sizes, chunk) == exp
