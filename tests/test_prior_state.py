"""Decoding from a given decoder state, on the CPU: the oracle started from a snapshot continues a serial decode exactly,
and shard.range_depends_on_prior_state -- what shard.decode_sharded trusts before it keeps a range decoded from the fresh
state -- is SOUND: whenever it says "does not depend", decodes of the range from three different prior states agree.
(It is documented as conservative, so it may say "depends" for a range that does not.)  No GPU."""
import os

import numpy as np
import pytest
import torch

import oracles as O
import streams as T
from libagmv_amd import shard


def _snapshot_state(pix, k, first_fc=0):
    """decoder state before frame k of a serial decode that started fresh at frame_count first_fc: img_data = frame k-1,
    iframe->img_data = the last frame before k with frame_count % 4 == 0 (zeroed if none)"""
    prev = pix[k - 1] if k else None
    last_i = [f for f in range(k) if (first_fc + f) % 4 == 0]
    return prev, (pix[last_i[-1]] if last_i else None)


@pytest.mark.parametrize("mode512", [True, False])
def test_oracle_decoder_started_from_a_snapshot(mode512):
    """OracleDecoder.set_state: decode a clip serially, start a second decoder from the state after frame k-1 (the last
    frame, the snapshot of the last I-frame, frame_count k); frames k.. must come out the same -- k inside a GOP and at
    a GOP boundary, clean streams (fresh bitstream buffer) and damaged ones (the buffer handed over too)"""
    rng = np.random.default_rng(31 + mode512)
    W, H, n = 24, 16, 14
    frames = T.clip(rng, W, H, n)
    p0, p1 = T.palettes(rng, frames)
    clean = T.encode(W, H, mode512, p0, p1, frames)
    hurt = [T.damage(rng, b, W, H, rate=1) for b in clean]
    for bits, hand_buffer in ((clean, False), (hurt, True)):
        dec = O.OracleDecoder(W, H, mode512, p0, p1)
        pix, bufs = [], []
        for b in bits:
            bufs.append(dec.state()[3])                       # the persistent buffer BEFORE frame f
            pix.append(dec.decode(b))
        pix = np.stack(pix)
        for k in (1, 3, 4, 6, 8, 9, 12):
            prev, previ = _snapshot_state(pix, k)
            d2 = O.OracleDecoder(W, H, mode512, p0, p1)
            d2.set_state(prev, previ, k, bufs[k] if hand_buffer else None)
            img, ifr, fc, _ = d2.state()
            assert fc == k and (img == (prev if prev is not None else 0)).all() and (ifr == (previ if previ is not None else 0)).all()
            for f in range(k, n):
                assert (d2.decode(bits[f]) == pix[f]).all(), "restart at %d (GOP %s): frame %d" % (k, "boundary" if k % 4 == 0 else "inside", f)
    # a fresh decoder is the state (0, 0, 0)
    d3 = O.OracleDecoder(W, H, mode512, p0, p1)
    d3.set_state(None, None, 0)
    assert all((d3.decode(b) == pix[f]).all() for f, b in enumerate(hurt))


def _streams(rng, W, H, n, mode512, p0, p1, first_fc, kind):
    if kind == "soup":
        return T.block_soup(rng, W, H, n, mode512)
    bits = T.encode(W, H, mode512, p0, p1, T.clip(rng, W, H, n), first_fc)
    if kind == "clean":
        return bits
    return [T.damage(rng, b, W, H, rate=2) for b in bits]


@pytest.mark.parametrize("seed", range(int(os.environ.get("AGMV_FUZZ_SEEDS", "6"))))
def test_host_dependency_predicate_is_sound(seed):
    """seeded clips (clean, damaged, block soup) decoded with the oracle in ranges, each range from the fresh state, from
    S_A (random) and from S_B = S_A ^ 0xFFFFFF: where range_depends_on_prior_state says False the three decodes are
    equal.  first_is_iframe=False is always a valid call (and always answers True); True only for a range that starts at a
    GOP boundary, where it must be sound."""
    rng = np.random.default_rng(7000 + seed)
    checked = 0
    for it in range(12):
        W, H = 4 * int(rng.integers(1, 20)), 4 * int(rng.integers(1, 14))
        nblk = W * H // 16
        mode512 = bool(rng.integers(0, 2))
        first_fc = int(rng.choice([0, 1, 2, 3, 8 + int(rng.integers(0, 4))]))
        kind = ("clean", "damaged", "damaged", "soup")[it % 4]
        n = int(rng.integers(1, 10))
        frames_for_pal = T.clip(rng, W, H, 2)
        p0, p1 = T.palettes(rng, frames_for_pal)
        bits = _streams(rng, W, H, n, mode512, p0, p1, first_fc, kind)
        cuts = sorted(set([0, n] + [int(c) for c in rng.integers(0, n + 1, 2)]))
        st = T.prior_states(rng, W, H)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            fc = first_fc + lo
            dec = {k: T.oracle_range(W, H, mode512, p0, p1, bits[lo:hi], fc, *v) for k, v in st.items()}
            pix = {k: v[0] for k, v in dec.items()}
            _, pads, offs, nent = dec["zero"]
            for k in ("A", "B"):                               # the parse is a function of the streams alone
                assert (dec[k][2] == offs).all() and (dec[k][3] == nent).all()
            rows, bpos = T.slab(bits[lo:hi], pads)
            args = (torch.from_numpy(rows), torch.from_numpy(bpos), torch.from_numpy(offs.astype(np.int64)),
                    torch.from_numpy(nent.astype(np.int32)), nblk, mode512)
            kw = {"w": W}
            depends = not (pix["A"] == pix["B"]).all()
            same3 = not depends and (pix["zero"] == pix["A"]).all()
            assert shard.range_depends_on_prior_state(*args, first_is_iframe=False, **kw)
            if fc % 4 == 0:
                pred = shard.range_depends_on_prior_state(*args, first_is_iframe=True, **kw)
                checked += 1
                if not pred:
                    assert same3, "predicate says independent, the decodes differ: %dx%d mode512=%s %s frames %d..%d (fc %d)" % (
                        W, H, mode512, kind, lo, hi, fc)
    assert checked


def test_host_predicate_width_4_last_block_fill():
    """rule (d) of range_depends_on_prior_state: at width 4 an encoder I-frame ending in a FILL reads pixel (3,0) of the
    frame before -- the decodes from S_A and S_B differ and the predicate says so when it knows the width (w=4, or a frame
    of one block); at width 8 the same content reads nothing from before the range and the predicate says so"""
    import synth as S
    for W, H, w_arg in ((4, 8, 4), (4, 4, None), (4, 4, 4), (8, 8, 8), (8, 8, None)):
        frames = np.stack([np.full((H, W), 0x123456 + 0x010101 * t, np.uint32) for t in range(4)])
        p0, p1 = S.content_palettes(frames)
        bits = T.encode(W, H, True, p0, p1, frames)
        st = T.prior_states(np.random.default_rng(W * H), W, H)
        dec = {k: T.oracle_range(W, H, True, p0, p1, bits, 0, *v) for k, v in st.items()}
        _, pads, offs, nent = dec["zero"]
        rows, bpos = T.slab(bits, pads)
        pred = shard.range_depends_on_prior_state(torch.from_numpy(rows), torch.from_numpy(bpos), torch.from_numpy(offs.astype(np.int64)),
                                                  torch.from_numpy(nent.astype(np.int32)), W * H // 16, True, first_is_iframe=True, w=w_arg)
        depends = not (dec["A"][0] == dec["B"][0]).all()
        assert depends == (W == 4), (W, H)
        assert pred == depends, (W, H, w_arg)
