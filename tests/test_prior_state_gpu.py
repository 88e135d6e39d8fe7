"""The decoder's prior-state contract on the GPU, against the oracle started from the same state (tests/streams.py):
pixels and nentered of every decode entry point from three prior states, the exactness of
agmv_hip_decode_prior_dependent after each of them, and batches past the parser's grid limit (65 535 frames) and the
65 532-frame parts of agmv_hip_decode_bitstreams_dev -- including the prior-dependence flag of a call cut into parts.
Needs an MI355X."""
import functools
import os

import numpy as np
import pytest

import oracles as O
import streams as T
import synth as S

pytestmark = pytest.mark.gpu

PART = 65532                                    # agmv_hip_decode_bitstreams_dev cuts longer batches into parts of at most this


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


def dev_u32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def to_u32(t):
    return t.cpu().numpy().view(np.uint32)


def _bad_frames(a, b):
    return np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0][:8].tolist()


# ------------------------------------------------------------------------------- C: decodes from foreign states
# (W, H, mode512, first_frame_count, kind) of the first seeds: one block, one block per row (a last-block FILL reads the
# block's own pixel of the frame before), a last block that is the first of its k_decode tile (nblk = 257 / 513: its left
# neighbour sits in another tile), odd sizes; later seeds draw at random
CASES = [(4, 4, True, 0, "clean"), (8, 8, False, 1, "damaged"), (4, 24, True, 0, "soup"), (20, 12, False, 3, "damaged"),
         (64, 48, True, 8, "clean"), (108, 76, False, 0, "clean"), (1028, 4, True, 0, "damaged"), (36, 228, False, 2, "soup"),
         (300, 40, True, 9, "damaged"), (132, 100, False, 3, "clean"), (108, 76, True, 0, "damaged"), (1028, 4, False, 8, "clean")]


def _case(seed):
    rng = np.random.default_rng(20000 + seed)
    if seed < len(CASES):
        W, H, mode512, first_fc, kind = CASES[seed]
    else:
        W, H = 4 * int(rng.integers(1, 80)), 4 * int(rng.integers(1, 60))
        mode512 = bool(rng.integers(0, 2))
        first_fc = int(rng.choice([0, 1, 2, 3, 8 + int(rng.integers(0, 4))]))
        kind = ("clean", "damaged", "soup", "damaged")[seed % 4]
    n = int(rng.integers(1, 11))
    return rng, W, H, mode512, first_fc, kind, n


def _entry_points(torch, hip, monkeypatch, dbits, dbpos, n, W, H, fc, prev, previ):
    """the batch through every decode entry point; yields (name, pixels, nentered, offsets or None, flag)"""
    monkeypatch.delenv("AGMV_DEC_SLICES", raising=False)
    offs, nent = hip.parse_dev(dbits, dbpos, n, W, H)
    pix = hip.decode_dev(dbits, dbpos, offs, nent, n, W, H, fc, prev=prev, prev_iframe=previ)
    yield "parse_dev+decode_dev", pix, nent, offs, hip.decode_depends_on_prior(W, H)
    for sl in (None, "3"):
        if sl:
            monkeypatch.setenv("AGMV_DEC_SLICES", sl)
        pix, offs, nent = hip.parse_decode_dev(dbits, dbpos, n, W, H, fc, prev=prev, prev_iframe=previ)
        yield "parse_decode_dev slices=%s" % sl, pix, nent, offs, hip.decode_depends_on_prior(W, H)
    monkeypatch.delenv("AGMV_DEC_SLICES", raising=False)
    nent = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    pix = hip.decode_bitstreams_dev(dbits, dbpos, n, W, H, fc, nentered=nent, prev=prev, prev_iframe=previ)
    yield "decode_bitstreams_dev", pix, nent, None, hip.decode_depends_on_prior(W, H)


@pytest.mark.parametrize("seed", range(int(os.environ.get("AGMV_FUZZ_SEEDS", "12"))))
def test_prior_state_decodes_and_exact_flag(torch, hip, monkeypatch, seed):
    """a batch (encoder output, damaged encoder output or block soup; first_frame_count 0..3 or inside a later GOP)
    decoded from the fresh state, S_A and S_B = S_A ^ 0xFFFFFF through parse_dev + decode_dev, parse_decode_dev (one range
    and AGMV_DEC_SLICES=3) and decode_bitstreams_dev: pixels and nentered equal the oracle started from the same state;
    the prior-dependence flag is the same after every entry point and EXACT -- 1 if and only if the S_A and S_B decodes
    differ (prior pixels are only ever copied, and the two states differ at every pixel of both planes); where the batch
    starts at a GOP boundary the host predicate agrees in the direction GPU => host, and encoder output gives 0."""
    from libagmv_amd import shard
    rng, W, H, mode512, first_fc, kind, n = _case(seed)
    nblk = W * H // 16
    p0, p1 = T.palettes(rng, T.clip(rng, W, H, 2))
    if kind == "soup":
        bits = T.block_soup(rng, W, H, n, mode512)
    else:
        bits = T.encode(W, H, mode512, p0, p1, T.clip(rng, W, H, n), first_fc)
        if kind == "damaged":
            bits = [T.damage(rng, b, W, H, rate=2) for b in bits]
    hip.set_palette(p0, p1, mode512)
    states = T.prior_states(rng, W, H)
    exp = {k: T.oracle_range(W, H, mode512, p0, p1, bits, first_fc, *v) for k, v in states.items()}
    _, pads, offs, nent = exp["zero"]
    rows, bpos = T.slab(bits, pads)
    dbits, dbpos = torch.from_numpy(rows).cuda(), torch.from_numpy(bpos).cuda()
    where = "%dx%d mode512=%s %s n=%d first_fc=%d" % (W, H, mode512, kind, n, first_fc)
    flags = set()
    for sname, (a, ai) in states.items():
        prev = dev_u32(torch, a) if a is not None else None
        previ = dev_u32(torch, ai) if ai is not None else None
        for name, pix, ne, of, flag in _entry_points(torch, hip, monkeypatch, dbits, dbpos, n, W, H, first_fc, prev, previ):
            got = to_u32(pix).reshape(n, -1)
            assert (ne.cpu().numpy() == nent).all(), "%s, state %s, %s: nentered" % (where, sname, name)
            assert (got == exp[sname][0]).all(), "%s, state %s, %s: pixels differ in frames %s" % (where, sname, name, _bad_frames(got, exp[sname][0]))
            if of is not None:
                o = to_u32(of).reshape(n, nblk)
                for f in range(n):
                    assert (o[f, :nent[f]] == offs[f, :nent[f]]).all(), "%s, %s: offsets of frame %d" % (where, name, f)
            flags.add((sname, name, flag))
    assert len({f for _, _, f in flags}) == 1, "%s: the flag depends on the entry point or the state: %s" % (where, sorted(flags))
    flag = flags.pop()[2]
    differs = not (exp["A"][0] == exp["B"][0]).all()
    if not flag:                                              # soundness: never relaxed
        assert not differs and (exp["zero"][0] == exp["A"][0]).all(), "%s: flag 0 but the prior state shows" % where
    assert flag == differs, "%s: flag 1 but no pixel derives from the prior state" % where
    if first_fc % 4 == 0:
        host = shard.range_depends_on_prior_state(torch.from_numpy(rows), torch.from_numpy(bpos), torch.from_numpy(offs.astype(np.int64)),
                                                  torch.from_numpy(nent.astype(np.int32)), nblk, mode512, first_is_iframe=True, w=W)
        assert host or not flag, "%s: the GPU says the batch depends on its prior state, the host predicate does not" % where
        if kind == "clean" and W > 4:                         # "never 1 for a stream the encoder emits" (w = 4: see agmv_hip.h)
            assert not flag, "%s: encoder output reported as prior-dependent" % where


@pytest.mark.parametrize("first_fc", [1, 2, 3])
def test_copy_in_the_first_iframe_of_a_batch_that_starts_inside_a_gop(torch, hip, monkeypatch, first_fc):
    """a batch that starts inside a GOP has no I-frame of its own before its second GOP: a COPY block in that GOP's
    I-frame (a damaged stream) reads the CALLER's I-frame snapshot.  The pixels follow it and the flag says 1, though
    no frame of the batch's first GOP reads anything from before the batch (found by the seeded fuzz above)"""
    W, H = 64, 48
    nblk = W * H // 16
    frames = np.stack([S.synth_frame(W, H, t) for t in range(8)])
    p0, p1 = S.content_palettes(frames[:4])
    hip.set_palette(p0, p1, True)
    bits = T.encode(W, H, True, p0, p1, frames, first_fc)
    i0 = 4 - first_fc                                         # the batch's first I-frame
    bits[i0] = np.concatenate([np.full(3, 0x5E, np.uint8), bits[i0][3:]])   # its first three blocks: COPY
    st = T.prior_states(np.random.default_rng(first_fc), W, H)
    exp = {k: T.oracle_range(W, H, True, p0, p1, bits, first_fc, *v) for k, v in st.items()}
    _, pads, _, nent = exp["zero"]
    assert (nent[:i0] == nblk).all()
    rows, bpos = T.slab(bits, pads)
    dbits, dbpos = torch.from_numpy(rows).cuda(), torch.from_numpy(bpos).cuda()
    assert (exp["A"][0][:i0] == exp["B"][0][:i0]).all() and not (exp["A"][0] == exp["B"][0]).all()
    for k in ("A", "B"):
        a, ai = st[k]
        for name, pix, ne, _, flag in _entry_points(torch, hip, monkeypatch, dbits, dbpos, 8, W, H, first_fc,
                                                      dev_u32(torch, a), dev_u32(torch, ai)):
            assert (to_u32(pix).reshape(8, -1) == exp[k][0]).all(), (k, name)
            assert flag, (k, name)


def test_encoder_output_at_width_4_reads_the_frame_before(torch, hip):
    """the one exception agmv_hip.h states for encoder output: with one block per row a FILL as the last block stores the
    block's own pixel (3,0) of the frame before (the reference's x-1 wraps), so an encoder I-frame ending in a FILL
    depends on the state before it -- the flag says so and the pixels follow the prior state; at width 8 it does not"""
    for W in (4, 8):
        H = 8
        frames = np.stack([np.full((H, W), 0x123456 + 0x010101 * t, np.uint32) for t in range(4)])
        p0, p1 = S.content_palettes(frames)
        hip.set_palette(p0, p1, True)
        bits = T.encode(W, H, True, p0, p1, frames)
        st = T.prior_states(np.random.default_rng(W), W, H)
        exp = {k: T.oracle_range(W, H, True, p0, p1, bits, 0, *v)[0] for k, v in st.items()}
        rows, bpos = T.slab(bits, [np.zeros(16, np.uint8)] * 4)
        dbits, dbpos = torch.from_numpy(rows).cuda(), torch.from_numpy(bpos).cuda()
        for k, (a, ai) in st.items():
            pix = hip.decode_bitstreams_dev(dbits, dbpos, 4, W, H, 0, prev=dev_u32(torch, a) if a is not None else None,
                                            prev_iframe=dev_u32(torch, ai) if ai is not None else None)
            assert (to_u32(pix).reshape(4, -1) == exp[k]).all(), (W, k)
            assert hip.decode_depends_on_prior(W, H) == (W == 4), (W, k)
        assert (not (exp["A"] == exp["B"]).all()) == (W == 4)


def test_robust_parser_alone_on_a_fresh_context(torch, monkeypatch):
    """AGMV_HIP_PARSE=robust with decode_bitstreams_dev as the FIRST call of a new context (no speculative walk has
    written the entry bitmap words before): streams whose bpos leaves region words past the parser's last chunk must
    decode as the serial parse and the oracle do"""
    from libagmv_amd import AgmvHip
    W, H, n = 320, 240, 6
    rng = np.random.default_rng(44)
    frames = np.stack([S.synth_frame(W, H, t) for t in range(n)])
    p0, p1 = S.content_palettes(frames[:4])
    bits = T.encode(W, H, True, p0, p1, frames)
    bits = [b[:max(1, len(b) - int(c))] for b, c in zip(bits, rng.integers(0, 3000, n))]     # bpos anywhere in a region
    exp, pads, offs, nent = T.oracle_range(W, H, True, p0, p1, bits, 0)
    rows, bpos = T.slab(bits, pads)
    dbits, dbpos = torch.from_numpy(rows).cuda(), torch.from_numpy(bpos).cuda()
    monkeypatch.setenv("AGMV_HIP_PARSE", "robust")
    h = AgmvHip(0)
    try:
        h.set_palette(p0, p1, True)
        ne = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        pix = h.decode_bitstreams_dev(dbits, dbpos, n, W, H, 0, nentered=ne)
        got = to_u32(pix).reshape(n, -1)
        assert (ne.cpu().numpy() == nent).all()
        assert (got == exp).all(), _bad_frames(got, exp)
        monkeypatch.setenv("AGMV_HIP_PARSE", "serial")
        o_ser, n_ser = h.parse_dev(dbits, dbpos, n, W, H)
        assert (n_ser.cpu().numpy() == nent).all()
    finally:
        h.close()


# ------------------------------------------------------------------------------- D: past the parser's grid limit
def _tiny_clip(W, H, N, seed):
    """N frames drawn from 48 mixed-content base frames with repeats (COPY), flat and tiled frames (FILL), noise (NORMAL)"""
    rng = np.random.default_rng(seed)
    base = T.clip(rng, W, H, 48)
    base[0] = 0x0A0B0C
    stay = rng.random(N) < 0.45
    idx = np.where(stay, 0, rng.integers(0, 48, N))
    for_runs = np.maximum.accumulate(np.where(stay, 0, np.arange(N)))   # a repeated frame repeats the last drawn one
    idx = idx[for_runs]
    return np.ascontiguousarray(base[idx]), S.content_palettes(base)


@functools.lru_cache(maxsize=None)
def _big(W, H):
    """the clip of (2 * PART + 5) frames, the GPU's encoding of it (kept on the device), a random prior state"""
    import torch
    N = 2 * PART + 5
    frames, (p0, p1) = _tiny_clip(W, H, N + 1, 700 + W)
    rng = np.random.default_rng(800 + W)
    prev = rng.integers(0, 1 << 24, size=(H, W), dtype=np.uint32)
    previ = rng.integers(0, 1 << 24, size=(H, W), dtype=np.uint32)
    return frames, p0, p1, prev, previ


@functools.lru_cache(maxsize=None)
def _oracle_decode(W, H, first_fc, key):
    """oracle decode of the device streams `_streams_cache[key]` (host copy) from the big clip's prior state"""
    bits = _streams_cache[key]
    frames, p0, p1, prev, previ = _big(W, H)
    return T.oracle_range(W, H, True, p0, p1, bits, first_fc, prev, previ)


_streams_cache = {}
TRUNCATED = (5, 4000, PART - 1, PART, PART + 1, 2 * PART - 2, 2 * PART, 2 * PART + 4)


_device_cache = {}


def _encoded(torch, hip, W, H):
    """the big clip encoded on the GPU, kept on the device: slab + sizes, with 8 streams cut to half their length (spread
    over both part boundaries); the host copy of the streams goes to _streams_cache.  Cached per geometry."""
    key = (W, H)
    frames, p0, p1, prev, previ = _big(W, H)
    hip.set_palette(p0, p1, True)
    if key not in _device_cache:
        N = 2 * PART + 5
        out, sizes = hip.encode_dev(dev_u32(torch, frames[:N]), N, W, H)
        hip.check()
        for f in TRUNCATED:
            sizes[f] = sizes[f] // 2
        host = out.cpu().numpy()
        sz = sizes.cpu().numpy()
        _streams_cache[key] = [host[f, :sz[f]].copy() for f in range(N)]
        _device_cache[key] = (out, sizes)
    return _device_cache[key]


def _with_pads(torch, out, sizes, pads):
    """the oracle's stale bytes behind every stream (they depend on the streams only, not on the state), on the device"""
    idx = sizes.long()[:, None] + torch.arange(16, device="cuda")[None, :]
    slab = out.clone()
    slab.scatter_(1, idx, torch.from_numpy(np.stack(pads)).cuda())
    return slab


def _parts(n, first_fc):
    """[f0, f1) parts of at most PART frames, each after the first starting with an I-frame (independent of the library)"""
    out, f0 = [], 0
    while f0 < n:
        f1 = n
        if f1 - f0 > PART:
            f1 = f0 + PART
            while (first_fc + f1) % 4:
                f1 -= 1
        out.append((f0, f1))
        f0 = f1
    return out


@pytest.mark.parametrize("geom", [(8, 8), (4, 4)])
def test_encode_past_65535_frames_vs_oracle(torch, hip, geom):
    """encode_dev of 2 * 65532 + 5 frames, and of 65537 frames starting inside a GOP (first_frame_count 1, the I-frame
    entries handed in), bit-exact against the serial oracle encoder"""
    W, H = geom
    frames, p0, p1, _, _ = _big(W, H)
    out, sizes = _encoded(torch, hip, W, H)
    N = 65538
    enc = O.OracleEncoder(W, H, True, p0, p1)
    exp = [enc.encode(frames[f]) for f in range(N)]
    host = out.cpu().numpy()
    sz = sizes.cpu().numpy()
    trunc = set(TRUNCATED)
    for f in range(N):
        if f not in trunc:
            assert sz[f] == len(exp[f]) and (host[f, :sz[f]] == exp[f]).all(), "frame %d" % f
        else:
            assert (host[f, :sz[f]] == exp[f][:sz[f]]).all(), "frame %d" % f
    ient = torch.zeros(W * H, dtype=torch.int16, device="cuda")
    hip.set_palette(p0, p1, True)
    o1, s1 = hip.encode_dev(dev_u32(torch, frames[:1]), 1, W, H, 0, ientries=ient)
    o2, s2 = hip.encode_dev(dev_u32(torch, frames[1:N]), N - 1, W, H, 1, ientries=ient)
    hip.check()
    h1, z1 = o1.cpu().numpy(), s1.cpu().numpy()
    h2, z2 = o2.cpu().numpy(), s2.cpu().numpy()
    assert z1[0] == len(exp[0]) and (h1[0, :z1[0]] == exp[0]).all()
    for f in range(1, N):
        assert z2[f - 1] == len(exp[f]) and (h2[f - 1, :z2[f - 1]] == exp[f]).all(), "frame %d of the batch from frame_count 1" % f


@pytest.mark.parametrize("geom,first_fc", [((8, 8), 0), ((8, 8), 1), ((8, 8), 3), ((4, 4), 3)])
def test_decode_bitstreams_in_parts(torch, hip, geom, first_fc):
    """decode_bitstreams_dev of 65532, 65533 and 2 * 65532 + 5 frames from a random prior state, with the part boundaries
    moved by first_frame_count: the oracle's serial decode from that state, and explicit calls of at most 65532 frames
    with the hand-off state (the last frame, the snapshot of the last I-frame) passed in"""
    W, H = geom
    frames, p0, p1, prev, previ = _big(W, H)
    out, sizes = _encoded(torch, hip, W, H)
    exp, pads, _, nent = _oracle_decode(W, H, first_fc, (W, H))
    slab = _with_pads(torch, out, sizes, pads)
    dprev, dprevi = dev_u32(torch, prev), dev_u32(torch, previ)
    npx = W * H
    for N in (PART, PART + 1, 2 * PART + 5) if geom == (8, 8) else (2 * PART + 5,):
        ne = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        pix = hip.decode_bitstreams_dev(slab, sizes, N, W, H, first_fc, nentered=ne, prev=dprev, prev_iframe=dprevi)
        got = to_u32(pix).reshape(N, npx)
        assert (ne.cpu().numpy() == nent[:N]).all(), N
        assert (got == exp[:N]).all(), "N=%d first_fc=%d: frames %s" % (N, first_fc, _bad_frames(got, exp[:N]))
        by_parts = torch.empty_like(pix)
        for f0, f1 in _parts(N, first_fc):
            if f0 == 0:
                a, ai = dprev, dprevi
            else:
                a = by_parts[f0 - 1]
                ai = by_parts[max(f for f in range(f0) if (first_fc + f) % 4 == 0)]
            by_parts[f0:f1] = hip.decode_bitstreams_dev(slab[f0:f1], sizes[f0:f1], f1 - f0, W, H, first_fc + f0, prev=a.contiguous(),
                                                        prev_iframe=ai.contiguous())
        torch.cuda.synchronize()
        assert torch.equal(by_parts, pix), "N=%d first_fc=%d: explicit parts differ" % (N, first_fc)


@pytest.mark.parametrize("N", [65535, 65536])
def test_parse_past_the_grid_limit(torch, hip, monkeypatch, N):
    """parse_dev (more than 65535 frames: the robust kernels alone) and parse_decode_dev at 65535 and 65536 frames:
    offsets below nentered and nentered as AGMV_HIP_PARSE=serial gives them, pixels as the oracle's"""
    W, H = 8, 8
    frames, p0, p1, prev, previ = _big(W, H)
    out, sizes = _encoded(torch, hip, W, H)
    exp, pads, _, nent = _oracle_decode(W, H, 0, (W, H))
    slab = _with_pads(torch, out, sizes, pads)
    dprev, dprevi = dev_u32(torch, prev), dev_u32(torch, previ)
    monkeypatch.setenv("AGMV_HIP_PARSE", "serial")
    o_ser, n_ser = hip.parse_dev(slab, sizes, N, W, H)
    monkeypatch.delenv("AGMV_HIP_PARSE")
    torch.cuda.synchronize()
    assert (n_ser.cpu().numpy() == nent[:N]).all()
    below = torch.arange(W * H // 16, device="cuda")[None, :] < n_ser[:, None]
    o1, n1 = hip.parse_dev(slab, sizes, N, W, H)
    pix1 = hip.decode_dev(slab, sizes, o1, n1, N, W, H, 0, prev=dprev, prev_iframe=dprevi)
    pix2, o2, n2 = hip.parse_decode_dev(slab, sizes, N, W, H, 0, prev=dprev, prev_iframe=dprevi)
    torch.cuda.synchronize()
    for name, o, n, pix in (("parse_dev", o1, n1, pix1), ("parse_decode_dev", o2, n2, pix2)):
        assert torch.equal(n, n_ser), name
        assert torch.equal(o[below], o_ser[below]), name
        got = to_u32(pix).reshape(N, -1)
        assert (got == exp[:N]).all(), "%s: frames %s" % (name, _bad_frames(got, exp[:N]))


@pytest.mark.parametrize("case", ["frame0_cut", "part1_first_cut", "clean"])
def test_prior_dependence_of_a_call_in_parts(torch, hip, case):
    """decode_bitstreams_dev of 65533 frames = two parts (65532 + 1).  The flag is the dependence of the whole call on
    the caller's state: (i) frame 0 cut short: 1; (ii) only the first frame of part 1 cut short -- its stale pixels come
    from part 0's output, inside the call: 0; (iii) clean: 0.  Each against the oracle from S_A / S_B."""
    W, H = 8, 8
    N = PART + 1
    frames, p0, p1, prev, previ = _big(W, H)
    hip.set_palette(p0, p1, True)
    out, sizes = hip.encode_dev(dev_u32(torch, frames[:N]), N, W, H)
    hip.check()
    if case == "frame0_cut":
        sizes[0] = 1
    elif case == "part1_first_cut":
        sizes[PART] = 1
    host, sz = out.cpu().numpy(), sizes.cpu().numpy()
    bits = [host[f, :sz[f]].copy() for f in range(N)]
    m = np.uint32(0xFFFFFF)
    expA, pads, _, _ = T.oracle_range(W, H, True, p0, p1, bits, 0, prev, previ)
    expB = T.oracle_range(W, H, True, p0, p1, bits, 0, prev ^ m, previ ^ m)[0]
    slab = _with_pads(torch, out, sizes, pads)
    pix = hip.decode_bitstreams_dev(slab, sizes, N, W, H, 0, prev=dev_u32(torch, prev), prev_iframe=dev_u32(torch, previ))
    assert (to_u32(pix).reshape(N, -1) == expA).all()
    flag = hip.decode_depends_on_prior(W, H)
    differs = not (expA == expB).all()
    assert differs == (case == "frame0_cut")
    assert flag == differs, "%s: flag %s" % (case, flag)
