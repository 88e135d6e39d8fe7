"""The LZSS stage on the GPU (agmv_hip_lzss_frames_dev / AgmvHip.lzss_frames_dev) against the brute-force restatement
(orc_lzss_compress), the host stage (agmv_lzss_mem) and the closed form of an all-literal stream.  Payloads are the
csize bytes the reference's file holds for a frame."""
import os
import time

import numpy as np
import pytest

import hostlib as H
import lzss_cases as Z
from lzss_cases import gpu_batch, orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    from libagmv_amd import AgmvHip
    assert torch.cuda.is_available()
    h = AgmvHip(0)
    yield h
    h.close()


def small_cases():
    from test_hostlib import lz_cases
    cases = list(lz_cases())
    rng = np.random.default_rng(77)
    for n in (0, 1, 2, 3, 4, 14, 15, 16, 17):
        cases.append(rng.integers(0, 3, n, dtype=np.uint8))
        cases.append(np.zeros(n, np.uint8))
    for p in range(1, 17):                                           # self-overlapping runs of period 1..16
        cases.append(np.tile(rng.integers(0, 256, p, dtype=np.uint8), 2000 // p + 1)[:2000 + p])
    # ties: the 3-gram ABC occurs at 0, 8 and 16 with different followers: at 16 the start 0 must win over 8
    cases.append(np.array([65, 66, 67, 1, 200, 201, 202, 203, 65, 66, 67, 2, 210, 211, 212, 213, 65, 66, 67, 3, 9], np.uint8))
    # equally long (5) matches at 0 and 40 for the copy at 80; and a longer one later must beat an earlier shorter one
    blk = rng.integers(0, 256, 5, dtype=np.uint8)
    t = rng.integers(100, 256, 120, dtype=np.uint8)
    t[0:5] = blk; t[40:45] = blk; t[80:85] = blk
    t[60:67] = np.concatenate([blk, [7, 7]]); t[100:107] = np.concatenate([blk, [7, 7]])
    cases.append(t)
    return cases


def fuzz_case(seed):
    rng = np.random.default_rng(9000 + seed)
    n = int(rng.integers(1, 6000))
    parts, have = [], 0
    while have < n:
        kind = int(rng.integers(0, 5))
        ln = int(rng.integers(1, 400))
        if kind == 0:
            p = rng.integers(0, 256, ln, dtype=np.uint8)
        elif kind == 1:
            p = np.full(ln, [0x5E, 0x4E, 0x2F, 0, 0xFF][int(rng.integers(0, 5))], np.uint8)
        elif kind == 2 and parts:
            src = np.concatenate(parts)
            at = int(rng.integers(0, len(src)))
            p = src[at:at + ln].copy()
        elif kind == 3:
            p = np.tile(rng.integers(0, 256, int(rng.integers(1, 20)), dtype=np.uint8), ln // 4 + 1)[:ln]
        else:
            p = rng.integers(0, 4, ln, dtype=np.uint8) + np.uint8(0x4C)
        parts.append(p)
        have += len(p)
    return np.concatenate(parts)[:n]


@pytest.mark.parametrize("case", range(len(small_cases())))
def test_small_cases_match_brute_force(hip, case):
    x = small_cases()[case]
    got = hip.lzss_frames([x])[0]
    exp = orc(x)
    assert len(got) == len(exp) and (got == exp).all()


@pytest.mark.parametrize("seed", range(int(os.environ.get("AGMV_FUZZ_SEEDS", "24"))))
def test_fuzz_matches_brute_force(hip, seed):
    x = fuzz_case(seed)
    got = hip.lzss_frames([x])[0]
    exp = orc(x)
    assert len(got) == len(exp) and (got == exp).all(), seed


def test_one_batched_call_mixed_sizes(hip):
    streams = small_cases() + [fuzz_case(s) for s in range(int(os.environ.get("AGMV_FUZZ_SEEDS", "24")))]
    streams.insert(3, np.zeros(0, np.uint8))
    got = gpu_batch(hip, streams, stride_extra=333, out_extra=77)
    for i, x in enumerate(streams):
        exp = orc(x)
        assert len(got[i]) == len(exp) and (got[i] == exp).all(), i


@pytest.mark.parametrize("dist", [65535, 65536])
def test_window_edge(hip, dist):
    """a 15-byte repeat at distance 65535 is a match, at 65536 it is out of the window"""
    rng = np.random.default_rng(dist)
    blk = rng.integers(0, 256, 15, dtype=np.uint8)
    x = np.concatenate([blk, rng.integers(0, 256, dist - 15, dtype=np.uint8), blk])
    got = hip.lzss_frames([x])[0]
    exp, ecs = H.lzss(x)
    assert len(got) == ecs and (got == exp).all()
    tail = np.concatenate([blk, [0]]).astype(np.uint8)
    y = np.concatenate([x[:dist], tail])                           # same prefix, no repeat at the end
    base, bcs = H.lzss(y)
    if dist == 65535:
        assert ecs < bcs                                             # one 21-bit token replaced 15 literals
    else:
        assert ecs >= bcs - 1


def encode_bitstreams(hip, frames_dev, n, W, H_, quality=1):
    import torch
    hist = hip.histogram_dev(frames_dev.reshape(-1), quality)
    torch.cuda.synchronize()
    hist_np = hist.cpu().numpy().view(np.uint32)
    p0 = np.zeros(256, np.uint64)
    p1 = np.zeros(256, np.uint64)
    H.lib().AGMV_BuildPalette(hist_np, quality, 3, p0, p1)
    hip.set_palette(p0.astype(np.uint32), p1.astype(np.uint32), True)
    out, sizes = hip.encode_dev(frames_dev, n, W, H_)
    hip.check()
    return out, sizes


def check_against_host(hip, out, sizes, n):
    import torch
    pay, cs = hip.lzss_frames_dev(out, sizes, n)
    torch.cuda.synchronize()
    pay = pay.cpu().numpy()
    cs = cs.cpu().numpy().view(np.uint32)
    bits = out.cpu().numpy()
    sz = sizes.cpu().numpy().view(np.uint32)
    for f in range(n):
        exp, ecs = H.lzss(bits[f, :sz[f]])
        assert cs[f] == ecs, f
        assert (pay[f, :ecs] == exp).all(), f
    return sz, cs


def test_c3_shaped_1080p_bitstreams(hip):
    W, H_, n = 1920, 1080, 64
    frames = hip.synth_dev(W, H_, 0, n)
    out, sizes = encode_bitstreams(hip, frames, n, W, H_)
    check_against_host(hip, out, sizes, n)


def test_foxlogo_bitstreams(hip, foxlogo):
    import torch
    fr = foxlogo["frames"]
    n, H_, W = fr.shape[:3]
    hip.set_palette(foxlogo["p0"], foxlogo["p1"], True)
    d = torch.from_numpy(np.ascontiguousarray(fr.reshape(n, H_, W)).view(np.int32)).cuda()
    out, sizes = hip.encode_dev(d, n, W, H_)
    hip.check()
    check_against_host(hip, out, sizes, n)


def test_normal_heavy_noise_frames_csize_tail(hip):
    """noise at 1080p: NORMAL-heavy frames of > 3 MB pre-LZ, > 2^24 output bits: the float csize rule decides the last byte"""
    import torch
    W, H_, n = 1920, 1080, 4
    rng = np.random.default_rng(11)
    frames = torch.from_numpy(rng.integers(0, 1 << 24, (n, H_, W), dtype=np.int64).astype(np.int32)).cuda()
    out, sizes = encode_bitstreams(hip, frames, n, W, H_)
    sz, cs = check_against_host(hip, out, sizes, n)
    assert (sz >= 3_000_000).all() and (cs.astype(np.int64) * 8 >= 1 << 24).all()


def test_all_literal_tail_stream(hip):
    x = Z.all_literal_stream()
    exp, ecs = Z.literal_payload(x)
    got = gpu_batch(hip, [x], stride_extra=5)[0]
    assert len(got) == ecs == 9 * len(x) // 8 + 1
    assert (got == exp).all()


@pytest.mark.parametrize("shape", ["zero", "period2", "period15", "noise"])
def test_worst_cases_finish_and_match_host(hip, shape):
    rng = np.random.default_rng(5)
    if shape == "zero":
        x = np.zeros(4 << 20, np.uint8)
    elif shape == "noise":
        x = rng.integers(0, 256, 4_300_000, dtype=np.uint8)
    else:
        p = int(shape[6:])
        x = np.tile(rng.integers(0, 256, p, dtype=np.uint8), (4 << 20) // p + 1)[:4 << 20]
    t0 = time.time()
    got = hip.lzss_frames([x])[0]
    dt = time.time() - t0
    exp, ecs = H.lzss(x)
    assert len(got) == ecs and (got == exp).all()
    assert dt < 60, dt
