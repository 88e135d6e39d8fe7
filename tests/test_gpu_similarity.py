"""The two per-pixel jobs of the memory sequences, through AgmvHip: agmv_hip_similarity_dev (the integer behind
AGMV_CompareFrameSimilarity, for every adjacent pair of a clip) and agmv_hip_gather_dev (the GBA / NDS nearest scale as a
gather).  Exact integers against numpy; the counts also against the host library's AGMV_CompareFrameSimilarity.  Needs an MI355X."""

import numpy as np
import pytest

import hostlib as H

pytestmark = pytest.mark.gpu


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


def grey(p):
    p = p.astype(np.uint32)
    return (((p >> 16) & 255) + ((p >> 8) & 255) + (p & 255)) // 3


def expected_counts(frames):
    g = grey(frames.reshape(frames.shape[0], -1))
    return (g[:-1] == g[1:]).sum(1).astype(np.uint32)


def gpu_counts(torch, hip, frames, counts=None):
    out = hip.similarity_dev(dev_u32(torch, frames), counts)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def host_counts(frames):
    """count = ratio * npx from the host library's AGMV_CompareFrameSimilarity (8-byte pixels): exact below 2^23 pixels, where the
    float ratio is off by less than half a pixel"""
    L = H.lib()
    fl = [np.ascontiguousarray(f.reshape(-1)).astype(np.uint64) for f in frames]
    npx = fl[0].size
    assert npx < 1 << 23
    return np.array([int(np.rint(float(L.AGMV_CompareFrameSimilarity(fl[k], fl[k + 1], npx, 1)) * npx)) for k in range(len(fl) - 1)], np.uint32)


def random_clip(rng, n, npx):
    """each frame keeps about half of the frame before it, so the counts are neither 0 nor npx; garbage in bits 24-31"""
    fr = np.empty((n, npx), np.uint32)
    fr[0] = rng.integers(0, 1 << 24, npx, dtype=np.uint32)
    for f in range(1, n):
        keep = rng.random(npx) < 0.5
        fr[f] = np.where(keep, fr[f - 1], rng.integers(0, 1 << 24, npx, dtype=np.uint32))
    return fr | (rng.integers(0, 256, (n, npx), dtype=np.uint32) << 24)


# 1 pixel; a quarter, three quarters, one short of, exactly and one past a wave of lanes (4 pixels each is the vector width: 63
# and 65 are not multiples of it); a frame of the small goldens; 2052 * 4 = one block of 2048 pixels and a tail, past it
@pytest.mark.parametrize("npx", [1, 16, 48, 63, 64, 65, 160 * 128, 2052 * 4])
@pytest.mark.parametrize("n", [2, 3, 9])
def test_similarity_counts_random_frames(torch, hip, n, npx):
    fr = random_clip(np.random.default_rng(1000 * n + npx), n, npx)
    exp = expected_counts(fr)
    assert (gpu_counts(torch, hip, fr) == exp).all()
    assert (host_counts(fr) == exp).all()


def test_similarity_counts_many_workgroups_per_frame(torch, hip):
    fr = random_clip(np.random.default_rng(5), 9, 1920 * 1080)
    exp = expected_counts(fr)
    assert 0 < exp.min() and exp.max() < 1920 * 1080
    assert (gpu_counts(torch, hip, fr) == exp).all()
    assert (host_counts(fr[:3]) == exp[:2]).all()


@pytest.mark.parametrize("npx", [65, 2052 * 4])
def test_similarity_identical_and_disjoint_frames(torch, hip, npx):
    rng = np.random.default_rng(npx)
    a = rng.integers(0, 1 << 24, npx, dtype=np.uint32)
    assert (gpu_counts(torch, hip, np.stack([a, a | 0xFF000000, a])) == npx).all()
    lo = rng.integers(0, 100, (npx, 3), dtype=np.uint32)           # greys 0..99 against greys 150..255
    hi = rng.integers(150, 256, (npx, 3), dtype=np.uint32)
    pack = lambda c: c[:, 0] << 16 | c[:, 1] << 8 | c[:, 2]
    assert (gpu_counts(torch, hip, np.stack([pack(lo), pack(hi), pack(lo)])) == 0).all()


def split_sum(s, order):
    """a colour whose channels add up to s, filled in the given channel order"""
    c = [0, 0, 0]
    for k in order:
        c[k] = min(s, 255)
        s -= c[k]
    return c[0] << 16 | c[1] << 8 | c[2]


def test_similarity_grey_edges(torch, hip):
    """every channel sum 0..765 against the sums 1 and 2 below and above it, the channels split differently in the two frames:
    the pair is equal exactly where both sums have the same third"""
    a, b = [], []
    for s in range(766):
        for d in (-2, -1, 1, 2):
            if 0 <= s + d <= 765:
                a.append(split_sum(s, (0, 1, 2)))
                b.append(split_sum(s + d, (2, 1, 0)))
    fr = np.array([a, b], np.uint32)
    exp = expected_counts(fr)
    assert 0 < exp[0] < len(a)
    assert (gpu_counts(torch, hip, fr) == exp).all()
    assert (host_counts(fr) == exp).all()


def test_similarity_overwrites_its_counts(torch, hip):
    rng = np.random.default_rng(9)
    first, second = random_clip(rng, 5, 4099), random_clip(rng, 5, 4099)
    counts = torch.full((4,), 123456, dtype=torch.int32, device="cuda")
    assert (gpu_counts(torch, hip, first, counts) == expected_counts(first)).all()
    assert (gpu_counts(torch, hip, second, counts) == expected_counts(second)).all()      # not cleared in between


def test_similarity_of_a_clip_that_is_not_16_byte_aligned(torch, hip):
    """frames of a multiple of 4 pixels behind a base 4 bytes past a 16-byte boundary: the 16-byte loads cannot be used"""
    fr = random_clip(np.random.default_rng(3), 3, 2048 + 64)
    buf = torch.zeros(fr.size + 1, dtype=torch.int32, device="cuda")
    buf[1:] = dev_u32(torch, fr).reshape(-1)
    clip = buf[1:].view(3, -1)
    assert clip.data_ptr() % 16 == 4
    out = hip.similarity_dev(clip)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == expected_counts(fr)).all()


@pytest.mark.parametrize("n_out", [1, 9600, 12288])
def test_gather_matches_fancy_indexing(torch, hip, n_out):
    rng = np.random.default_rng(n_out)
    src_px = 1000 * 77 + 3                                         # not a multiple of 64
    src = rng.integers(0, 1 << 32, (3, src_px), dtype=np.uint32)
    index = rng.integers(0, src_px, n_out, dtype=np.uint32)
    none = rng.random(n_out) < 0.2
    index[none] = 0xFFFFFFFF
    exp = np.where(none[None, :], 0, src[:, np.where(none, 0, index)])
    out = hip.gather_dev(dev_u32(torch, src), dev_u32(torch, index))
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == exp).all()


def test_gather_reads_nothing_outside_the_source_frame(torch, hip):
    src = np.arange(1, 3 * 100 + 1, dtype=np.uint32).reshape(3, 100)
    index = np.array([0, 99, 100, 0x7FFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    out = hip.gather_dev(dev_u32(torch, src), dev_u32(torch, index))
    torch.cuda.synchronize()
    exp = np.stack([[f[0], f[99], 0, 0, 0, 0] for f in src]).astype(np.uint32)
    assert (out.cpu().numpy().view(np.uint32) == exp).all()
