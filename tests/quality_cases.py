"""The measurement of include/agmv.h ("measuring a decoded clip") stated in numpy and Python integers, the shift-and-subtract
division the kernel uses, a float64 SSIM of the same windows, and the clips the tests share (tests/test_quality_cpu.py on the
CPU, tests/test_gpu_quality*.py on the GPU).  No float in the statement: the Q20 value of a window is (num << 20) // den in Python
integers."""
import os
import re

import numpy as np

import dither_cases as D
import scale_cases as SC

C1 = 26634                                      # floor(0.01^2 * 255^2 * 64^2 + 0.5)
C2 = 235963                                     # floor(0.03^2 * 255^2 * 64 * 63 + 0.5)
ONE = 1 << 20
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def windows(w, h):
    """SSIM windows per frame and channel"""
    return (w // 4 - 1) * (h // 4 - 1)


def window_moments(test, ref):
    """uint32 [n, h, w] twice -> (s1, s2, ss, s12), int64 [n, h/4 - 1, w/4 - 1, 3]: the sums over the 8x8 windows at stride 4"""
    a, b = D.channels(test), D.channels(ref)
    n, h, w, _ = a.shape

    def win(x):
        m = x.reshape(n, h // 4, 4, w // 4, 4, 3).sum(axis=(2, 4))
        return m[:, :-1, :-1] + m[:, :-1, 1:] + m[:, 1:, :-1] + m[:, 1:, 1:]
    return win(a), win(b), win(a * a) + win(b * b), win(a * b)


def num_den(s1, s2, ss, s12):
    """int64 arrays: |num| <= den < 2^58, both fit"""
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    cov = 64 * s12 - s1 * s2
    return (2 * s1 * s2 + C1) * (2 * cov + C2), (s1 * s1 + s2 * s2 + C1) * (vars_ + C2)


def q20(num, den):
    """floor(num * 2^20 / den) towards minus infinity, in Python integers; object arrays"""
    return (np.asarray(num).astype(object) << 20) // np.asarray(den).astype(object)


def q20_shift_subtract(num, den):
    """the same value for one window by 20 shift-and-subtract steps on magnitudes below 2^64, as the kernel computes it"""
    num, den = int(num), int(den)
    mag = abs(num)
    assert 0 < den < 1 << 58 and mag <= den
    q = 1 if mag >= den else 0
    r = mag - q * den
    for _ in range(20):
        r <<= 1
        q <<= 1
        assert r < 1 << 59
        if r >= den:
            r -= den
            q |= 1
    return -q - (1 if r else 0) if num < 0 else q


def window_values(test, ref):
    """the Q20 value of every window: object array [n, h/4 - 1, w/4 - 1, 3]"""
    return q20(*num_den(*window_moments(test, ref)))


def float_ssim(test, ref):
    """float64 SSIM of the same windows with the same constants: [n, h/4 - 1, w/4 - 1, 3]"""
    s1, s2, ss, s12 = (x.astype(np.float64) for x in window_moments(test, ref))
    vars_, cov = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
    return (2 * s1 * s2 + C1) * (2 * cov + C2) / ((s1 * s1 + s2 * s2 + C1) * (vars_ + C2))


def measure(test, ref):
    """test, ref: uint32 [n, h, w] (bits >= 24 ignored), w and h multiples of 4 -> {"sse", "block_sse", "max_err", "ssim"}: int64 [n, 3]"""
    test, ref = np.asarray(test, np.uint32), np.asarray(ref, np.uint32)
    assert test.shape == ref.shape and test.ndim == 3 and test.shape[1] % 4 == 0 and test.shape[2] % 4 == 0
    n = test.shape[0]
    a, b = D.channels(test), D.channels(ref)
    d = a - b
    bs = D.block_sums(test) - D.block_sums(ref)
    v = window_values(test, ref).reshape(n, -1, 3)
    ssim = np.array([[sum(v[f, :, c].tolist()) for c in range(3)] for f in range(n)], np.int64).reshape(n, 3)
    return {"sse": (d * d).sum(axis=(1, 2)), "block_sse": (bs * bs).sum(axis=(1, 2)), "max_err": np.abs(d).max(axis=(1, 2)) if d.size else np.zeros((n, 3), np.int64),
            "ssim": ssim}


def entries(q):
    """the statement's result as the words of AGMV_FRAME_QUALITY: uint64 [n, 12] (the signed sums as their two's complement)"""
    return np.concatenate([q["sse"], q["block_sse"], q["max_err"], q["ssim"]], axis=1).astype(np.int64).view(np.uint64)


# ---- clips
def noise(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 1 << 24, (n, h, w)).astype(np.uint32)


def perturbed(pix, seed, amount=3):
    """every channel moved by -amount .. amount, clipped; frame f by at most amount + f, so that no two frames have the same error"""
    rng = np.random.default_rng(seed)
    c = D.channels(pix)
    step = amount + np.arange(c.shape[0]).reshape(-1, 1, 1, 1)
    c = np.clip(c + rng.integers(-64, 65, c.shape) * step // 64, 0, 255)
    return (c[..., 0] << 16 | c[..., 1] << 8 | c[..., 2]).astype(np.uint32)


def complement(pix):
    return np.asarray(pix, np.uint32) ^ np.uint32(0xFFFFFF)


def checkerboard(n, h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.broadcast_to(np.where((x + y) & 1, 0xFFFFFF, 0).astype(np.uint32), (n, h, w)).copy()


def reference_clip(fmt, pix):
    """uint32 [n, h, w] -> (the clip in the layout fmt as uint8 [n, frame bytes], the XRGB32 clip it stands for): the writing of
    a YUV layout is lossy, so the clip that is compared is the one the layout's reading rule gives back"""
    n, h, w = pix.shape
    raw = np.ascontiguousarray(SC.from_packed(fmt, pix)).view(np.uint8).reshape(n, -1)
    return raw, SC.to_packed(fmt, raw, w, h)


def kernel_grid():
    """the most workgroups a launch of k_measure has: with more items than that, a workgroup walks several"""
    src = open(os.path.join(ROOT, "libagmv_amd", "csrc", "agmv_clip_hip.hip")).read()
    return int(re.search(r"k_measure, \(unsigned\)\(A\.items < (\d+) \? A\.items : \1\)", src).group(1))


def kernel_tile():
    """(blocks per tile row, per tile column) of k_measure, read from its source"""
    src = open(os.path.join(ROOT, "libagmv_amd", "csrc", "agmv_clip_hip.hip")).read()
    return int(re.search(r"#define MS_TW (\d+)", src).group(1)), int(re.search(r"#define MS_TH (\d+)", src).group(1))
