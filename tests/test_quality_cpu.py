"""The measurement of include/agmv.h ("measuring a decoded clip") as tests/quality_cases.py states it: the values the definition
fixes by hand, the existing block-sum measure of the dither, the shift-and-subtract division against Python integers and a
float64 SSIM of the same windows.  The refusals of the two public calls come before a device is opened and are checked here too.
No GPU."""
import ctypes as C

import numpy as np
import pytest

import dither_cases as D
import hostlib as H
import quality_cases as Q


def test_equal_clips():
    pix = Q.noise(1, 3, 12, 20)
    q = Q.measure(pix | np.uint32(0x5A000000), pix)             # bits >= 24 are ignored
    assert (q["sse"] == 0).all() and (q["block_sse"] == 0).all() and (q["max_err"] == 0).all()
    assert (q["ssim"] == Q.windows(20, 12) * Q.ONE).all() and Q.windows(20, 12) == 8
    assert (Q.window_values(pix, pix) == Q.ONE).all()


def test_no_window_at_width_or_height_4():
    for h, w in ((4, 4), (4, 8), (8, 4)):
        q = Q.measure(Q.noise(2, 2, h, w), Q.noise(3, 2, h, w))
        assert Q.windows(w, h) == 0 and (q["ssim"] == 0).all() and (q["sse"] > 0).all()


def test_black_against_white():
    """0 against 255: s1 = 0, s2 = 64 * 255, vars = cov = 0, so the value is floor(C1 * 2^20 / (s2^2 + C1)); the SSE of one 320x240
    frame does not fit 32 bits"""
    z = np.zeros((1, 240, 320), np.uint32)
    q = Q.measure(z, Q.complement(z))
    assert (q["sse"] == 320 * 240 * 255 * 255).all() and 320 * 240 * 255 * 255 == 4993920000 > 1 << 32
    assert (q["block_sse"] == 80 * 60 * (16 * 255) ** 2).all() and (q["max_err"] == 255).all()
    value = (26634 << 20) // ((64 * 255) ** 2 + 26634)
    assert value == 104
    assert (q["ssim"] == 79 * 59 * value).all()


def test_checkerboard_against_its_inverse():
    """s1 = s2 = 32 * 255, s12 = 0: cov = -s1^2, vars = 2 * s1^2; a negative value, floored towards minus infinity"""
    cb = Q.checkerboard(1, 8, 8)
    v = Q.window_values(cb, Q.complement(cb))
    s = (32 * 255) ** 2
    num, den = (2 * s + Q.C1) * (Q.C2 - 2 * s), (2 * s + Q.C1) * (2 * s + Q.C2)
    assert v.shape == (1, 1, 1, 3) and (v == (num << 20) // den).all()
    assert round(int(v[0, 0, 0, 0]) / Q.ONE, 5) == -0.99646
    assert -((-num << 20) // den) != (num << 20) // den         # (truncation towards zero would give another word)
    q = Q.measure(cb, Q.complement(cb))
    assert (q["block_sse"] == 0).all() and (q["sse"] == 64 * 255 * 255).all()


def test_block_sse_is_the_dither_measure():
    """summed over the channels it is dither_cases.block_sum_error, on the clips that module crafts and on the golden frame"""
    fox = D.fox()[0][D.FOX_FRAME:D.FOX_FRAME + 1]
    clips = [(fox, Q.perturbed(fox, 4, 9))]
    for _, _, frames, in D.crafted().values():
        n, h, w = frames.shape
        if h % 4 == 0 and w % 4 == 0:
            clips.append((frames, Q.noise(5, n, h, w)))
    assert len(clips) >= 3
    for out, src in clips:
        assert int(Q.measure(out, src)["block_sse"].sum()) == D.block_sum_error(out, src)


def windows_of_every_kind():
    base = Q.noise(6, 4, 24, 24)
    cb = Q.checkerboard(1, 24, 24)
    flat = np.full((1, 24, 24), 0x808080, np.uint32)
    pairs = [(base, Q.perturbed(base, 7)), (base, Q.complement(base)), (base, Q.noise(8, 4, 24, 24)), (cb, Q.complement(cb)), (cb, flat),
             (np.zeros_like(flat), Q.complement(np.zeros_like(flat))), (flat, flat), (base[:1], cb), (flat, Q.perturbed(flat, 9, 1))]
    return pairs


def test_shift_and_subtract_division_is_the_floor():
    seen_negative = seen_one = 0
    for a, b in windows_of_every_kind():
        num, den = Q.num_den(*Q.window_moments(a, b))
        assert (den > 0).all() and (np.abs(num) <= den).all() and int(den.max()) < 1 << 58
        want = Q.q20(num, den).reshape(-1)
        for nu, de, wv in zip(num.reshape(-1).tolist(), den.reshape(-1).tolist(), want.tolist()):
            assert Q.q20_shift_subtract(nu, de) == wv == (nu << 20) // de
            seen_negative += nu < 0
            seen_one += wv == Q.ONE
    assert seen_negative and seen_one
    # remainders of every kind, away from image statistics
    rng = np.random.default_rng(10)
    for _ in range(2000):
        de = int(rng.integers(1, 1 << 58))
        nu = int(rng.integers(-de, de + 1))
        assert Q.q20_shift_subtract(nu, de) == (nu << 20) // de
    assert Q.q20_shift_subtract(-1, 3) == -349526 and Q.q20_shift_subtract(-3, 3) == -Q.ONE and Q.q20_shift_subtract(0, 5) == 0


def test_float64_ssim_agrees_to_one_q20_step():
    for a, b in windows_of_every_kind():
        f = Q.float_ssim(a, b)
        v = Q.window_values(a, b).astype(np.float64) / Q.ONE
        assert np.abs(f - v).max() <= 2.0 ** -20


# ---- the public calls refuse before a device is opened (this host has none)
from libagmv_amd.abi import AGMV_FRAME_QUALITY as QUALITY, AGMV_INFO as INFO  # noqa: E402

lib = H.lib


def test_entry_is_96_bytes():
    assert C.sizeof(QUALITY) == 96


def test_measure_frames_refuses_before_a_device_is_opened():
    L = lib()
    q = (QUALITY * 2)()
    fake = C.c_void_p(0x1000)                                   # never dereferenced: every call below returns before the device is opened
    for fmt in (0, 6, 18, 0x101, 16 | 0x400):
        assert L.AGMV_MeasureFramesDev(fake, fake, fmt, 2, 8, 8, q) == -1
    assert L.AGMV_MeasureFramesDev(None, fake, 1, 2, 8, 8, q) == -1
    assert L.AGMV_MeasureFramesDev(fake, None, 1, 2, 8, 8, q) == -1
    assert L.AGMV_MeasureFramesDev(fake, fake, 1, 2, 8, 8, None) == -1
    for w, h in ((6, 8), (8, 6), (0, 8), (8, 0), (1 << 16, 1 << 16)):
        assert L.AGMV_MeasureFramesDev(fake, fake, 1, 2, w, h, q) == -3
    assert L.AGMV_MeasureFramesDev(fake, fake, 16, 2, 6, 6, q) == -3           # an odd-sized YUV clip is no multiple of 4 either
    assert L.AGMV_MeasureFramesDev(fake, fake, 2, 0, 8, 8, q) == 0             # no frame: nothing to do


def test_measure_file_refuses_before_a_device_is_opened(tmp_path):
    L = lib()
    q = (QUALITY * 2)()
    fake = C.c_void_p(0x1000)
    missing = str(tmp_path / "missing.agmv").encode()
    assert L.AGMV_MeasureFileDev(missing, fake, 6, 2, q, None) == -1
    assert L.AGMV_MeasureFileDev(missing, None, 1, 2, q, None) == -1
    assert L.AGMV_MeasureFileDev(missing, fake, 1, 2, q, None) == -2           # FILE_NOT_FOUND_ERR, negated
    assert L.AGMV_MeasureFileDev(None, fake, 1, 2, q, None) == -2


def test_measure_file_reads_the_header_and_refuses_what_cannot_correspond(tmp_path):
    """on a file of the goldens: the info-only call, a frame count that is not the header's, and -- with the header's width made odd
    by hand -- a YUV reference that such a size cannot hold; all before a device is opened"""
    import os
    L = lib()
    q = (QUALITY * 1)()
    fake = C.c_void_p(0x1000)
    data = open(os.path.join(D.GOLDEN, "agmv_splash.agmv"), "rb").read()
    n, w, h = (int.from_bytes(data[k:k + 4], "little") for k in (4, 8, 12))
    good = str(tmp_path / "good.agmv").encode()
    open(good, "wb").write(data)
    info = INFO()
    assert L.AGMV_MeasureFileDev(good, None, 1, 0, None, C.byref(info)) == 0
    assert (info.number_of_frames, info.width, info.height) == (n, w, h) and n > 1 and w % 4 == 0 and h % 4 == 0
    for fmt in (1, 2, 16):
        assert L.AGMV_MeasureFileDev(good, fake, fmt, n - 1, q, None) == -3
        assert L.AGMV_MeasureFileDev(good, fake, fmt, n + 1, q, None) == -3
    odd = str(tmp_path / "odd.agmv").encode()
    open(odd, "wb").write(data[:8] + (w - 1).to_bytes(4, "little") + data[12:])
    info = INFO()
    for fmt in (16, 17 | 0x300):
        assert L.AGMV_MeasureFileDev(odd, fake, fmt, n, q, C.byref(info)) == -3 and info.width == w - 1
    assert L.AGMV_MeasureFileDev(odd, fake, 16, n, None, None) == 0            # info only: nothing is refused


def test_python_names_are_exported():
    import libagmv_amd
    from libagmv_amd import seq
    assert libagmv_amd.clip_quality is seq.clip_quality and libagmv_amd.file_quality is seq.file_quality
    n = 2
    e = (seq.AGMV_FRAME_QUALITY * n)()
    assert C.sizeof(seq.AGMV_FRAME_QUALITY) == 96
    for f in range(n):
        for c in range(3):
            e[f].sse[c], e[f].block_sse[c], e[f].max_err[c], e[f].ssim[c] = 100 * f + c, 1000 * f + c, 7 + c, -(1 << 20) * (f + 1)
    r = seq.Quality(e, n, 8, 8)
    assert r.sse.dtype == np.int64 and r.sse.shape == r.block_sse.shape == r.max_err.shape == r.ssim_sum.shape == (2, 3)
    assert r.sse.tolist() == [[0, 1, 2], [100, 101, 102]] and r.max_err.tolist() == [[7, 8, 9]] * 2 and r.ssim_sum[1, 2] == -(2 << 20)
    assert r.ssim() == pytest.approx(-1.5) and r.psnr() == pytest.approx(10 * np.log10(255.0 ** 2 * 2 * 64 * 3 / 306))
    assert r.block_psnr() == pytest.approx(10 * np.log10(255.0 ** 2 * 2 * 4 * 3 * 256 / 3006))
    z = seq.Quality((seq.AGMV_FRAME_QUALITY * 1)(), 1, 4, 8)
    assert z.psnr() == float("inf") and z.block_psnr() == float("inf") and np.isnan(z.ssim())
