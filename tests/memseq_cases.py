"""Clips of the memory-sequence tests (tests/test_gpu_memseq.py) and of their fixture generator
(tests/golden/make_golden_memseq.py): one statement of the frames, so both see the same pixels."""
import numpy as np

import synth as S

# the mixed adaptive clip: AGMV_EncodeVideo's frame skipping takes BOTH branches on it (the two older EncodeVideo goldens take
# the "similar" branch in every group)
MIXED_W, MIXED_H, MIXED_T = 160, 128, 26
MIXED_NOISE = (2, 3, 6, 11, 12, 13, 18, 22)
# name -> (opt, quality, compression): LOW quality, LZSS; leniency 0.2282 (OPT_III, OPT_I) and 0.1282 (OPT_II)
MIXED_CASES = {"mixed_video_opt3_low_lzss_160x128": (3, 3, 1), "mixed_video_opt1_low_lzss_160x128": (1, 3, 1),
               "mixed_video_opt2_low_lzss_160x128": (2, 3, 1)}


def synth_clip(W, H, T):
    """frames 1..T of the canonical clip, as the file goldens number them (f<t>.bmp = synth_frame(W, H, t))"""
    return np.stack([S.synth_frame(W, H, t) for t in range(1, T + 1)])


def mixed_clip():
    """[26, 128, 160] uint32: synth_frame(W, H, t) for t = 1..26 with the frames t of MIXED_NOISE replaced by uniform noise
    (one generator, seed 7, drawn in that order)"""
    fr = synth_clip(MIXED_W, MIXED_H, MIXED_T)
    rng = np.random.default_rng(7)
    for t in MIXED_NOISE:
        fr[t - 1] = rng.integers(0, 1 << 24, size=(MIXED_H, MIXED_W), dtype=np.uint32)
    return fr


def adaptive_chain(similar, n, heavy):
    """the steps of AGMV_EncodeVideo's loop over frames 1..n (reference src/agmv_encode.c:719-2268): similar(x) says whether
    the pair of frames (x, x + 1) passes.  Returns the list of decisions taken."""
    out, i = [], 1
    while i <= n:
        ok = bool(similar(i if heavy else i + 1))
        out.append(ok)
        i += (2 if heavy else 4) if ok else 1
        if i + 4 >= n:
            break
    return out
