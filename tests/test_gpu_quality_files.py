"""AGMV_MeasureFileDev against AGMV_MeasureFramesDev on the decoded clip, and libagmv_amd.seq's clip_quality / file_quality on
torch tensors.

A 21-frame 64 x 48 clip is written with AGMV_SCHEDULE_FULL, LZSS and LZ77.  Measuring the file -- decoded in three batches of 8
with the decoder's state carried across them, never held as a clip -- must give, entry for entry, what clip_quality gives for
decode_frames(path) and what the numpy statement (tests/quality_cases.py) gives for those pixels, with the host LZ stage and with
AGMV_LZ_DECODE_DEVICE=1, for a reference in XRGB32, RGB24 and NV12; ten frames of 36 x 20 repeat it at a width that is no
multiple of 16.  One child process does all of it (the drivers keep process-wide state and read their knobs from the
environment); the tests read its answer.  Needs an MI355X."""
import functools
import os
import tempfile
import textwrap

import pytest

import children as K

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
N, W, HT = 21, 64, 48
REFS = ["xrgb32", "rgb24", "nv12"]

CHILD = textwrap.dedent("""
    import ctypes as C, json, os, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"]); sys.path.insert(0, job["tests"])
    import libagmv_amd
    from libagmv_amd import seq
    import quality_cases as Q
    N, W, HT = job["n"], job["w"], job["h"]
    rng = np.random.default_rng(180)
    y, x = np.mgrid[0:HT, 0:W]
    t = np.arange(N).reshape(N, 1, 1)
    ch = lambda v: (v + rng.integers(0, 6, (N, HT, W))) & 255              # gradients that move, with a little noise: every block kind
    src = (ch(4 * x + 3 * t) << 16 | ch(5 * y + t) << 8 | ch(x + y + 7 * t)).astype(np.uint32)
    src[:, 32:, :16] = src[0, 32:, :16]                                   # and a part that stands still
    FMT = {"xrgb32": 1, "rgb24": 2, "nv12": 16}
    refs = {}
    for name, v in FMT.items():
        raw, stands_for = Q.reference_clip(v, src)
        shape = {1: (N, HT, W), 2: (N, HT, W, 3), 16: (N, HT * 3 // 2, W)}[v]
        tens = torch.from_numpy(raw.view(np.uint32).view(np.int32) if v == 1 else raw).reshape(shape).cuda()
        refs[name] = (v, tens, stands_for)
    L = seq.load_library()
    words = lambda e, n: np.frombuffer(e, dtype=np.uint64, count=12 * n).reshape(n, 12)
    of = lambda q: np.concatenate([q.sse, q.block_sse, q.max_err, q.ssim_sum], axis=1).view(np.uint64)
    res = {"cases": {}}
    frames = torch.from_numpy(src.view(np.int32)).cuda()
    for cname, comp in (("lzss", 1), ("lz77", 2)):
        path = cname + ".agmv"
        seq.encode_frames(path, frames, opt=3, quality=3, compression=comp, schedule=seq.SCHEDULE_FULL)
        for lz_dev in ("0", "1"):
            os.environ["AGMV_LZ_DECODE_DEVICE"] = lz_dev
            decoded, info = seq.decode_frames(path)
            dec = decoded.cpu().numpy().view(np.uint32)
            for name, (v, tens, stands_for) in refs.items():
                a = seq.clip_quality(decoded, tens, fmt=name)
                e = (seq.AGMV_FRAME_QUALITY * N)()
                rc = L.AGMV_MeasureFileDev(path.encode(), tens.data_ptr(), v, N, e, None)
                b = seq.file_quality(path, tens, fmt=name)
                want = Q.entries(Q.measure(dec, stands_for))
                res["cases"]["%s-%s-%s" % (cname, lz_dev, name)] = {
                    "rc": rc, "frames": int(info.number_of_frames), "decoded": list(decoded.shape),
                    "file_is_clip": bool((words(e, N) == of(a)).all()), "clip_is_statement": bool((of(a) == want).all()),
                    "seq_file_is_file": bool(len(b) == N and (of(b) == words(e, N)).all()),
                    "lossy": bool((a.sse.sum(axis=1) > 0).all()), "psnr": [a.psnr(), b.psnr()], "block_psnr": a.block_psnr(), "ssim": a.ssim(),
                    "dims": [a.width, a.height, b.width, b.height]}
    os.environ["AGMV_LZ_DECODE_DEVICE"] = "0"
    # the refusals and the info-only call, on the real file and a real reference
    v, tens, _ = refs["nv12"]
    e = (seq.AGMV_FRAME_QUALITY * (N + 1))()
    info = seq.AGMV_INFO()
    data = open("lzss.agmv", "rb").read()
    open("odd.agmv", "wb").write(data[:12] + (HT - 1).to_bytes(4, "little") + data[16:])
    res["count_low"] = L.AGMV_MeasureFileDev(b"lzss.agmv", tens.data_ptr(), v, N - 1, e, None)
    res["count_high"] = L.AGMV_MeasureFileDev(b"lzss.agmv", tens.data_ptr(), v, N + 1, e, None)
    res["odd_yuv"] = L.AGMV_MeasureFileDev(b"odd.agmv", tens.data_ptr(), v, N, e, None)
    res["info_only"] = [L.AGMV_MeasureFileDev(b"lzss.agmv", None, v, 0, None, C.byref(info)), int(info.number_of_frames), int(info.width), int(info.height)]
    res["untouched"] = bool((words(e, N + 1) == 0).all())
    same = seq.clip_quality(frames, refs["rgb24"][1])                     # the layout inferred; a clip against itself
    res["same"] = [int(same.sse.sum()), same.psnr(), same.ssim(), int(same.ssim_sum.min()), same.windows]
    try:
        seq.clip_quality(frames[:5], refs["rgb24"][1])
        res["mismatch"] = "accepted"
    except ValueError as ex:
        res["mismatch"] = "ValueError"
    try:
        seq.file_quality("lzss.agmv", refs["rgb24"][1][:5].contiguous())
        res["file_mismatch"] = "accepted"
    except ValueError as ex:
        res["file_mismatch"] = "ValueError"
    # the measuring sink at a width that is no multiple of 16: 10 frames of 36 x 20 (two batches), an RGB24 reference
    n2, h2, w2 = 10, 20, 36
    small = np.ascontiguousarray(src[:n2, :h2, :w2])
    raw, stands_for = Q.reference_clip(2, small)
    tens = torch.from_numpy(raw).reshape(n2, h2, w2, 3).cuda()
    seq.encode_frames("small.agmv", torch.from_numpy(small.view(np.int32)).cuda(), opt=3, quality=3, compression=1, schedule=seq.SCHEDULE_FULL)
    decoded, _ = seq.decode_frames("small.agmv")
    e = (seq.AGMV_FRAME_QUALITY * n2)()
    rc = L.AGMV_MeasureFileDev(b"small.agmv", tens.data_ptr(), 2, n2, e, None)
    a = seq.clip_quality(decoded, tens, fmt="rgb24")
    want = Q.entries(Q.measure(decoded.cpu().numpy().view(np.uint32), stands_for))
    res["small"] = {"rc": rc, "decoded": list(decoded.shape), "file_is_clip": bool((words(e, n2) == of(a)).all()),
                    "clip_is_statement": bool((of(a) == want).all())}
    print(json.dumps(res))
""")


@functools.lru_cache(maxsize=None)
def answer():
    env = dict(dict.fromkeys(("AGMV_DITHER", "AGMV_PALETTE_REFINE", "AGMV_TRACE", "AGMV_LZ_DECODE_DEVICE")), AGMV_BATCH_FRAMES="8")
    with tempfile.TemporaryDirectory() as d:
        return K.run_child(d, CHILD, {"n": N, "w": W, "h": HT}, env, prelude="")


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("lz_stage", ["host", "device"])
@pytest.mark.parametrize("compression", ["lzss", "lz77"])
def test_file_measure_is_the_clip_measure_of_its_decode(compression, lz_stage, ref):
    c = answer()["cases"]["%s-%s-%s" % (compression, "1" if lz_stage == "device" else "0", ref)]
    assert c["rc"] == N == c["frames"] and c["decoded"] == [N, HT, W]
    assert c["clip_is_statement"], "AGMV_MeasureFramesDev differs from the numpy statement on the decoded clip"
    assert c["file_is_clip"], "AGMV_MeasureFileDev differs from AGMV_MeasureFramesDev on the decoded clip"
    assert c["seq_file_is_file"], "file_quality differs from AGMV_MeasureFileDev"
    assert c["lossy"] and c["dims"] == [W, HT, W, HT]
    assert c["psnr"][0] == c["psnr"][1] and 10.0 < c["psnr"][0] < 100.0 and c["block_psnr"] > c["psnr"][0] and 0.0 < c["ssim"] < 1.0


def test_file_measure_at_a_width_that_is_no_multiple_of_16():
    """36 x 20, ten frames in two batches: the reference's frames of the second batch lie 8 * 36 * 20 * 3 bytes into the clip"""
    c = answer()["small"]
    assert c["rc"] == 10 and c["decoded"] == [10, 20, 36]
    assert c["clip_is_statement"], "AGMV_MeasureFramesDev differs from the numpy statement on the decoded clip"
    assert c["file_is_clip"], "AGMV_MeasureFileDev differs from AGMV_MeasureFramesDev on the decoded clip"


def test_refusals_and_the_info_only_call():
    a = answer()
    assert a["count_low"] == a["count_high"] == -3
    assert a["odd_yuv"] == -3
    assert a["info_only"] == [0, N, W, HT]
    assert a["untouched"], "a refused call wrote entries"


def test_seq_checks_and_figures():
    a = answer()
    assert a["same"] == [0, float("inf"), 1.0, (W // 4 - 1) * (HT // 4 - 1) << 20, (W // 4 - 1) * (HT // 4 - 1)]
    assert a["mismatch"] == a["file_mismatch"] == "ValueError"
