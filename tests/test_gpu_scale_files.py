"""Whole files from clips scaled to a target size: AGMV_EncodeFramesScaledDev of libagmv_amd/libagmv.so and
libagmv_amd.encode_frames(size=, scale=) on torch tensors.

The comparator: the clip is read to XRGB32 and scaled in numpy (tests/scale_cases.py); AGMV_EncodeFramesScaledDev(clip) must write
the bytes that AGMV_EncodeFramesDev(numpy-scaled clip) writes in the same child, for every layout and both filters, from a source
size the unscaled calls refuse (50 x 38).  The reference's golden: the mixed clip with every pixel doubled scales back to the mixed
clip under both rules, so the scaled encode must give the files the compiled reference wrote for the mixed clip.  Child processes
as in tests/test_gpu_yuv_files.py (the drivers keep process-wide state).  Needs an MI355X."""
import functools
import hashlib
import json
import os
import textwrap

import children as K
import numpy as np
import pytest

import memseq_cases as MC
import pixfmt_cases as P
import scale_cases as SC
import yuv_cases as Y

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(TESTS, "golden")
FULL, PDIFS, ADAPTIVE = 1, 2, 3
I420_709F = Y.I420 | Y.BT709 | Y.FULL_RANGE
FORMATS = SC.BYTE_LAYOUTS + (Y.NV12, I420_709F)

CHILD = textwrap.dedent("""
    L.AGMV_SetBatchFrames(job["batch"])
    rcs = []

    for e in job["enc"]:
        tail = [24, e["opt"], e["quality"], e["compression"], e["schedule"]]
        if "raw" in e:                       # the clip in its layout through the scaled call (filter 0: through AGMV_EncodeFramesFmtDev, unscaled)
            raw = np.load(e["raw"])
            d = upload(raw)
            if e["filter"]:
                rcs.append(L.AGMV_EncodeFramesScaledDev(e["out"].encode(), d, e["fmt"], raw.shape[0], e["sw"], e["sh"], e["w"], e["h"], e["filter"], *tail))
            else:
                rcs.append(L.AGMV_EncodeFramesFmtDev(e["out"].encode(), d, e["fmt"], raw.shape[0], e["sw"], e["sh"], *tail))
        else:                                # an XRGB32 clip through AGMV_EncodeFramesDev
            packed = np.load(e["packed"])
            n, h, w = packed.shape
            d = upload(packed)
            rcs.append(L.AGMV_EncodeFramesDev(e["out"].encode(), d, n, w, h, *tail))
        free(d)
    print(json.dumps({"rc": rcs}))
""")

# libagmv_amd.encode_frames on torch tensors, in a child as well
SEQ_CHILD = textwrap.dedent("""
    import json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    rgb = torch.from_numpy(np.load("rgb24.npy")).cuda()                     # uint8 [n, 38, 50, 3]
    nv12 = torch.from_numpy(np.load("nv12.npy")).cuda()                     # uint8 [n, 72, 64]
    small = torch.from_numpy(np.load("small.npy")).cuda()                   # uint8 [n, 16, 24, 3]
    for scale in ("area", "nearest"):
        libagmv_amd.encode_frames("rgb24_%s.agmv" % scale, rgb, size=(16, 24), scale=scale)
        libagmv_amd.encode_frames("nv12_%s.agmv" % scale, nv12, fmt="nv12", yuv="bt709", size=(24, 32), scale=scale)
        libagmv_amd.encode_frames("same_%s.agmv" % scale, small, size=(16, 24), scale=scale)
    libagmv_amd.encode_frames("area_by_default.agmv", rgb, size=(16, 24))
    libagmv_amd.encode_frames("none.agmv", small, size=None)
    libagmv_amd.encode_frames("today.agmv", small)
    refused = []
    # no multiple of 4; an area upscale; the same upscale with nearest, which is fine and writes its file; 50 x 38 unscaled
    for k, kw in enumerate((dict(size=(18, 24)), dict(size=(40, 24)), dict(size=(40, 24), scale="nearest"), dict())):
        try:
            libagmv_amd.encode_frames("attempt%d.agmv" % k, rgb, **kw)
            refused.append("")
        except ValueError as e:
            refused.append(str(e))
    print(json.dumps({"refused": refused}))
""")


def run_child(cwd, job, script=CHILD):
    return K.run_child(cwd, script, job, prelude="" if script is SEQ_CHILD else K.PRELUDE)


@functools.lru_cache(maxsize=None)
def clips(fmt, w, h, n=12):
    """(synth_clip written in fmt: uint8 [n, frame bytes]; the XRGB32 clip that stands for: uint32 [n, h, w]), computed once"""
    raw = SC.from_packed(fmt, MC.synth_clip(w, h, n))
    packed = SC.to_packed(fmt, raw, w, h)
    raw.setflags(write=False)
    packed.setflags(write=False)
    return raw, packed


def scaled_against_comparator(tmp_path, fmt, sw, sh, w, h, filters, schedule, opt=3, quality=3, compression=1):
    """per filter: AGMV_EncodeFramesScaledDev(clip in fmt) and AGMV_EncodeFramesDev(numpy-scaled clip) in one child -> equal bytes"""
    raw, packed = clips(fmt, sw, sh)
    np.save(tmp_path / "raw.npy", raw)
    enc = []
    common = {"opt": opt, "quality": quality, "compression": compression, "schedule": schedule}
    for f in filters:
        np.save(tmp_path / ("packed%d.npy" % f), SC.scale(f, packed, w, h))
        enc.append(dict(common, raw="raw.npy", fmt=fmt, sw=sw, sh=sh, w=w, h=h, filter=f, out="scaled%d.agmv" % f))
        enc.append(dict(common, packed="packed%d.npy" % f, out="comparator%d.agmv" % f))
    assert run_child(tmp_path, {"batch": 8, "enc": enc})["rc"] == [0] * len(enc)
    files = {}
    for f in filters:
        a, b = open(tmp_path / ("scaled%d.agmv" % f), "rb").read(), open(tmp_path / ("comparator%d.agmv" % f), "rb").read()
        assert len(b) > 1000 and int.from_bytes(b[4:8], "little") >= 1
        assert int.from_bytes(b[8:12], "little") == w and int.from_bytes(b[12:16], "little") == h
        assert a == b, "%s: the file from the scaled clip differs from the file of the numpy-scaled clip (%d / %d bytes)" % (SC.FILTER_NAMES[f], len(a), len(b))
        files[f] = a
    return files


@pytest.mark.parametrize("schedule", [FULL, PDIFS], ids=["full", "pdifs"])
@pytest.mark.parametrize("fmt", FORMATS, ids=[SC.fmt_name(f) for f in FORMATS])
def test_scaled_encode_equals_encode_of_the_numpy_scaled_clip(fmt, schedule, tmp_path):
    """50 x 38 (no multiple of 4: the unscaled calls refuse it) -> 24 x 16, both filters, 12 frames, LZSS"""
    files = scaled_against_comparator(tmp_path, fmt, 50, 38, 24, 16, (SC.AREA, SC.NEAREST), schedule)
    assert files[SC.AREA] != files[SC.NEAREST]


def test_scaled_encode_with_lz77(tmp_path):
    scaled_against_comparator(tmp_path, P.RGB24, 50, 38, 24, 16, (SC.AREA,), PDIFS, compression=2)


def test_scaled_encode_with_256_colours(tmp_path):
    scaled_against_comparator(tmp_path, Y.NV12, 50, 38, 24, 16, (SC.AREA, SC.NEAREST), PDIFS, opt=2)


@pytest.mark.parametrize("fmt", [P.RGB24, P.RGB8P], ids=["rgb24", "rgb8p"])
def test_doubled_mixed_clip_gives_the_references_files(fmt, tmp_path):
    """the mixed clip, every pixel doubled (320 x 256), scaled to 160 x 128 with either filter and encoded with
    AGMV_SCHEDULE_ADAPTIVE is the mixed clip encoded: the files of the compiled reference (tests/golden/golden_memseq.json),
    whose chain takes both branches.  From RGB layouts only: a YUV writing would not give the doubled clip back."""
    gold = json.load(open(os.path.join(GOLDEN, "golden_memseq.json")))
    clip = MC.mixed_clip()
    big = SC.doubled(clip)
    # a condition on the input, not on the code under test
    assert (SC.scale_area(big, MC.MIXED_W, MC.MIXED_H) == clip).all() and (SC.scale_nearest(big, MC.MIXED_W, MC.MIXED_H) == clip).all()
    np.save(tmp_path / "raw.npy", SC.from_packed(fmt, big))
    enc = []
    for name, (opt, quality, compression) in sorted(MC.MIXED_CASES.items()):
        assert 0 in gold[name]["chain"] and 1 in gold[name]["chain"]
        for f in (SC.AREA, SC.NEAREST):
            enc.append({"raw": "raw.npy", "fmt": fmt, "sw": 320, "sh": 256, "w": MC.MIXED_W, "h": MC.MIXED_H, "filter": f, "opt": opt, "quality": quality,
                        "compression": compression, "schedule": ADAPTIVE, "out": "%s.%s.agmv" % (name, SC.FILTER_NAMES[f])})
    assert run_child(tmp_path, {"batch": 8, "enc": enc})["rc"] == [0] * len(enc)
    for e in enc:
        g = gold[e["out"].split(".")[0]]
        data = open(tmp_path / e["out"], "rb").read()
        assert int.from_bytes(data[4:8], "little") == g["frames"] and int.from_bytes(data[18:22], "little") == g["fps_field"], e["out"]
        assert len(data) == g["file_len"], e["out"]
        assert hashlib.sha256(data).hexdigest() == g["file_sha"], "%s differs from the reference's file" % e["out"]


def test_seq_scales_tensors(tmp_path):
    """encode_frames(size=, scale=) on an rgb24 and an nv12 tensor equals the comparator's file; size=None is today's call and
    today's file; a target of the source's own size, with either filter, is today's AGMV_EncodeFramesFmtDev file"""
    rgb_raw, rgb_packed = clips(P.RGB24, 50, 38)
    nv_fmt = Y.NV12 | Y.BT709
    nv_raw, nv_packed = clips(nv_fmt, 64, 48)
    small_raw, small_packed = clips(P.RGB24, 24, 16)
    n = rgb_raw.shape[0]
    np.save(tmp_path / "rgb24.npy", rgb_raw.reshape(n, 38, 50, 3))
    np.save(tmp_path / "nv12.npy", nv_raw.reshape(n, 72, 64))
    np.save(tmp_path / "small.npy", small_raw.reshape(n, 16, 24, 3))
    refused = run_child(tmp_path, {}, SEQ_CHILD)["refused"]
    assert "50x38" in refused[0] and "24x18" in refused[0] and "50x38" in refused[1] and "24x40" in refused[1], refused       # both sizes are named
    assert refused[2] == "" and "50x38" in refused[3], refused
    assert [os.path.exists(tmp_path / ("attempt%d.agmv" % k)) for k in range(4)] == [False, False, True, False]      # a refusal creates no file
    # the comparator files, from the C entry points in another child
    enc, common = [], {"opt": 3, "quality": 3, "compression": 1, "schedule": PDIFS}
    for f in (SC.AREA, SC.NEAREST):
        np.save(tmp_path / ("rgb_packed%d.npy" % f), SC.scale(f, rgb_packed, 24, 16))
        np.save(tmp_path / ("nv_packed%d.npy" % f), SC.scale(f, nv_packed, 32, 24))
        enc.append(dict(common, packed="rgb_packed%d.npy" % f, out="cmp_rgb24_%s.agmv" % SC.FILTER_NAMES[f]))
        enc.append(dict(common, packed="nv_packed%d.npy" % f, out="cmp_nv12_%s.agmv" % SC.FILTER_NAMES[f]))
    np.save(tmp_path / "small_raw.npy", small_raw)
    enc.append(dict(common, raw="small_raw.npy", fmt=P.RGB24, sw=24, sh=16, filter=0, out="cmp_fmtdev.agmv"))
    assert run_child(tmp_path, {"batch": 0, "enc": enc})["rc"] == [0] * len(enc)
    read = lambda name: open(tmp_path / name, "rb").read()
    for name in ("area", "nearest"):
        assert read("rgb24_%s.agmv" % name) == read("cmp_rgb24_%s.agmv" % name), name
        assert read("nv12_%s.agmv" % name) == read("cmp_nv12_%s.agmv" % name), name
        assert read("same_%s.agmv" % name) == read("cmp_fmtdev.agmv"), name
    assert read("area_by_default.agmv") == read("rgb24_area.agmv") != read("rgb24_nearest.agmv")
    assert read("none.agmv") == read("today.agmv") == read("cmp_fmtdev.agmv")
    assert len(read("cmp_fmtdev.agmv")) > 1000
