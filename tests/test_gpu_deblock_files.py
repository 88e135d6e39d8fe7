"""The deblocking through whole files: libagmv_amd.decode_frames(path, deblock=s) / file_quality(path, ref, deblock=s) on torch tensors
and AGMV_DEBLOCK in the environment of the BMP export.

The comparator is never the code under test: the file is decoded in full without the knob (decode_frames(path), which the file tests
hold to the reference), deblocked by the numpy statement (tests/deblock_cases.py), and then sliced (tests/view_cases.py), scaled
(tests/upscale_cases.py) and written in the layout or as a tensor by the numpy statements of tests/scale_cases.py and
tests/tensor_cases.py; the deblocked decode must deliver exactly those bytes, and the same call without the knob exactly the bytes of
the plain clip.  The clip is 24 frames of 64 x 48 (6 GOPs), encoded in the child; AGMV_BATCH_FRAMES=8 puts three batches and GOP
starts inside them.  Child processes as in tests/test_gpu_view_files.py.  Needs an MI355X."""
import textwrap

import children as CH
import numpy as np
import pytest

import deblock_cases as K
import dither_cases as D
import memseq_cases as MC
import pixfmt_cases as P
import quality_cases as Q
import scale_cases as SC
import tensor_cases as TC
import upscale_cases as U
import view_cases as V
import yuv_cases as Y

pytestmark = pytest.mark.gpu

W, H0, T, S = 64, 48, 24, 16
FMT_VALUE = {"xrgb32": P.XRGB32, "rgb24": P.RGB24, "nv12": Y.NV12, "rgb8p": P.RGB8P}
FILTER = {"area": U.AREA, "bilinear": U.BILINEAR}
ZERO = {"strength": 0, "frames": 0, "lines": 0, "weak": 0, "strong": 0}

# job: clip (npy of the XRGB32 clip to encode), path, s, decodes: [{fmt, size, scale, mean, std, frames ([start, stop, step] or none),
# crop}].  Every decode runs with deblock=s and with deblock=None.  Answers one JSON line.
CHILD = textwrap.dedent("""
    import json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    from libagmv_amd import seq
    path, s = job["path"], job["s"]
    src = torch.from_numpy(np.load(job["clip"]).view(np.int32)).cuda()
    libagmv_amd.encode_frames(path, src, schedule=libagmv_amd.SCHEDULE_FULL)
    res = {"fresh": libagmv_amd.deblock_stats(), "decodes": []}
    before, info = libagmv_amd.decode_frames(path)
    res["plain_stats"] = libagmv_amd.deblock_stats()
    np.save("native.npy", before.cpu().numpy().view(np.uint32))
    for k, d in enumerate(job["decodes"]):
        kw = dict(fmt=d["fmt"], mean=d.get("mean"), std=d.get("std"), crop=tuple(d["crop"]) if d.get("crop") else None)
        if d.get("size"):
            kw.update(size=tuple(d["size"]), scale=d["scale"])
        if d.get("frames") is not None:
            kw["frames"] = slice(*d["frames"])
        r = {}
        for name, knob in (("on", s), ("off", None)):
            got, _ = libagmv_amd.decode_frames(path, deblock=knob, **kw)
            r[name + "_shape"], r[name + "_stats"] = list(got.shape), libagmv_amd.deblock_stats()
            np.save("%s_%d.npy" % (name, k), got.contiguous().view(torch.uint8).cpu().numpy().reshape(-1))
        res["decodes"].append(r)
    if job.get("quality"):
        of = lambda q: np.concatenate([q.sse, q.block_sse, q.max_err, q.ssim_sum], axis=1).view(np.uint64)
        deblocked, _ = libagmv_amd.decode_frames(path, deblock=s)
        a, b = seq.clip_quality(deblocked, src), seq.file_quality(path, src, deblock=s)
        res["quality_stats"] = libagmv_amd.deblock_stats()
        plain = seq.file_quality(path, src)
        res["quality_plain_stats"] = libagmv_amd.deblock_stats()
        res["file_is_clip"] = bool(len(b) == len(a) and (of(a) == of(b)).all())
        res["plain_is_plain"] = bool((of(plain) == of(seq.clip_quality(before, src))).all())
        res["quality_differs"] = bool((of(plain) != of(b)).any())
        np.save("quality.npy", of(b))
    after, _ = libagmv_amd.decode_frames(path)
    res["same"] = bool(before.shape == after.shape and (before == after).all())
    res["after_stats"] = libagmv_amd.deblock_stats()
    print(json.dumps(res))
""")


def run_child(cwd, job, env=None):
    return CH.run_child(cwd, CHILD, job, dict({"AGMV_BATCH_FRAMES": "8", "AGMV_LZ_DECODE_DEVICE": None, "AGMV_DEBLOCK": None}, **(env or {})), prelude="")


def case(fmt, frames=None, crop=None, size=None, scale="bilinear", norm=None):
    d = {"fmt": fmt, "frames": frames, "crop": crop, "size": list(size) if size else None, "scale": scale}
    if norm:
        d["mean"], d["std"] = TC.NORMS[norm]
    return d


DECODES = [
    case("xrgb32"),                                                                # 0: the filter writes the caller's clip
    case("rgb24"),                                                                 # 1: a byte layout, through the extra batch
    case("nv12"),                                                                  # 2
    case("xrgb32", size=(72, 96), scale="bilinear"),                               # 3
    case("rgb8p", size=(24, 32), scale="area"),                                    # 4: through d_scaled
    case("f16", norm="imagenet"),                                                  # 5
    case("xrgb32", frames=[5, None, 3], crop=[3, 5, 14, 20]),                      # 6: an odd crop offset, stride 3, from inside GOP 1; packed windows
    case("rgb24", frames=[5, None, 3], crop=[3, 5, 14, 20]),                       # 7: ... through the batch of windows
    case("xrgb32", frames=[13, 21, 1]),                                            # 8: whole frames, copied from where they were filtered
]


def selection(d):
    """-> (the AGMV_VIEW fields of tests/view_cases.py, the frames of the file that pass the GPU stage)"""
    if d["frames"] is None and d["crop"] is None:
        return [0, 0, 1, 0, 0, 0, 0], (0, T)
    first, stop, step = d["frames"]
    sel = range(T)[slice(first, stop, step)]
    y, x, h, w = d["crop"] or (0, 0, 0, 0)
    return [first, len(sel), step, x, y, w, h], (first & ~3, sel[-1] + 1)


def expected(clip, d):
    """the bytes of the decode d of the XRGB32 clip `clip` (plain or deblocked), uint8 [frames, frame bytes]"""
    sel = V.view(clip, *selection(d)[0])
    if d["size"]:
        sel = U.scale(FILTER[d["scale"]], sel, d["size"][1], d["size"][0])
    if d["fmt"] == "f16":
        out = TC.from_packed(TC.table(TC.F16, d["mean"], d["std"]), sel)
    else:
        out = np.asarray(SC.from_packed(FMT_VALUE[d["fmt"]], sel))
    return np.ascontiguousarray(out).view(np.uint8).reshape(len(sel), -1)


def stats_of(native, span, s):
    lo, hi = span
    _, weak, strong = K.deblock(native[lo:hi], s)
    return {"strength": s, "frames": hi - lo, "lines": K.lines_examined(hi - lo, H0, W), "weak": weak, "strong": strong}


def check(tmp_path, decodes, res, s=S):
    native = np.load(tmp_path / "native.npy")
    assert native.shape == (T, H0, W)
    deblocked, weak, strong = K.deblock(native, s)
    assert weak + strong and (deblocked != native).any()
    assert res["fresh"] == ZERO and res["plain_stats"] == ZERO and res["after_stats"] == ZERO
    assert res["same"], "a plain decode before and after the deblocked ones differs"
    for k, (d, r) in enumerate(zip(decodes, res["decodes"])):
        for name, clip in (("on", deblocked), ("off", native)):
            exp = expected(clip, d)
            got = np.load(tmp_path / ("%s_%d.npy" % (name, k)))
            assert r[name + "_shape"][0] == len(exp) and got.size == exp.size, (k, d, name, r)
            assert (got.reshape(exp.shape) == exp).all(), (k, d, name, np.argwhere(got.reshape(exp.shape) != exp)[:4])
        assert r["off_stats"] == ZERO, (k, d, r)
        assert r["on_stats"] == stats_of(native, selection(d)[1], s), (k, d, r)
    return native


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    p = tmp_path_factory.mktemp("deblock_clip") / "clip.npy"
    np.save(p, MC.synth_clip(W, H0, T))
    return str(p)


def test_every_sink_receives_the_deblocked_clip_and_the_plain_one_without_the_knob(tmp_path, clip):
    res = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "s": S, "decodes": DECODES, "quality": True})
    native = check(tmp_path, DECODES, res)
    assert res["decodes"][6]["on_stats"]["frames"] == 20                          # the GPU stage of the view starts at frame 4
    # file_quality(deblock=s) is clip_quality of the deblocked decode, and that is the statement's measurement of the statement's clip
    assert res["file_is_clip"] and res["plain_is_plain"] and res["quality_differs"]
    want = Q.entries(Q.measure(K.deblock(native, S)[0], np.load(clip)))
    assert (np.load(tmp_path / "quality.npy") == want.reshape(T, -1)).all()
    assert res["quality_stats"] == stats_of(native, (0, T), S) and res["quality_plain_stats"] == ZERO


@pytest.mark.parametrize("batch,lz", [("4", None), ("5", "1"), ("64", "1")], ids=["batches of 4", "batches of 5, LZ on the device", "one batch, LZ on the device"])
def test_the_same_clip_under_other_batches_and_the_lz_stage_on_the_device(tmp_path, clip, batch, lz):
    decodes = [DECODES[0], DECODES[2], DECODES[4], DECODES[6], DECODES[7]]
    res = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "s": 32, "decodes": decodes}, {"AGMV_BATCH_FRAMES": batch, "AGMV_LZ_DECODE_DEVICE": lz})
    check(tmp_path, decodes, res, s=32)


def test_the_environment_sets_the_strength_and_the_bmp_export_writes_the_deblocked_frames(tmp_path, clip):
    """AGMV_DEBLOCK=16 in a child that only calls AGMV_DecodeAGMV; anything but a decimal number from 1 to 64 is off"""
    res = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "s": S, "decodes": []})
    native = np.load(tmp_path / "native.npy")
    deblocked = K.deblock(native, S)[0]
    from test_gpu_memseq import exported_pixels
    for value, want in (("16", deblocked), ("65", native), ("x", native), ("16abc", native)):
        d = tmp_path / ("bmp_" + value)
        d.mkdir()
        r = CH.decode_child(d, tmp_path / "clip.agmv", batch=8, env={"AGMV_DEBLOCK": value})
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        for k in range(T):
            assert (exported_pixels(str(d), k + 1, W, H0) == want[k] & np.uint32(0xFFFFFF)).all(), (value, k)
    assert res["same"]


BUYS = textwrap.dedent("""
    import json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    src = torch.from_numpy(np.load(job["clip"]).view(np.int32)).cuda()
    rows = []
    for opt in (2, 3):
        path = "fox_%d.agmv" % opt
        libagmv_amd.encode_frames(path, src, opt=opt, quality=1, schedule=libagmv_amd.SCHEDULE_FULL)
        for s in (None, 4, 16):
            q = libagmv_amd.file_quality(path, src, deblock=s)
            st = libagmv_amd.deblock_stats()
            rows.append([opt, s or 0, q.psnr(), q.block_psnr(), q.ssim(), st["weak"], st["strong"], st["lines"]])
    print(json.dumps(rows))
""")


def test_what_it_buys_on_the_golden_clip(tmp_path):
    """prints PSNR and SSIM of the golden clip's files (quality 1, every frame coded) against the source, without the knob and at
    strengths 4 and 16; asserts none of them (DESIGN.md section 4 records what came out) -- only that the measurement ran"""
    p = tmp_path / "fox.npy"
    np.save(p, D.fox()[0])
    rows = CH.run_child(tmp_path, BUYS, {"clip": str(p)}, {"AGMV_DEBLOCK": None}, prelude="")
    assert len(rows) == 6
    for opt, s, psnr, block_psnr, ssim, weak, strong, lines in rows:
        print("deblock: golden clip AGMV_OPT_%s strength %2d: PSNR %.3f dB, block PSNR %.3f dB, SSIM %.5f; %d weak + %d strong of %d lines"
              % ("I" * opt, s, psnr, block_psnr, ssim, weak, strong, lines))
        assert (lines == 0) == (s == 0) and np.isfinite(psnr)
