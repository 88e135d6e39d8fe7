"""Whole files decoded at a target size: AGMV_DecodeFramesScaledDev of libagmv_amd/libagmv.so and
libagmv_amd.decode_frames(size=, scale=, fmt=) on torch tensors.

The comparator: the file is decoded natively (decode_frames without a size, which the existing file tests hold to the reference),
scaled in numpy (tests/upscale_cases.py, tests/scale_cases.py) and written in the layout by the numpy statement of its writing
rule; the scaled decode must deliver exactly those bytes, for the three filters and every layout.  The library rounds
AGMV_BATCH_FRAMES=3 up to whole GOPs of 4, so the 8-frame clip takes two batches and the decoder's state (the last frame, the
I-frame snapshot) has to survive in the double buffer at the file's size while the sink writes another size.  Child processes as
in tests/test_gpu_scale_files.py (the drivers keep process-wide state).  Needs an MI355X."""
import os
import textwrap

import children as K
import numpy as np
import pytest

import hostlib as H
import memseq_cases as MC
import pixfmt_cases as P
import scale_cases as SC
import upscale_cases as U
import yuv_cases as Y

pytestmark = pytest.mark.gpu

SPLASH = os.path.join(H.ROOT, "tests", "golden", "agmv_splash.agmv")
W, H0, T = 64, 48, 8
FMT_VALUE = {"xrgb32": P.XRGB32, "rgb24": P.RGB24, "bgr24": P.BGR24, "rgba32": P.RGBA32, "rgb8p": P.RGB8P, "nv12": Y.NV12, "i420": Y.I420}

# decode_frames on torch tensors.  job: clip (npy of the XRGB32 clip to encode, or none), path, dec: [{fmt, yuv, full, size, scale, out}],
# cap: {size, scale, fmt value, cap} for the C call.  Answers one JSON line.
CHILD = textwrap.dedent("""
    import ctypes as C, json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    from libagmv_amd import seq
    path = job["path"]
    if job.get("clip"):
        libagmv_amd.encode_frames(path, torch.from_numpy(np.load(job["clip"]).view(np.int32)).cuda(), schedule=libagmv_amd.SCHEDULE_FULL)
    before, info = libagmv_amd.decode_frames(path)
    np.save("native.npy", before.cpu().numpy().view(np.uint32)[:job.get("keep", 1 << 30)])
    shapes = []
    for d in job["dec"]:
        got, info2 = libagmv_amd.decode_frames(path, fmt=d["fmt"], yuv=d["yuv"], full_range=d["full"], size=tuple(d["size"]), scale=d["scale"])
        assert (info2.width, info2.height) == (info.width, info.height)
        shapes.append(list(got.shape))
        np.save(d["out"], got.cpu().numpy()[:job.get("keep", 1 << 30)])
    after, _ = libagmv_amd.decode_frames(path)
    res = {"shapes": shapes, "same": bool((before == after).all()), "frames": int(info.number_of_frames), "file": [int(info.width), int(info.height)]}
    c = job.get("cap")
    if c:
        L = seq.load_library()
        h, w = c["size"]
        fb = c["frame_bytes"]
        buf = torch.full((info.number_of_frames, fb), 0xA5, dtype=torch.uint8, device="cuda")
        res["cap_rc"] = L.AGMV_DecodeFramesScaledDev(path.encode(), buf.data_ptr(), c["fmt"], w, h, c["scale"], c["cap"], None)
        torch.cuda.synchronize()
        np.save("capped.npy", buf.cpu().numpy())
    print(json.dumps(res))
""")


def run_child(cwd, job, env=None):
    return K.run_child(cwd, CHILD, job, dict({"AGMV_BATCH_FRAMES": None, "AGMV_LZ_DECODE_DEVICE": None}, **(env or {})), prelude="")


def dec(fmt, size, scale, yuv=None, full=False):
    return {"fmt": fmt, "yuv": yuv, "full": full, "size": list(size), "scale": scale, "out": "%s_%s_%dx%d_%s%d.npy" % (fmt, scale, size[1], size[0], yuv, full)}


def fmt_value(d):
    return FMT_VALUE[d["fmt"]] | (Y.BT709 if d["yuv"] == "bt709" else 0) | (Y.FULL_RANGE if d["full"] else 0)


def tensor_shape(d, n):
    h, w = d["size"]
    return {"xrgb32": [n, h, w], "rgb24": [n, h, w, 3], "bgr24": [n, h, w, 3], "rgba32": [n, h, w, 4], "rgb8p": [n, 3, h, w],
            "nv12": [n, h * 3 // 2, w], "i420": [n, h * 3 // 2, w]}[d["fmt"]]


def check(tmp_path, jobs, res, n):
    native = np.load(tmp_path / "native.npy")
    assert native.shape[0] == n and (native >> 24 == 0).all()
    for d, shape in zip(jobs, res["shapes"]):
        h, w = d["size"]
        assert shape == tensor_shape(d, res["frames"]), d
        got = np.load(tmp_path / d["out"]).view(np.uint8).reshape(n, -1)
        exp = np.asarray(SC.from_packed(fmt_value(d), U.scale({"nearest": U.NEAREST, "area": U.AREA, "bilinear": U.BILINEAR}[d["scale"]], native, w, h)))
        exp = exp.view(np.uint8).reshape(n, -1)
        assert got.shape == exp.shape, d
        assert (got == exp).all(), (d, np.argwhere(got != exp)[:4])
    return native


# (h, w): 160 x 90 and 96 x 72 up, 32 x 20 down; every layout at least once; 37 x 23 and the I420 at 90 x 50 take the per-pixel path
JOBS = [dec("xrgb32", (90, 160), "bilinear"), dec("rgb24", (90, 160), "nearest"), dec("bgr24", (72, 96), "bilinear"), dec("rgba32", (72, 96), "nearest"),
        dec("rgb8p", (90, 160), "bilinear"), dec("nv12", (90, 160), "bilinear"), dec("i420", (72, 96), "nearest", "bt709", True),
        dec("nv12", (72, 96), "bilinear", "bt709"), dec("i420", (50, 90), "bilinear"), dec("rgb24", (23, 37), "bilinear"), dec("xrgb32", (72, 96), "nearest"),
        dec("xrgb32", (20, 32), "area"), dec("rgb24", (20, 32), "area"), dec("nv12", (20, 32), "area"), dec("rgb8p", (48, 64), "bilinear")]


def test_scaled_decode_equals_the_numpy_scaled_native_decode(tmp_path):
    """8 synthetic frames of 64 x 48 in two batches; a native decode before and after the scaled ones gives the same tensor (the
    context carries no scale state); the C call with cap_frames = 5 leaves the frames behind the cap alone"""
    np.save(tmp_path / "clip.npy", MC.synth_clip(W, H0, T))
    cap = {"size": [90, 160], "scale": U.BILINEAR, "fmt": Y.NV12, "cap": 5, "frame_bytes": SC.frame_bytes(Y.NV12, 160, 90)}
    res = run_child(tmp_path, {"clip": "clip.npy", "path": "clip.agmv", "dec": JOBS, "cap": cap}, {"AGMV_BATCH_FRAMES": "3"})
    assert res["frames"] == T and res["file"] == [W, H0] and res["same"]
    native = check(tmp_path, JOBS, res, T)
    assert len(np.unique(native.reshape(T, -1), axis=0)) == T                                      # every frame its own content
    ident = np.load(tmp_path / JOBS[-1]["out"])                                                    # a target of the file's own size is the native decode
    assert (ident.reshape(T, -1) == SC.from_packed(P.RGB8P, native)).all()
    capped = np.load(tmp_path / "capped.npy")
    assert res["cap_rc"] == 5
    assert (capped[:5] == SC.from_packed(Y.NV12, U.scale_bilinear(native[:5], 160, 90))).all()
    assert (capped[5:] == 0xA5).all()


def test_scaled_decode_with_the_lz_stage_on_the_device(tmp_path):
    np.save(tmp_path / "clip.npy", MC.synth_clip(W, H0, T))
    jobs = [JOBS[0], JOBS[5], JOBS[12]]
    res = run_child(tmp_path, {"clip": "clip.npy", "path": "clip.agmv", "dec": jobs}, {"AGMV_BATCH_FRAMES": "3", "AGMV_LZ_DECODE_DEVICE": "1"})
    assert res["same"]
    check(tmp_path, jobs, res, T)


def test_the_splash_file_at_twice_its_size(tmp_path):
    """agmv_splash.agmv (119 frames of 320 x 240) to 640 x 480: its first 4 frames against the numpy-scaled native decode"""
    jobs = [dec("xrgb32", (480, 640), "bilinear"), dec("nv12", (480, 640), "nearest")]
    res = run_child(tmp_path, {"path": SPLASH, "dec": jobs, "keep": 4})
    assert res["frames"] == 119 and res["file"] == [320, 240] and res["same"]
    check(tmp_path, jobs, res, 4)
