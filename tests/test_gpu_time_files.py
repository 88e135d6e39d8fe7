"""Whole files at another frame rate: libagmv_amd.encode_frames(rate=, time=, select=, crop=, fit=, size=) on torch tensors, which is
AGMV_EncodeViewRateDev of libagmv_amd/libagmv.so.

The comparator is never the code under test: the clip is read to XRGB32, its frames and window are taken and the result R is formed
in numpy (tests/time_cases.py); the file must be, byte for byte, the file encode_frames writes in the same child for that contiguous
XRGB32 clip R -- with the same size= and scale= where the case has a target, which the scale tests hold to numpy.  The clip is 13
frames of 40 x 24 whose pixels move from frame to frame; AGMV_GetEncodeRateStats against the statement's counts.  Child processes as
in tests/test_gpu_view_source_files.py (the drivers keep process-wide state).  Needs an MI355X."""
import os
import textwrap

import children as K
import numpy as np
import pytest

import pixfmt_cases as P
import time_cases as TC
import view_cases as V
import yuv_cases as Y

pytestmark = pytest.mark.gpu

W, H0, T = 40, 24, 13
FULL, PDIFS, ADAPTIVE = 1, 2, 3
# name -> (fmt value, encode_frames' fmt, yuv, full_range)
LAYOUTS = {"rgb24": (P.RGB24, "rgb24", None, False), "nv12": (Y.NV12, "nv12", None, False)}

# job: enc = [{out, clip (npy), fmt, yuv, full_range, kw (encode_frames' keywords; select as [start, stop, step]), stage (AGMV_VIEW_STAGE_FRAMES
# or none)}].  Answers one JSON line: per encode the ValueError's text ("" for none), the rate stats and the view stats.
CHILD = textwrap.dedent("""
    import json, os, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    errors, stats, views = [], [], []
    for e in job["enc"]:
        a = np.load(e["clip"])
        clip = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        kw = dict(e["kw"])
        for name in ("crop", "size", "rate", "select"):
            if kw.get(name) is not None:
                kw[name] = tuple(kw[name])
        os.environ.pop("AGMV_VIEW_STAGE_FRAMES", None)
        if e.get("stage"):
            os.environ["AGMV_VIEW_STAGE_FRAMES"] = e["stage"]
        try:
            libagmv_amd.encode_frames(e["out"], clip, fmt=e["fmt"], yuv=e.get("yuv"), full_range=e.get("full_range", False), **kw)
            errors.append("")
        except ValueError as err:
            errors.append(str(err))
        stats.append(list(libagmv_amd.encode_rate_stats()))
        views.append(list(libagmv_amd.encode_view_stats()))
    print(json.dumps({"errors": errors, "stats": stats, "views": views}))
""")


def run_child(cwd, enc):
    return K.run_child(cwd, CHILD, {"enc": enc}, {"AGMV_BATCH_FRAMES": "8", "AGMV_VIEW_STAGE_FRAMES": None}, prelude="")


_clips = {}


def clips(name):
    """(the moving clip written in the layout, shaped as encode_frames takes it; the XRGB32 clip that stands for: uint32 [T, 24, 40]), once"""
    if name not in _clips:
        fmt = LAYOUTS[name][0]
        raw, packed = TC.moving_clip(fmt, T, H0, W, 77)
        tensor = raw.reshape((T, H0, W, 3) if fmt == P.RGB24 else (T, H0 * 3 // 2, W))
        tensor.setflags(write=False)
        packed.setflags(write=False)
        _clips[name] = tensor, packed
    return _clips[name]


class Jobs:
    """pairs of an encode of the clip in its layout at a rate and the encode of the numpy-made R, for one child"""

    def __init__(self, tmp_path, name):
        self.tmp, self.name, self.enc, self.pairs = tmp_path, name, [], []
        self.tensor, self.packed = clips(name)
        np.save(tmp_path / "clip.npy", self.tensor)

    def source(self, out, stage=None, **kw):
        _, fmt, yuv, full_range = LAYOUTS[self.name]
        self.enc.append({"out": out, "clip": "clip.npy", "fmt": fmt, "yuv": yuv, "full_range": full_range, "kw": kw, "stage": stage})
        return len(self.enc) - 1

    def rated(self, tag, rate, time="area", select=None, crop=None, stage=None, **kw):
        """the encode at a rate, and the comparator: R from numpy as an xrgb32 clip, with what is left of the keywords"""
        first, stop, step = select if select is not None else (0, T, 1)
        top, left, ch, cw = crop if crop is not None else (0, 0, 0, 0)
        v = V.view(self.packed, first, len(range(first, min(stop, T), step)), step, left, top, cw, ch)
        filt = {"area": TC.AREA, "nearest": TC.NEAREST}[time]
        r = TC.resample(v, rate[0], rate[1], filt)
        np.save(self.tmp / (tag + ".npy"), r)
        extra = {} if time == "area" and len(self.enc) % 2 else {"time": time}      # the default is "area"
        k = self.source(tag + ".rate.agmv", stage, rate=list(rate), select=select, crop=crop, **extra, **kw)
        self.enc.append({"out": tag + ".cmp.agmv", "clip": tag + ".npy", "fmt": "xrgb32", "kw": kw})
        self.pairs.append((tag, k, [v.shape[0], r.shape[0], TC.frame_reads(v.shape[0], rate[0], rate[1], filt)]))
        return k

    def run(self):
        self.res = run_child(self.tmp, self.enc)
        assert self.res["errors"] == [""] * len(self.enc), self.res["errors"]
        for tag, k, counts in self.pairs:
            a, b = self.read(tag + ".rate.agmv"), self.read(tag + ".cmp.agmv")
            assert len(b) > 500 and int.from_bytes(b[4:8], "little") >= 1, tag
            assert a == b, "%s %s: the file differs from the file of the numpy-made clip (%d / %d bytes)" % (self.name, tag, len(a), len(b))
            assert self.res["stats"][k] == counts, (tag, self.res["stats"][k], counts)
            assert self.res["views"][k][0] == counts[1], (tag, self.res["views"][k])
        return self.res

    def read(self, name):
        return open(self.tmp / name, "rb").read()


WINDOW, ODD = (4, 8, 16, 24), (3, 5, 16, 24)         # (top, left, height, width)
SCALED = (2, 6, 20, 32)


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_rated_files_equal_the_files_of_the_numpy_made_clip(name, tmp_path):
    j = Jobs(tmp_path, name)
    k_whole = j.rated("whole", (5, 2))                                          # no view at all: the whole clip, 5 frames
    j.rated("window", (3, 2), crop=WINDOW)
    j.rated("odd", (13, 12), crop=ODD)                                          # NV12: across the 2 x 2 cells
    j.rated("stride", (3, 2), select=(1, T, 2))                                 # 6 frames of V, 4 of R
    j.rated("nearest", (3, 1), time="nearest", crop=WINDOW)
    j.rated("doubled", (2, 5), time="nearest", select=(2, 9, 3), crop=ODD)      # 3 frames of V, 7 of R
    j.rated("reduced", (10, 4), select=(0, T, 1), crop=WINDOW)
    staged = {}
    for stage in ("1", "3", None):
        staged["area", stage] = j.rated("area%s" % (stage or ""), (5, 2), crop=SCALED, stage=stage, size=(8, 16), scale="area")
        staged["nearest", stage] = j.rated("nearest-size%s" % (stage or ""), (3, 2), crop=SCALED, stage=stage, size=(24, 32), scale="nearest")
    k_fit = j.source("fit.agmv", fit="crop", size=(16, 16), rate=[3, 2])
    j.rated("fit", (3, 2), crop=(0, 8, 24, 24), size=(16, 16))
    res = j.run()
    st, vs = res["stats"], res["views"]
    assert st[k_whole] == [T, 5, 5 * 5 // 2 + 5 - 5 // 2] and vs[k_whole] == [5, 4 * W * H0 * 5, 0]
    window_bytes = 4 * 32 * 20
    assert vs[staged["area", "1"]] == [5, 4 * 16 * 8 * 5, window_bytes] and vs[staged["area", "3"]] == [5, 4 * 16 * 8 * 5, 3 * window_bytes]
    assert vs[staged["area", None]] == [5, 4 * 16 * 8 * 5, 5 * window_bytes] and vs[staged["nearest", "3"]] == [8, 4 * 32 * 24 * 8, 3 * window_bytes]
    for f in ("area", "nearest-size"):
        assert j.read(f + "1.rate.agmv") == j.read(f + "3.rate.agmv") == j.read(f + ".rate.agmv")      # the batches change nothing
    assert j.read("fit.agmv") == j.read("fit.rate.agmv") and st[k_fit] == [T, 8, 8 * 3 // 2 + 8 - 8 // 2]
    assert j.read("reduced.rate.agmv") != j.read("window.rate.agmv")
    assert len({j.read(t + ".rate.agmv") for t, _, _ in j.pairs}) >= len(j.pairs) - 5          # (different rates and views, different files)


def test_schedules_and_knobs(tmp_path):
    j = Jobs(tmp_path, "rgb24")
    for schedule in (FULL, PDIFS, ADAPTIVE):
        j.rated("schedule%d" % schedule, (3, 2), crop=WINDOW, schedule=schedule)
        j.rated("schedule%d-scaled" % schedule, (13, 12) if schedule == ADAPTIVE else (5, 2), time="nearest" if schedule == PDIFS else "area", crop=SCALED,
                size=(8, 16), schedule=schedule)
    j.rated("one-frame", (13, 1), crop=WINDOW, schedule=FULL)                   # all frames into one
    j.rated("heavy", (4, 1), crop=WINDOW, opt=1)                                # three frames are enough for a heavy opt
    j.rated("lz77", (3, 2), crop=WINDOW, compression=2, opt=2)
    j.rated("knobs", (13, 12), crop=WINDOW, dither=8, stabilise=6, palette_refine=3)
    j.rated("knobs-scaled", (3, 2), crop=SCALED, size=(8, 16), dither=8, stabilise=6, palette_refine=3, stage="3")
    j.rated("fps", (5, 2), fps=10, schedule=FULL)
    j.run()
    assert j.read("knobs.rate.agmv") != j.read("schedule2.rate.agmv")
    assert int.from_bytes(j.read("fps.rate.agmv")[18:22], "little") == int.from_bytes(j.read("fps.cmp.agmv")[18:22], "little")


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_no_rate_and_one_to_one_are_the_view_call(name, tmp_path):
    """rate=None and rate=(3, 3) give the file of today's encode_frames(select=...), and the view's stats"""
    j = Jobs(tmp_path, name)
    cases = {"stride": dict(select=[1, T, 2]), "window": dict(select=[0, T, 1], crop=list(ODD)), "scaled": dict(select=[0, T, 3], crop=list(SCALED), size=[8, 16]),
             "whole": dict(select=[0, T, 1])}
    ks = {}
    for tag, kw in cases.items():
        ks[tag] = [j.source("%s.%s.agmv" % (tag, how), **dict(kw, **extra))
                   for how, extra in (("view", {}), ("none", {"rate": None}), ("same", {"rate": [3, 3]}), ("same-nearest", {"rate": [7, 7], "time": "nearest"}))]
    res = run_child(tmp_path, j.enc)
    assert res["errors"] == [""] * len(j.enc), res["errors"]
    for tag, (k_view, k_none, k_same, k_near) in ks.items():
        want = j.read("%s.view.agmv" % tag)
        assert len(want) > 500
        for how, k in (("none", k_none), ("same", k_same), ("same-nearest", k_near)):
            assert j.read("%s.%s.agmv" % (tag, how)) == want, (tag, how)
            assert res["views"][k] == res["views"][k_view], (tag, how)
        n = res["views"][k_view][0]
        assert res["stats"][k_same] == [n, n, n] and res["stats"][k_near] == [n, n, n]
    assert res["views"][ks["whole"][2]] == [T, 0, 0] and res["views"][ks["stride"][2]][0] == 6


def test_a_result_too_short_creates_no_file(tmp_path):
    """13 frames at 4 : 1 are 3, one short of what the PDIFS schedule reads first: -2 from the library, which opened no file; so is a
    window whose size the encoder refuses (-3).  The stats of a refused call are zero; the next call is not disturbed."""
    tensor, _ = clips("nv12")
    np.save(tmp_path / "clip.npy", tensor)
    base = {"clip": "clip.npy", "fmt": "nv12"}
    enc = [dict(base, out="short.agmv", kw={"rate": [4, 1]}),
           dict(base, out="short-view.agmv", kw={"rate": [3, 2], "select": [0, 5, 1]}),
           dict(base, out="none.agmv", kw={"rate": [14, 1], "schedule": FULL}),
           dict(base, out="odd-size.agmv", kw={"rate": [3, 2], "crop": [0, 0, 10, 16]}),
           dict(base, out="area-up.agmv", kw={"rate": [3, 2], "crop": list(WINDOW), "size": [20, 24]}),
           dict(base, out="good.agmv", kw={"rate": [3, 1]})]
    res = run_child(tmp_path, enc)
    assert all("AGMV_EncodeViewRateDev refused its arguments (%d)" % rc in e for rc, e in zip((-2, -2, -2, -3, -3), res["errors"])), res["errors"]
    assert res["errors"][5] == "" and res["stats"][:5] == [[0, 0, 0]] * 5 and res["views"][:5] == [[0, 0, 0]] * 5
    assert res["stats"][5] == [T, 4, TC.frame_reads(T, 3, 1, TC.AREA)] and res["views"][5] == [4, 4 * W * H0 * 4, 0]
    assert [os.path.exists(tmp_path / e["out"]) for e in enc] == [False] * 5 + [True]
