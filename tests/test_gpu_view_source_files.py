"""Whole files from views of a clip: libagmv_amd.encode_frames(select=, crop=, fit=, size=) on torch tensors, which is
AGMV_EncodeViewDev of libagmv_amd/libagmv.so.

The comparator is never the code under test: the clip is read to XRGB32 and its frames and window are taken in numpy
(tests/view_source_cases.py); the view's file must be, byte for byte, the file encode_frames writes in the same child for that
contiguous XRGB32 clip V -- with the same size= and scale= where the view has a target, which the scale tests hold to numpy.  The
clip is 13 frames of 40 x 24 in each of the seven layouts; AGMV_GetEncodeViewStats shows which path ran.  Child processes as in
tests/test_gpu_scale_files.py (the drivers keep process-wide state).  Needs an MI355X."""
import os
import textwrap

import children as K
import numpy as np
import pytest

import memseq_cases as MC
import pixfmt_cases as P
import scale_cases as SC
import view_cases as V
import view_source_cases as VS
import yuv_cases as Y

pytestmark = pytest.mark.gpu

W, H0, T = 40, 24, 13
FULL, PDIFS, ADAPTIVE = 1, 2, 3
# name -> (fmt value, encode_frames' fmt, yuv, full_range)
LAYOUTS = {"xrgb32": (P.XRGB32, "xrgb32", None, False), "rgb24": (P.RGB24, "rgb24", None, False), "bgr24": (P.BGR24, "bgr24", None, False),
           "rgba32": (P.RGBA32, "rgba32", None, False), "rgb8p": (P.RGB8P, "rgb8p", None, False), "nv12": (Y.NV12, "nv12", None, False),
           "i420-bt709full": (Y.I420 | Y.BT709 | Y.FULL_RANGE, "i420", "bt709", True)}

# job: enc = [{out, clip (npy), fmt, yuv, full_range, kw (encode_frames' keywords; select as [start, stop, step], stop None for a slice),
# stage (AGMV_VIEW_STAGE_FRAMES or none)}].  Answers one JSON line: per encode the ValueError's text ("" for none) and the stats.
CHILD = textwrap.dedent("""
    import json, os, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    errors, stats = [], []
    for k, e in enumerate(job["enc"]):
        a = np.load(e["clip"])
        clip = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        kw = dict(e["kw"])
        for name in ("crop", "size"):
            if kw.get(name) is not None:
                kw[name] = tuple(kw[name])
        s = kw.get("select")
        if s is not None:
            kw["select"] = slice(*s) if s[1] is None else (tuple(s), range(*s), slice(*s))[k % 3]
        os.environ.pop("AGMV_VIEW_STAGE_FRAMES", None)
        if e.get("stage"):
            os.environ["AGMV_VIEW_STAGE_FRAMES"] = e["stage"]
        try:
            libagmv_amd.encode_frames(e["out"], clip, fmt=e["fmt"], yuv=e.get("yuv"), full_range=e.get("full_range", False), **kw)
            errors.append("")
        except ValueError as err:
            errors.append(str(err))
        stats.append(list(libagmv_amd.encode_view_stats()))
    print(json.dumps({"errors": errors, "stats": stats}))
""")


def run_child(cwd, enc):
    return K.run_child(cwd, CHILD, {"enc": enc}, {"AGMV_BATCH_FRAMES": "8", "AGMV_VIEW_STAGE_FRAMES": None}, prelude="")


_clips = {}


def clips(name):
    """(the synthetic clip written in the layout, shaped as encode_frames takes it; the XRGB32 clip that stands for: uint32 [T, 24, 40]), once"""
    if name not in _clips:
        fmt = LAYOUTS[name][0]
        raw = SC.from_packed(fmt, MC.synth_clip(W, H0, T))
        packed = VS.packed(fmt, raw, W, H0)
        shape = {P.XRGB32: (T, H0, W), P.RGB24: (T, H0, W, 3), P.BGR24: (T, H0, W, 3), P.RGBA32: (T, H0, W, 4), P.RGB8P: (T, 3, H0, W)}.get(fmt, (T, H0 * 3 // 2, W))
        tensor = raw.view(np.uint32).reshape(shape) if fmt == P.XRGB32 else raw.reshape(shape)
        tensor.setflags(write=False)
        packed.setflags(write=False)
        _clips[name] = tensor, packed
    return _clips[name]


class Jobs:
    """pairs of a view encode of the clip in its layout and the encode of the numpy-made V, for one child"""

    def __init__(self, tmp_path, name):
        self.tmp, self.name, self.enc, self.pairs = tmp_path, name, [], []
        self.tensor, self.packed = clips(name)
        np.save(tmp_path / "clip.npy", self.tensor)

    def source(self, out, stage=None, **kw):
        _, fmt, yuv, full_range = LAYOUTS[self.name]
        self.enc.append({"out": out, "clip": "clip.npy", "fmt": fmt, "yuv": yuv, "full_range": full_range, "kw": kw, "stage": stage})
        return len(self.enc) - 1

    def view(self, tag, select=None, crop=None, stage=None, **kw):
        """the view, and the comparator: V from numpy as an xrgb32 clip, with what is left of the keywords"""
        first, stop, step = select if select is not None else (0, T, 1)
        top, left, ch, cw = crop if crop is not None else (0, 0, 0, 0)
        v = V.view(self.packed, first, len(range(first, min(T if stop is None else stop, T), step)), step, left, top, cw, ch)
        np.save(self.tmp / (tag + ".npy"), v)
        k = self.source(tag + ".view.agmv", stage, select=select, crop=crop, **kw)
        self.enc.append({"out": tag + ".cmp.agmv", "clip": tag + ".npy", "fmt": "xrgb32", "kw": kw})
        self.pairs.append((tag, k, v))
        return k

    def run(self):
        self.res = run_child(self.tmp, self.enc)
        assert self.res["errors"] == [""] * len(self.enc), self.res["errors"]
        for tag, k, v in self.pairs:
            a, b = self.read(tag + ".view.agmv"), self.read(tag + ".cmp.agmv")
            assert len(b) > 500 and int.from_bytes(b[4:8], "little") >= 1, tag
            assert a == b, "%s %s: the view's file differs from the file of the numpy-made clip (%d / %d bytes)" % (self.name, tag, len(a), len(b))
            assert self.res["stats"][k][0] == v.shape[0], (tag, self.res["stats"][k])
        return self.res

    def read(self, name):
        return open(self.tmp / name, "rb").read()


WINDOW, ODD = (4, 8, 16, 24), (3, 5, 16, 24)         # (top, left, height, width)
SCALED = (2, 6, 20, 32)


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_view_files_equal_the_files_of_the_numpy_made_clip(name, tmp_path):
    j = Jobs(tmp_path, name)
    k_window = j.view("window", crop=WINDOW)
    j.view("odd", crop=ODD)                                                     # NV12 / I420: across the 2 x 2 cells
    k_stride = j.view("stride", select=(1, T, 2))
    k_range = j.view("range", select=(3, 11, 1))
    j.source("sliced.agmv")                                                     # (replaced below: the sliced clip in its own layout)
    j.enc[-1]["clip"] = "sliced.npy"
    np.save(tmp_path / "sliced.npy", np.ascontiguousarray(j.tensor[3:11]))
    k_cut = j.view("cut", select=(5, None, 1))                                  # a slice to the end: consecutive full frames again
    staged = {}
    for stage in ("4", None):
        staged["area", stage] = j.view("area%s" % (stage or ""), crop=SCALED, stage=stage, size=(8, 16), scale="area")
        staged["nearest", stage] = j.view("nearest%s" % (stage or ""), crop=SCALED, stage=stage, size=(24, 32), scale="nearest")
    k_both = j.view("both", select=(2, 12, 3), crop=ODD, stage="1", size=(12, 20), scale="area")
    k_same = j.view("identity", select=(0, None, 1), crop=(0, 0, H0, W))
    j.source("whole.agmv")
    k_same_scaled = j.view("identity-scaled", select=(0, T, 1), size=(16, 24), scale="area")
    j.source("whole-scaled.agmv", size=(16, 24), scale="area")
    st = j.run()["stats"]
    # which path ran: (frames, clip_bytes, staging_bytes)
    assert st[k_window] == [T, 4 * 24 * 16 * T, 0] and st[k_stride] == [6, 4 * W * H0 * 6, 0]
    assert st[k_range] == [8, 0, 0] and st[k_cut] == [8, 0, 0] and st[k_same] == [T, 0, 0]
    window_bytes = 4 * 32 * 20
    assert st[staged["area", "4"]] == [T, 4 * 16 * 8 * T, 4 * window_bytes] and st[staged["nearest", "4"]] == [T, 4 * 32 * 24 * T, 4 * window_bytes]
    assert st[staged["area", None]] == [T, 4 * 16 * 8 * T, T * window_bytes] and st[staged["nearest", None]] == [T, 4 * 32 * 24 * T, T * window_bytes]
    assert st[k_both] == [4, 4 * 20 * 12 * 4, 4 * 24 * 16] and st[k_same_scaled] == [T, 4 * 24 * 16 * T, 0]
    # consecutive full frames: the file of the sliced clip; the identity: the file of the call without a view; the batches change nothing
    assert j.read("range.view.agmv") == j.read("sliced.agmv")
    assert j.read("identity.view.agmv") == j.read("whole.agmv") and j.read("identity-scaled.view.agmv") == j.read("whole-scaled.agmv")
    for f in ("area", "nearest"):
        assert j.read(f + "4.view.agmv") == j.read(f + ".view.agmv")
    assert len({j.read(t + ".view.agmv") for t, _, _ in j.pairs}) >= len(j.pairs) - 4          # (different views, different files)


def test_schedules_opts_and_knobs(tmp_path):
    j = Jobs(tmp_path, "rgb24")
    for schedule in (FULL, PDIFS, ADAPTIVE):
        j.view("schedule%d" % schedule, select=(1, T, 1), crop=WINDOW, schedule=schedule)
        j.view("schedule%d-scaled" % schedule, select=(0, T, 2) if schedule == FULL else (1, T, 1), crop=SCALED, size=(8, 16), schedule=schedule)
    j.view("heavy", select=(0, T, 6), crop=WINDOW, opt=1)                       # three frames are enough for a heavy opt
    j.view("gba", crop=ODD, opt=5)                                              # a GBA opt without a target: its own scaler, on V
    j.view("lz77", select=(0, T, 2), crop=WINDOW, compression=2, opt=2)
    j.view("knobs", select=(0, 12, 1), crop=WINDOW, dither=8, stabilise=6, palette_refine=3)
    j.view("knobs-scaled", crop=SCALED, size=(8, 16), dither=8, stabilise=6, palette_refine=3, stage="5")
    j.view("fps", select=(0, T, 4), crop=(0, 0, H0, W), fps=15, schedule=FULL)
    k_fit = j.source("fit.agmv", fit="crop", size=(16, 16))
    assert VS.fit_window(H0, W, 16, 16) == (0, 8, 24, 24)
    j.view("fit", crop=(0, 8, 24, 24), size=(16, 16))
    k_fit_select = j.source("fit-select.agmv", fit="crop", size=(16, 16), select=[1, T, 2], scale="nearest")
    j.view("fit-select", select=(1, T, 2), crop=(0, 8, 24, 24), size=(16, 16), scale="nearest")
    st = j.run()["stats"]
    assert j.read("fit.agmv") == j.read("fit.view.agmv") and j.read("fit-select.agmv") == j.read("fit-select.view.agmv")
    assert st[k_fit] == [T, 4 * 16 * 16 * T, T * 4 * 24 * 24] and st[k_fit_select][0] == 6
    assert j.read("knobs.view.agmv") != j.read("schedule2.view.agmv")
    assert int.from_bytes(j.read("fps.view.agmv")[18:22], "little") == int.from_bytes(j.read("fps.cmp.agmv")[18:22], "little")


def test_a_view_too_short_after_the_cut_creates_no_file(tmp_path):
    """select= reaches past the clip and is cut to two frames: -2 from the library, which opened no file; so is a window whose size
    the encoder refuses (-3).  The stats of a refused call are zero; the next call is not disturbed."""
    tensor, _ = clips("nv12")
    np.save(tmp_path / "clip.npy", tensor)
    base = {"clip": "clip.npy", "fmt": "nv12"}
    enc = [dict(base, out="short.agmv", kw={"select": [11, 30, 1]}),
           dict(base, out="short-window.agmv", kw={"select": [2, 9, 3], "crop": list(WINDOW)}),
           dict(base, out="odd-size.agmv", kw={"crop": [0, 0, 10, 16]}),
           dict(base, out="area-up.agmv", kw={"crop": list(WINDOW), "size": [20, 24]}),
           dict(base, out="good.agmv", kw={"select": [9, 30, 1]})]
    res = run_child(tmp_path, enc)
    assert all("AGMV_EncodeViewDev refused its arguments (%d)" % rc in e for rc, e in zip((-2, -2, -3, -3), res["errors"])), res["errors"]
    assert res["errors"][4] == "" and res["stats"] == [[0, 0, 0]] * 4 + [[4, 0, 0]]
    assert [os.path.exists(tmp_path / e["out"]) for e in enc] == [False, False, False, False, True]
