"""Views of whole files: AGMV_DecodeViewDev / AGMV_DecodeViewTensorDev of libagmv_amd/libagmv.so and
libagmv_amd.decode_frames(frames=, crop=) on torch tensors.

The comparator is never the code under test: the file is decoded in full by the path without a view (decode_frames(path), which the
file tests hold to the reference), sliced in numpy (tests/view_cases.py), scaled in numpy (tests/upscale_cases.py) and written in
the layout or as a tensor by the numpy statements of tests/scale_cases.py and tests/tensor_cases.py; the view must deliver exactly
those bytes.  AGMV_GetViewStats shows which path ran: how far the LZ stage went, where the GPU stage started, whether the call was
run again from frame 0.  The clip is 24 frames of 64 x 48 (6 GOPs), its left quarter static so that P-frames hold COPY blocks;
AGMV_BATCH_FRAMES=8 puts GOP starts inside batches.  Child processes as in tests/test_gpu_upscale_files.py.  Needs an MI355X."""
import textwrap

import children as K
import numpy as np
import pytest

import deblock_cases as DK
import memseq_cases as MC
import pixfmt_cases as P
import scale_cases as SC
import tensor_cases as TC
import upscale_cases as U
import view_cases as V
import yuv_cases as Y

pytestmark = pytest.mark.gpu

W, H0, T = 64, 48, 24
FMT_VALUE = {"xrgb32": P.XRGB32, "rgb24": P.RGB24, "bgr24": P.BGR24, "rgba32": P.RGBA32, "rgb8p": P.RGB8P, "nv12": Y.NV12, "i420": Y.I420}
TENSOR = {"f32": TC.F32, "f16": TC.F16, "bf16": TC.BF16}
FILTER = {"nearest": U.NEAREST, "area": U.AREA, "bilinear": U.BILINEAR}
WHOLE = [0, 0, 1, 0, 0, 0, 0]

# job: clip (npy of the XRGB32 clip to encode, or none), compression, craft ([a, b]: chunk a replaced by the bytes of chunk b), path,
# views: [{fmt, value (the C call's fmt or type), size, scale, filt, mean, std, view ([first, count, step, x, y, w, h] or none), cap, frames
# ([start, stop, step] for decode_frames, or none), crop, py, frame_bytes, buf_frames, deblock (a strength: decode_frames once more with
# deblock= it and once with deblock=None, the restarts and libagmv_amd.deblock_stats() of each)}].  Answers one JSON line.
CHILD = textwrap.dedent("""
    import ctypes as C, json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    from libagmv_amd import abi, seq
    path = job["path"]
    if job.get("clip"):
        libagmv_amd.encode_frames(path, torch.from_numpy(np.load(job["clip"]).view(np.int32)).cuda(), schedule=libagmv_amd.SCHEDULE_FULL,
                                  compression=job.get("compression", 1))
    if job.get("craft"):
        data, at = open(path, "rb").read(), []
        p = data.find(b"AGFC")
        while p >= 0:
            at.append(p)
            p = data.find(b"AGFC", p + 16 + int.from_bytes(data[p + 12:p + 16], "little"))
        at.append(len(data))
        a, b = job["craft"]
        path = "crafted.agmv"
        open(path, "wb").write(data[:at[a]] + data[at[b]:at[b + 1]] + data[at[a + 1]:])
    L = seq.load_library()
    stats = abi.AGMV_VIEW_STATS()

    def view_stats():
        L.AGMV_GetViewStats(C.byref(stats))
        return [stats.lz_frames, stats.gpu_frames, stats.delivered, stats.restarts]
    before, info = libagmv_amd.decode_frames(path)
    np.save("native.npy", before.cpu().numpy().view(np.uint32))
    res = {"views": [], "frames": int(info.number_of_frames)}
    for k, d in enumerate(job["views"]):
        r = {}
        if d["py"]:
            kw = dict(fmt=d["fmt"], mean=d.get("mean"), std=d.get("std"), crop=tuple(d["crop"]) if d.get("crop") else None)
            if d.get("size"):
                kw.update(size=tuple(d["size"]), scale=d["scale"])
            fr = d.get("frames")
            if fr is not None:
                kw["frames"] = slice(*fr) if fr[1] is None else range(*fr) if k % 2 else tuple(fr)
            got, info2 = libagmv_amd.decode_frames(path, **kw)
            assert (info2.width, info2.height, info2.number_of_frames) == (info.width, info.height, info.number_of_frames)
            r["py_shape"], r["py_stats"] = list(got.shape), view_stats()
            np.save("py_%d.npy" % k, got.contiguous().view(torch.uint8).cpu().numpy().reshape(-1))
            for name, knob in (("on", d["deblock"]), ("off", None)) if d.get("deblock") else ():
                got, _ = libagmv_amd.decode_frames(path, deblock=knob, **kw)
                r[name + "_restarts"], r[name + "_stats"] = view_stats()[3], libagmv_amd.deblock_stats()
                np.save("%s_%d.npy" % (name, k), got.contiguous().view(torch.uint8).cpu().numpy().reshape(-1))
        buf = torch.full((d["buf_frames"], d["frame_bytes"]), 0xA5, dtype=torch.uint8, device="cuda")
        view = abi.AGMV_VIEW(*d["view"]) if d["view"] is not None else None
        th, tw = d["size"] if d.get("size") else (0, 0)
        tail = (tw, th, d.get("filt", 0), C.byref(view) if view is not None else None, d.get("cap", d["buf_frames"]), None)
        if d.get("mean") is not None:
            m, s = (C.c_float * 3)(*d["mean"]), (C.c_float * 3)(*d["std"])
            r["c_rc"] = L.AGMV_DecodeViewTensorDev(path.encode(), buf.data_ptr(), d["value"], m, s, *tail)
        else:
            r["c_rc"] = L.AGMV_DecodeViewDev(path.encode(), buf.data_ptr(), d["value"], *tail)
        torch.cuda.synchronize()
        r["c_stats"] = view_stats()
        np.save("c_%d.npy" % k, buf.cpu().numpy())
        res["views"].append(r)
    after, _ = libagmv_amd.decode_frames(path)
    res["same"] = bool(before.shape == after.shape and (before == after).all())
    print(json.dumps(res))
""")


def run_child(cwd, job, env=None):
    return K.run_child(cwd, CHILD, job, dict({"AGMV_BATCH_FRAMES": "8", "AGMV_LZ_DECODE_DEVICE": None}, **(env or {})), prelude="")


def case(fmt, view, frames=None, crop=None, size=None, scale="bilinear", norm=None, cap=None, py=True, buf_frames=None):
    """view: what the C call gets; frames, crop: the same selection as decode_frames takes it; buf_frames: the frames the C call's
    destination holds (default: as many as the view could deliver at most, plus one that must stay untouched)"""
    window = (view[6], view[5]) if view is not None and view[5] else (H0, W)
    h, w = size if size else window
    d = {"fmt": fmt, "view": view, "frames": frames, "crop": crop, "size": list(size) if size else None, "scale": scale, "py": py}
    if size:
        d["filt"] = FILTER[scale]
    if fmt in TENSOR:
        d["value"], (d["mean"], d["std"]) = TENSOR[fmt], TC.NORMS[norm]
        d["frame_bytes"] = 3 * h * w * np.dtype(TC.BITS[TENSOR[fmt]]).itemsize
    else:
        d["value"], d["frame_bytes"] = FMT_VALUE[fmt], SC.frame_bytes(FMT_VALUE[fmt], w, h)
    if cap is not None:
        d["cap"] = cap
    d["buf_frames"] = buf_frames if buf_frames is not None else T + 1
    return d


def expected(native, d):
    """the bytes of the view, uint8 [frames, frame bytes]"""
    sel = V.view(native, *(d["view"] or WHOLE), cap=d.get("cap"))
    if d["size"]:
        sel = U.scale(FILTER[d["scale"]], sel, d["size"][1], d["size"][0])
    if d["fmt"] in TENSOR:
        out = TC.from_packed(TC.table(TENSOR[d["fmt"]], d["mean"], d["std"]), sel)
    else:
        out = np.asarray(SC.from_packed(d["value"], sel))
    return np.ascontiguousarray(out).view(np.uint8).reshape(len(sel), d["frame_bytes"])


def check(tmp_path, views, res):
    native = np.load(tmp_path / "native.npy")
    assert res["same"], "a plain decode before and after the views differs"
    for k, (d, r) in enumerate(zip(views, res["views"])):
        exp = expected(native, d)
        n = len(exp)
        c = np.load(tmp_path / ("c_%d.npy" % k))
        assert r["c_rc"] == n and r["c_stats"][2] == n, (k, d, r)
        assert (c[:n] == exp).all(), (k, d, np.argwhere(c[:n] != exp)[:4])
        assert (c[n:] == 0xA5).all(), (k, d, "frames behind the view were written")
        if d["py"]:
            py = np.load(tmp_path / ("py_%d.npy" % k))
            assert r["py_shape"][0] == n and py.size == n * d["frame_bytes"], (k, d, r)
            assert (py.reshape(n, d["frame_bytes"]) == exp).all(), (k, d)
    return native


VIEWS = [
    case("xrgb32", [13, 8, 1, 0, 0, 0, 0], frames=[13, 21, 1]),                                    # 0: contiguous, across a batch boundary
    case("xrgb32", [5, 0, 3, 0, 0, 0, 0], frames=[5, None, 3]),                                    # 1: strided, to the end
    case("xrgb32", [20, 100, 1, 0, 0, 0, 0], frames=[20, 120, 1]),                                 # 2: cut at the file's end: 4 frames
    case("xrgb32", [24, 0, 1, 0, 0, 0, 0], frames=[24, 30, 1]),                                    # 3: behind the end: nothing
    case("xrgb32", [5, 0, 3, 0, 0, 0, 0], cap=3, py=False),                                        # 4: cap_frames below the view's length
    case("rgb24", [2, 0, 5, 5, 3, 20, 14], frames=[2, None, 5], crop=[3, 5, 14, 20]),              # 5
    case("nv12", [0, 0, 1, 6, 2, 32, 24], crop=[2, 6, 24, 32]),                                    # 6: a window alone: every frame
    case("rgb8p", [9, 4, 2, 8, 4, 16, 12], frames=[9, 17, 2], crop=[4, 8, 12, 16], size=(24, 32), scale="bilinear"),      # 7: x 2
    case("xrgb32", [3, 0, 4, 4, 4, 40, 30], frames=[3, None, 4], crop=[4, 4, 30, 40], size=(15, 20), scale="area"),       # 8
    case("i420", [3, 0, 4, 4, 4, 40, 30], frames=[3, None, 4], crop=[4, 4, 30, 40], size=(14, 20), scale="area"),         # 9: through d_scaled
    case("f16", [6, 5, 3, 12, 8, 28, 20], frames=[6, 21, 3], crop=[8, 12, 20, 28], norm="imagenet"),                       # 10
    case("f16", [6, 5, 3, 12, 8, 28, 20], frames=[6, 21, 3], crop=[8, 12, 20, 28], norm="imagenet", size=(28, 20)),        # 11
    case("bf16", [20, 0, 1, 0, 0, 0, 0], frames=[20, None, 1], norm="half"),                       # 12: full frames from a GOP start, a tensor
    case("xrgb32", list(WHOLE), frames=[0, None, 1]),                                              # 13: the identity view
    case("xrgb32", None, py=False),                                                                # 14: view == NULL
    case("rgb24", None, py=False),                                                                 # 15
    case("xrgb32", [0, 0, 1, 0, 0, W, H0], py=False),                                              # 16: the full frame as an explicit window
    case("xrgb32", [7, 0, 2, 1, 3, 5, 7], frames=[7, None, 2], crop=[3, 1, 7, 5]),                 # 17: straight into the caller's clip, word by word
]


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    p = tmp_path_factory.mktemp("view_clip") / "clip.npy"
    np.save(p, MC.synth_clip(W, H0, T))
    return str(p)


def test_views_equal_the_numpy_view_of_the_full_decode(tmp_path, clip):
    res = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "views": VIEWS})
    assert res["frames"] == T
    native = check(tmp_path, VIEWS, res)
    assert native.shape == (T, H0, W) and len(np.unique(native.reshape(T, -1), axis=0)) == T       # every frame its own content
    v = res["views"]
    assert v[0]["c_stats"] == [21, 9, 8, 0] and v[0]["py_stats"] == [21, 9, 8, 0]                 # LZ 0 .. 20, GPU 12 .. 20, no restart
    assert v[1]["c_stats"] == [24, 20, 7, 0]                                                       # GPU from frame 4
    assert v[2]["c_rc"] == 4 and v[3]["c_rc"] == 0 and v[3]["c_stats"] == [0, 0, 0, 0] and v[3]["py_shape"] == [0, H0, W]
    assert v[4]["c_rc"] == 3 and v[4]["c_stats"] == [12, 8, 3, 0]                                  # ends behind frame 11, the last one it needs
    assert v[12]["c_stats"] == [24, 4, 4, 0]                                                       # sunk from where they were decoded
    for k in (13, 14, 15, 16):                                                                     # the decode without a view
        assert v[k]["c_stats"] == [24, 24, 24, 0], k
    assert (np.load(tmp_path / "c_14.npy")[:T].reshape(-1).view(np.uint32) == native.reshape(-1)).all()


def test_batches_of_four_and_batches_without_a_selected_frame(tmp_path, clip):
    views = [case("xrgb32", [1, 0, 7, 0, 0, 0, 0], frames=[1, None, 7]), case("rgb24", [1, 0, 7, 5, 3, 20, 14], frames=[1, None, 7], crop=[3, 5, 14, 20]),
             VIEWS[0], VIEWS[9], VIEWS[11]]
    res = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "views": views}, {"AGMV_BATCH_FRAMES": "4"})
    check(tmp_path, views, res)
    assert res["views"][0]["c_stats"] == [23, 23, 4, 0] and res["views"][2]["c_stats"] == [21, 9, 8, 0]


def test_a_view_of_an_lz77_file(tmp_path, clip):
    views = [VIEWS[0], VIEWS[5], VIEWS[10]]
    res = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "compression": 2, "views": views})
    check(tmp_path, views, res)
    assert res["views"][0]["c_stats"] == [21, 9, 8, 0]


@pytest.mark.parametrize("lz", ["host", "device"])
def test_a_file_that_depends_on_the_frames_before_a_gop_start_is_decoded_again_from_frame_0(tmp_path, clip, lz):
    """chunk 8 replaced by the bytes of chunk 9: a P-frame's stream, COPY blocks included, stands where an I-frame is read, so the
    decode of GOP 2 from the fresh state is not the file's decode.  A view from frame 9 must still be the slice of the full decode
    of that same file -- and must say that it was run again: a crafted file that does not trigger the restart fails here."""
    views = [case("xrgb32", [9, 0, 2, 0, 0, 0, 0], frames=[9, None, 2]), case("rgb24", [9, 5, 1, 4, 4, 24, 16], frames=[9, 14, 1], crop=[4, 4, 16, 24]),
             VIEWS[0]]
    res = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "craft": [8, 9], "views": views},
                    {"AGMV_LZ_DECODE_DEVICE": "1"} if lz == "device" else None)
    assert res["frames"] == T
    check(tmp_path, views, res)
    for k in (0, 1):
        assert res["views"][k]["c_stats"][3] == 1 and res["views"][k]["py_stats"][3] == 1, (k, res["views"][k])
    assert res["views"][0]["c_stats"] == [24, 24, 8, 1]                                            # the run that delivered: the GPU stage from frame 0
    assert res["views"][2]["c_stats"] == [21, 9, 8, 0]                                             # GOP 3 on stands on its own again


@pytest.mark.parametrize("lz", ["host", "device"])
def test_a_view_that_is_decoded_again_with_the_deblocking_on_counts_the_delivering_run_alone(tmp_path, clip, lz):
    """the crafted file of the test above, its views from frame 9 with deblock=16 and then with deblock=None.  The first run of each is given
    up; what the deblocked call delivers is the numpy view of the statement's deblocked full decode of that file, and its statistics are
    those of the run from frame 0 alone: the frames 0 .. the last one the view needs, and the statement's counts over exactly those."""
    s = 16
    views = [dict(case("xrgb32", [9, 0, 2, 0, 0, 0, 0], frames=[9, None, 2]), deblock=s),
             dict(case("rgb24", [9, 5, 1, 4, 4, 24, 16], frames=[9, 14, 1], crop=[4, 4, 16, 24]), deblock=s)]
    res = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "craft": [8, 9], "views": views}, {"AGMV_LZ_DECODE_DEVICE": "1"} if lz == "device" else None)
    native = check(tmp_path, views, res)
    deblocked = DK.deblock(native, s)[0]
    assert (deblocked != native).any()
    for k, (d, r) in enumerate(zip(views, res["views"])):
        for name, full in (("on", deblocked), ("off", native)):
            exp = expected(full, d)
            got = np.load(tmp_path / ("%s_%d.npy" % (name, k)))
            assert got.size == exp.size and (got.reshape(exp.shape) == exp).all(), (k, name, np.argwhere(got.reshape(exp.shape) != exp)[:4])
            assert r[name + "_restarts"] == 1, (k, name, r)
        through = d["view"][0] + d["view"][2] * (len(exp) - 1) + 1                                # the GPU stage of the delivering run: frames 0 .. through - 1
        _, weak, strong = DK.deblock(native[:through], s)
        assert weak + strong
        assert r["on_stats"] == {"strength": s, "frames": through, "lines": DK.lines_examined(through, H0, W), "weak": weak, "strong": strong}, (k, r)
        assert r["off_stats"] == {"strength": 0, "frames": 0, "lines": 0, "weak": 0, "strong": 0}, (k, r)
    assert [d["view"][0] + d["view"][2] * (r["py_shape"][0] - 1) + 1 for d, r in zip(views, res["views"])] == [T, 14]


def test_the_frame_13_view_with_the_lz_stage_on_the_device(tmp_path, clip):
    views = [VIEWS[0], VIEWS[1], VIEWS[7]]
    res = run_child(tmp_path, {"clip": clip, "path": "clip.agmv", "views": views}, {"AGMV_LZ_DECODE_DEVICE": "1"})
    check(tmp_path, views, res)
    assert res["views"][0]["c_stats"] == [21, 9, 8, 0]
