"""What a view of a file (AGMV_VIEW of include/agmv.h) does before any GPU is touched: the one function that says which frames of
a batch belong to a view (agmv_view_in_batch of agmv_pipeline.h, exported for this test) against its statement by enumeration
(tests/view_cases.py), what AGMV_DecodeViewDev / AGMV_DecodeViewTensorDev refuse and in which order -- the expected values are the
header's list, written out here -- and the ValueErrors of decode_frames(frames=, crop=), which come before the library is loaded."""
import ctypes as C
import os
import subprocess

import pytest

import hostlib as H
import view_cases as V

SPLASH = os.path.join(H.ROOT, "tests", "golden", "agmv_splash.agmv")         # 119 frames of 320 x 240
FAKE = C.c_void_p(4096)                                                      # never dereferenced
u32 = C.c_uint32


@pytest.fixture(scope="module")
def L():
    from libagmv_amd import abi
    lib = H.lib()
    return abi.bind(lib, {"agmv_view_in_batch": (u32, (u32, u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32))),
                          "agmv_view_length": (u32, (u32, u32, u32, u32))})


def test_the_header_declares_the_view_and_the_tables_hold_it(L):
    from libagmv_amd import abi
    hdr = open(os.path.join(H.ROOT, "include", "agmv.h")).read()
    for name in ("AGMV_DecodeViewDev", "AGMV_DecodeViewTensorDev", "AGMV_GetViewStats"):
        assert name + "(" in hdr and name in abi.AGMV and hasattr(L, name)


def test_the_view_header_and_its_table_state_each_other():
    """include/agmv_hip_view.h against abi.HIP_VIEW the way tests/test_abi.py holds include/agmv_hip.h to abi.HIP: the same names, the
    header's return and parameter classes, the symbol exported and bound, a NULL context refused with its text before any HIP call"""
    import test_abi as TA
    from libagmv_amd import abi, build, hip
    protos = TA._prototypes("agmv_hip_view.h")
    assert set(protos) == set(abi.HIP_VIEW) == {"agmv_hip_view_frames_async"} and not set(abi.HIP_VIEW) & set(abi.HIP)
    for name, (restype, argtypes) in abi.HIP_VIEW.items():
        ret, params = protos[name]
        assert TA._ctypes_class(restype) == TA._c_class(ret, True), name
        assert [TA._ctypes_class(a) for a in argtypes] == [TA._c_class(p) for p in params], name
    build.build()
    G = hip.load_library()
    f = G.agmv_hip_view_frames_async
    assert list(f.argtypes) == list(abi.HIP_VIEW["agmv_hip_view_frames_async"][1]) and f.restype is C.c_int
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    assert f(None, p, 4, 4, 0, 1, 1, 0, 0, 4, 4, p, None) < 0 and b"NULL context" in G.agmv_hip_last_error()


def test_the_two_structures_have_the_headers_layout(tmp_path):
    from libagmv_amd import abi
    structs = (abi.AGMV_VIEW, abi.AGMV_VIEW_STATS)
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include \"agmv.h\"\nint main(void) {\n" + "".join(
        '    printf("%s %%zu%s\\n", sizeof(%s)%s);\n' % (s.__name__, " %zu" * len(s._fields_), s.__name__,
                                                     "".join(", offsetof(%s, %s)" % (s.__name__, f[0]) for f in s._fields_))
        for s in structs) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", str(src), "-I" + os.path.join(H.ROOT, "include"), "-o", exe], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert lines == ["%s %d%s" % (s.__name__, C.sizeof(s), "".join(" %d" % getattr(s, f[0]).offset for f in s._fields_)) for s in structs]
    assert C.sizeof(abi.AGMV_VIEW) == 28 and C.sizeof(abi.AGMV_VIEW_STATS) == 16


@pytest.mark.parametrize("cap", [4, 8, 12])
def test_selection_in_a_batch_is_the_enumeration(L, cap):
    """all first < 12, step 1 .. 9, count 0, 1, 5, files of 0 .. 30 frames, cut into batches of `cap`: per batch the function gives
    what the enumeration gives, and over the batches every frame of the view appears exactly once, at its view index, in order"""
    row, index = u32(), u32()
    for first in range(12):
        for step in range(1, 10):
            for count in (0, 1, 5):
                for nframes in range(31):
                    want = V.frames_of(first, step, count, nframes)
                    assert L.agmv_view_length(first, step, count, nframes) == len(want)
                    seen = []
                    for b0 in range(0, nframes, cap):
                        bn = min(cap, nframes - b0)
                        n = L.agmv_view_in_batch(first, step, count, b0, bn, C.byref(row), C.byref(index))
                        e = V.in_batch(first, step, count, b0, bn, nframes)
                        assert n == e[0] and (n == 0 or (row.value, index.value) == e[1:]), (first, step, count, nframes, b0, bn)
                        seen += [(index.value + k, b0 + row.value + k * step) for k in range(n)]
                    assert seen == list(enumerate(want)), (first, step, count, nframes)


def test_selection_at_the_edges_of_32_bits(L):
    row, index = u32(), u32()
    assert L.agmv_view_in_batch(0xFFFFFFF0, 7, 0, 0xFFFFFFF0, 15, C.byref(row), C.byref(index)) == 3 and (row.value, index.value) == (0, 0)
    assert L.agmv_view_in_batch(3, 0xFFFFFFFF, 0, 0, 16, C.byref(row), C.byref(index)) == 1 and (row.value, index.value) == (3, 0)
    assert L.agmv_view_in_batch(5, 1, 0, 0, 0, C.byref(row), C.byref(index)) == 0
    assert L.agmv_view_length(0, 1, 0, 0xFFFFFFFF) == 0xFFFFFFFF and L.agmv_view_length(0xFFFFFFFF, 1, 0, 0xFFFFFFFF) == 0


# ---- refusals: the header's list.  Baseline: RGB24, no target, the whole file as an explicit view, on the splash file.
def _view(first=0, count=0, step=1, x=0, y=0, width=0, height=0):
    from libagmv_amd import abi
    return abi.AGMV_VIEW(first, count, step, x, y, width, height)


AREA, BILINEAR = 2, 3
REFUSALS = [
    # 1: -1
    ("null-filename", dict(path=None), -1),
    ("unknown-format", dict(fmt=6), -1),
    ("unknown-filter-with-a-target", dict(w=16, h=16, filt=4), -1),
    ("step-0", dict(view=dict(step=0)), -1),
    ("window-width-0", dict(view=dict(width=0, height=8)), -1),
    ("window-height-0", dict(view=dict(width=8, height=0)), -1),
    ("x-with-a-zero-window", dict(view=dict(x=4)), -1),
    ("y-with-a-zero-window", dict(view=dict(y=4)), -1),
    # 2: -4, the target
    ("target-0x16", dict(w=0, h=16, filt=BILINEAR), -4),
    ("target-16x0", dict(w=16, h=0, filt=BILINEAR), -4),
    ("target-above-2^28", dict(w=1 << 14, h=(1 << 14) + 1, filt=BILINEAR), -4),
    # 3: -Error
    ("missing-file", dict(path="missing"), -2),
    ("bad-fourcc", dict(path="badfourcc"), None),                                    # (whatever AGMV_DecodeFramesFmtDev returns for it)
    # 4: 0
    ("no-destination", dict(dst=None), 0),
    ("no-destination-and-a-filter-nobody-reads", dict(dst=None, filt=99), 0),
    # 5: -4, the file decides
    ("window-past-the-right-edge", dict(view=dict(x=300, y=0, width=32, height=8)), -4),
    ("window-past-the-bottom", dict(view=dict(x=0, y=236, width=8, height=5)), -4),
    ("window-x-behind-the-frame", dict(view=dict(x=321, y=0, width=1, height=1)), -4),
    ("area-wider-than-the-window", dict(w=101, h=50, filt=AREA, view=dict(x=8, y=8, width=100, height=100)), -4),
    ("area-taller-than-the-window", dict(w=50, h=101, filt=AREA, view=dict(x=8, y=8, width=100, height=100)), -4),
    ("area-on-a-frame-above-2^24", dict(path="huge", w=16, h=16, filt=AREA), -4),
    ("nv12-over-an-odd-window", dict(fmt=16, view=dict(x=0, y=0, width=5, height=4)), -4),
    ("i420-over-an-odd-window", dict(fmt=17, view=dict(x=0, y=0, width=4, height=5)), -4),
    # the order: one pair per two adjacent classes
    ("-1-before-the-target", dict(view=dict(step=0), w=0, h=16, filt=BILINEAR), -1),
    ("unknown-filter-before-the-target", dict(w=0, h=16, filt=4), -1),
    ("the-target-before-the-file", dict(w=0, h=16, filt=BILINEAR, path="missing"), -4),
    ("the-file-before-the-destination", dict(path="missing", dst=None), -2),
    ("the-destination-before-the-window", dict(dst=None, view=dict(x=300, y=0, width=32, height=8)), 0),
]


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("view")
    data = open(SPLASH, "rb").read()
    le = lambda v: v.to_bytes(4, "little")
    made = {"badfourcc": b"AGMX" + data[4:], "huge": data[:8] + le(8192) + le(4096) + data[16:]}
    out = {None: None, "good": SPLASH.encode(), "missing": str(tmp / "missing.agmv").encode()}
    for name, content in made.items():
        out[name] = str(tmp / (name + ".agmv")).encode()
        open(out[name], "wb").write(content)
    return out


# (the two rules of the YUV layouts have no tensor form)
MATRIX = [(r, False) for r in REFUSALS] + [(r, True) for r in REFUSALS if r[1].get("fmt") not in (16, 17)]


@pytest.mark.parametrize("case,tensor", MATRIX, ids=["%s-%s" % ("tensor" if t else "frames", r[0]) for r, t in MATRIX])
def test_refusals_and_their_order(L, paths, case, tensor):
    """(the destination is never written and no device is opened: every one of these returns first, in the header's order)"""
    from libagmv_amd.abi import AGMV_INFO
    from libagmv_amd.abi import AGMV_VIEW_STATS
    _, change, code = case
    a = dict(dict(path="good", dst=FAKE, fmt=2, w=0, h=0, filt=0, view={}), **change)
    view, info = _view(**a["view"]), AGMV_INFO()
    if code is None:
        code = L.AGMV_DecodeFramesFmtDev(paths[a["path"]], None, 2, 0, None)
        assert code < 0
    if tensor:
        mean, std = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
        call = lambda v: L.AGMV_DecodeViewTensorDev(paths[a["path"]], a["dst"], 0 if a["fmt"] == 6 else 2, mean, std, a["w"], a["h"], a["filt"], v, 4, C.byref(info))
    else:
        call = lambda v: L.AGMV_DecodeViewDev(paths[a["path"]], a["dst"], a["fmt"], a["w"], a["h"], a["filt"], v, 4, C.byref(info))
    assert call(C.byref(view)) == code
    if not a["view"]:
        assert call(None) == code                                                # view == NULL is the whole file
    if code == 0:
        assert (info.width, info.height, info.number_of_frames) == (320, 240, 119)
    stats = AGMV_VIEW_STATS(9, 9, 9, 9)
    L.AGMV_GetViewStats(C.byref(stats))
    assert (stats.lz_frames, stats.gpu_frames, stats.delivered, stats.restarts) == (0, 0, 0, 0)      # no call reached the decode


def test_a_refused_normalisation_is_minus_one(L, paths):
    mean, std = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 0, 1)
    assert L.AGMV_DecodeViewTensorDev(paths["good"], FAKE, 2, mean, std, 0, 0, 0, None, 4, None) == -1
    assert L.AGMV_DecodeViewTensorDev(paths["good"], FAKE, 2, None, std, 0, 0, 0, None, 4, None) == -1
    assert L.AGMV_DecodeViewTensorDev(paths["missing"], FAKE, 2, mean, std, 0, 16, BILINEAR, None, 4, None) == -1


def test_a_view_without_a_frame_opens_no_device(L, paths):
    """`first` at or behind the end: 0 frames, and the fake destination is never written"""
    for first in (119, 120, 0xFFFFFFFF):
        v = _view(first=first, step=3)
        assert L.AGMV_DecodeViewDev(paths["good"], FAKE, 2, 0, 0, 0, C.byref(v), 4, None) == 0
    v = _view(first=5, step=3, x=4, y=4, width=8, height=8)
    assert L.AGMV_DecodeViewDev(paths["good"], FAKE, 2, 0, 0, 0, C.byref(v), 0, None) == 0              # cap_frames 0 of a real view


BAD_FRAMES = ["0:4", 4, (0, 4), (0, 4, 0), (0, 4, -1), (0.0, 4, 1), (True, 4, 1), range(4, 0, -1), range(-2, 4), slice(None, None, -1), slice(0, 4, 0),
              slice(0.5, 4), [0, 1, 2]]
BAD_CROPS = ["4x4", (0, 0, 4), (0, 0, 0, 4), (0, 0, 4, 0), (-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 4.0, 4), (0, 0, True, 4)]


def test_seq_refuses_bad_frames_and_crops_before_the_library_is_loaded(monkeypatch):
    import libagmv_amd
    from libagmv_amd import seq

    def reached():
        raise AssertionError("the library was called")
    monkeypatch.setattr(seq, "load_library", reached)
    for frames in BAD_FRAMES:
        for fmt in ("xrgb32", "f16"):
            with pytest.raises(ValueError, match="frames"):
                libagmv_amd.decode_frames(SPLASH, fmt=fmt, frames=frames)
    for crop in BAD_CROPS:
        for fmt in ("rgb24", "f32"):
            with pytest.raises(ValueError, match="crop"):
                libagmv_amd.decode_frames(SPLASH, fmt=fmt, crop=crop)
    for kw in (dict(frames=range(0, 8, 2)), dict(frames=slice(None, None, 4)), dict(frames=(1, 9, 3)), dict(crop=(0, 0, 8, 8)), dict(frames=range(5, 5))):
        with pytest.raises(AssertionError, match="the library was called"):
            libagmv_amd.decode_frames(SPLASH, **kw)                                # a good value goes on to the library


def test_seq_refuses_an_impossible_window_after_the_header_is_read(monkeypatch):
    """a crop outside the frame, "area" above the window, a YUV layout over an odd window: ValueError behind the header call, before
    anything is allocated (only the call without a destination reaches the library)"""
    import torch
    import libagmv_amd
    from libagmv_amd import seq
    lib = seq.load_library()
    calls = []

    class Watch:
        def __getattr__(self, name):
            f = getattr(lib, name)

            def call(*a):
                calls.append((name, a[1]))
                return f(*a)
            return call
    monkeypatch.setattr(seq, "load_library", lambda: Watch())
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a tensor was allocated")))
    for crop in ((0, 0, 241, 8), (0, 0, 8, 321), (236, 0, 5, 8), (0, 316, 8, 5)):
        with pytest.raises(ValueError, match="inside"):
            libagmv_amd.decode_frames(SPLASH, crop=crop)
        with pytest.raises(ValueError, match="inside"):
            libagmv_amd.decode_frames(SPLASH, fmt="f16", crop=crop, frames=range(2))
    with pytest.raises(ValueError, match="area"):
        libagmv_amd.decode_frames(SPLASH, fmt="rgb24", crop=(0, 0, 100, 100), size=(50, 101), scale="area")
    with pytest.raises(ValueError, match="even"):
        libagmv_amd.decode_frames(SPLASH, fmt="nv12", crop=(0, 0, 5, 8))
    assert calls and all(c in (("AGMV_DecodeViewDev", None), ("AGMV_DecodeViewTensorDev", None)) for c in calls)
