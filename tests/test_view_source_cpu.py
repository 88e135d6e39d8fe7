"""What a view of a source clip (AGMV_EncodeViewDev of include/agmv.h, agmv_hip_view_source_async of include/agmv_hip_view_source.h)
does before any GPU is touched: the new header against its ctypes table, the way tests/test_view_cpu.py holds the decoder's view
header; what AGMV_EncodeViewDev refuses and in which order -- the expected values are the header's list, written out here; the
pointers are never read and no file is created; the ValueErrors of encode_frames(select=, crop=, fit=), which come before the library
is loaded; and the window of fit="crop" against a search without divisions."""
import ctypes as C
import os

import pytest

import hostlib as H
import view_source_cases as VS

FAKE = C.c_void_p(4096)                                                      # never dereferenced
NEAREST, AREA, BILINEAR = 1, 2, 3
FULL, PDIFS, ADAPTIVE = 1, 2, 3
RGB24, NV12, I420 = 2, 16, 17
N, SW, SH = 13, 40, 24                                                       # the clip of the baseline


@pytest.fixture(scope="module")
def L():
    return H.lib()


def test_the_header_declares_the_entry_points_and_the_tables_hold_them(L):
    from libagmv_amd import abi
    hdr = open(os.path.join(H.ROOT, "include", "agmv.h")).read()
    for name in ("AGMV_EncodeViewDev", "AGMV_GetEncodeViewStats"):
        assert name + "(" in hdr and name in abi.AGMV and hasattr(L, name)
    assert "AGMV_VIEW_STAGE_FRAMES" in hdr


def test_the_view_source_header_and_its_table_state_each_other():
    """include/agmv_hip_view_source.h against abi.HIP_VIEW_SOURCE: the same names, the header's return and parameter classes, the
    symbol exported and bound, a NULL context refused with its text before any HIP call; disjoint from the other three tables"""
    import test_abi as TA
    from libagmv_amd import abi, build, hip
    name = "agmv_hip_view_source_async"
    protos = TA._prototypes("agmv_hip_view_source.h")
    assert set(protos) == set(abi.HIP_VIEW_SOURCE) == {name}
    assert not set(abi.HIP_VIEW_SOURCE) & (set(abi.HIP) | set(abi.HIP_VIEW) | set(abi.HIP_STABILISE))
    restype, argtypes = abi.HIP_VIEW_SOURCE[name]
    ret, params = protos[name]
    assert TA._ctypes_class(restype) == TA._c_class(ret, True)
    assert [TA._ctypes_class(a) for a in argtypes] == [TA._c_class(p) for p in params]
    build.build()
    G = hip.load_library()
    f = getattr(G, name)
    assert list(f.argtypes) == list(argtypes) and f.restype is C.c_int
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    for fmt in (1, 2, NV12):
        assert f(None, fmt, p, 4, 4, 0, 1, 1, 0, 0, 4, 4, p, None) < 0 and b"NULL context" in G.agmv_hip_last_error()


def test_the_stats_structure_has_the_headers_layout(tmp_path):
    import subprocess
    from libagmv_amd import abi
    s = abi.AGMV_ENCODE_VIEW_STATS
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include \"agmv.h\"\nint main(void) {\n"
                   '    printf("%%zu%s\\n", sizeof(%s)%s);\n' % (" %zu" * len(s._fields_), s.__name__, "".join(", offsetof(%s, %s)" % (s.__name__, f[0]) for f in s._fields_))
                   + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", str(src), "-I" + os.path.join(H.ROOT, "include"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(s)] + [getattr(s, f[0]).offset for f in s._fields_]


# ---- refusals: the header's list.  Baseline: 13 frames of 40 x 24 RGB24, the whole clip as an explicit view, no target, OPT_III, PDIFS --
# which no case leaves as it is: every case below is refused before a device is opened.
def _view(first=0, count=0, step=1, x=0, y=0, width=0, height=0):
    from libagmv_amd import abi
    return abi.AGMV_VIEW(first, count, step, x, y, width, height)


WIN = dict(x=4, y=4, width=16, height=8)
REFUSALS = [
    # -1
    ("null-filename", dict(path=None), -1),
    ("null-frames", dict(src=None), -1),
    ("unknown-format", dict(fmt=6), -1),
    ("unknown-yuv-flag", dict(fmt=NV12 | 0x400), -1),
    ("flags-on-a-byte-layout", dict(fmt=RGB24 | 0x100), -1),
    ("opt-0", dict(opt=0), -1),
    ("opt-9", dict(opt=9), -1),
    ("quality-0", dict(quality=0), -1),
    ("quality-4", dict(quality=4), -1),
    ("compression-0", dict(compression=0), -1),
    ("compression-3", dict(compression=3), -1),
    ("schedule-0", dict(schedule=0), -1),
    ("schedule-4", dict(schedule=4), -1),
    ("bilinear-with-a-target", dict(w=16, h=8, filt=BILINEAR), -1),
    ("filter-0-with-a-target", dict(w=16, h=8, filt=0), -1),
    ("filter-0-with-half-a-target", dict(w=0, h=8, filt=0), -1),
    ("step-0", dict(view=dict(step=0)), -1),
    ("window-width-0", dict(view=dict(width=0, height=8)), -1),
    ("window-height-0", dict(view=dict(width=8, height=0)), -1),
    ("x-with-a-zero-window", dict(view=dict(x=4)), -1),
    ("y-with-a-zero-window", dict(view=dict(y=4)), -1),
    # -5
    ("adaptive-with-a-track", dict(schedule=ADAPTIVE, track=True), -5),
    # -3: the source
    ("source-width-0", dict(sw=0), -3),
    ("source-height-0", dict(sh=0), -3),
    ("source-above-2^28", dict(sw=1 << 15, sh=(1 << 13) + 4), -3),
    # -3: the window
    ("window-past-the-right-edge", dict(view=dict(x=28, y=0, width=16, height=8)), -3),
    ("window-past-the-bottom", dict(view=dict(x=0, y=20, width=8, height=8)), -3),
    ("window-x-behind-the-frame", dict(view=dict(x=41, y=0, width=4, height=4)), -3),
    ("x-that-wraps", dict(view=dict(x=0xFFFFFFFC, y=0, width=8, height=8)), -3),
    ("y-that-wraps", dict(view=dict(x=0, y=0xFFFFFFFF, width=8, height=8)), -3),
    ("nv12-of-odd-width-with-a-window", dict(fmt=NV12, sw=41, view=WIN), -3),
    ("i420-of-odd-height-with-a-stride", dict(fmt=I420, sh=25, view=dict(step=2)), -3),
    # -3: without a target, the size AGMV_EncodeFramesDev refuses
    ("window-width-no-multiple-of-4", dict(view=dict(x=0, y=0, width=10, height=8)), -3),
    ("window-height-no-multiple-of-4", dict(view=dict(x=0, y=0, width=8, height=10)), -3),
    ("full-frame-no-multiple-of-4", dict(sw=42, view=dict(step=2)), -3),
    ("gba-window-of-one-pixel", dict(opt=5, view=dict(x=3, y=3, width=1, height=1)), -3),
    # -3: with a target, what AGMV_EncodeFramesScaledDev refuses for a source of the window's size
    ("target-no-multiple-of-4", dict(w=18, h=8, filt=AREA, view=WIN), -3),
    ("target-0x8", dict(w=0, h=8, filt=NEAREST, view=WIN), -3),
    ("target-8x0", dict(w=8, h=0, filt=NEAREST, view=WIN), -3),
    ("gba-with-a-target", dict(w=8, h=8, filt=NEAREST, opt=5, view=WIN), -3),
    ("nds-with-a-target", dict(w=8, h=8, filt=NEAREST, opt=8, view=WIN), -3),
    ("area-wider-than-the-window", dict(w=20, h=8, filt=AREA, view=WIN), -3),
    ("area-taller-than-the-window", dict(w=16, h=12, filt=AREA, view=WIN), -3),
    ("area-fits-the-frame-but-not-the-window", dict(w=24, h=16, filt=AREA, view=WIN), -3),
    ("area-on-a-window-above-2^24", dict(sw=8192, sh=4096, w=16, h=16, filt=AREA, view=dict(x=0, y=0, width=8192, height=2052)), -3),
    # -2: the view's length
    ("first-at-the-end", dict(view=dict(first=13)), -2),
    ("first-behind-the-end", dict(view=dict(first=0xFFFFFFFF, step=7)), -2),
    ("three-frames-by-count", dict(view=dict(count=3)), -2),
    ("three-frames-by-stride", dict(view=dict(first=1, step=5)), -2),
    ("three-frames-after-the-cut", dict(view=dict(first=10, count=8)), -2),
    ("a-clip-of-three-frames", dict(n=3), -2),
    ("one-frame-with-a-heavy-opt", dict(opt=1, view=dict(first=12)), -2),
    ("no-frame-with-the-full-schedule", dict(schedule=FULL, view=dict(first=13, **WIN)), -2),
    ("no-frame-with-a-target", dict(w=8, h=8, filt=AREA, view=dict(first=20, **WIN)), -2),
    # the order: pairs from different classes
    ("-1-before--5", dict(view=dict(step=0), schedule=ADAPTIVE, track=True), -1),
    ("-1-before--3", dict(fmt=6, sw=0), -1),
    ("-1-before--2", dict(view=dict(step=0, first=13)), -1),
    ("unknown-filter-before-the-target", dict(w=18, h=8, filt=BILINEAR, view=WIN), -1),
    ("-5-before--3", dict(schedule=ADAPTIVE, track=True, sw=0), -5),
    ("-5-before--2", dict(schedule=ADAPTIVE, track=True, view=dict(first=13)), -5),
    ("-3-before--2-the-source", dict(sh=0, view=dict(first=13)), -3),
    ("-3-before--2-the-window", dict(view=dict(first=13, x=28, y=0, width=16, height=8)), -3),
    ("-3-before--2-the-target", dict(w=18, h=8, filt=AREA, view=dict(first=13, **WIN)), -3),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_and_their_order(L, tmp_path, case):
    from libagmv_amd.abi import AGMV_ENCODE_VIEW_STATS
    _, change, code = case
    out = str(tmp_path / "out.agmv").encode()
    a = dict(dict(path=out, src=FAKE, fmt=RGB24, n=N, sw=SW, sh=SH, view={}, w=0, h=0, filt=0, opt=3, quality=3, compression=1, schedule=PDIFS, track=False), **change)

    def call(v):
        if a["track"]:
            assert L.AGMV_SetAudioDev(FAKE, 1, 48000, 48000, 2) == 0
        return L.AGMV_EncodeViewDev(a["path"], a["src"], a["fmt"], a["n"], a["sw"], a["sh"], v, a["w"], a["h"], a["filt"], 24, a["opt"], a["quality"], a["compression"],
                                    a["schedule"])
    view = _view(**a["view"])
    assert call(C.byref(view)) == code
    if not a["view"]:
        assert call(None) == code                                                # view == NULL is the whole clip
    if a["track"]:
        # the track is consumed whatever the call returns: the same call again, with a source nobody can encode, is no longer -5
        a["track"] = False
        assert L.AGMV_EncodeViewDev(out, FAKE, RGB24, N, 0, SH, None, 0, 0, 0, 24, 3, 3, 1, ADAPTIVE) == -3
    stats = AGMV_ENCODE_VIEW_STATS(9, 9, 9)
    L.AGMV_GetEncodeViewStats(C.byref(stats))
    assert (stats.frames, stats.clip_bytes, stats.staging_bytes) == (0, 0, 0)
    assert not os.path.exists(out)


def _cpu_clip(shape=(N, SH, SW, 3), dtype=None):
    import torch
    return torch.zeros(shape, dtype=dtype or torch.uint8)


BAD_SELECTS = ["0:4", 4, (0, 4), (0, 4, 0), (0, 4, -1), (0.0, 4, 1), (True, 4, 1), range(4, 0, -1), range(-2, 4), slice(None, None, -1), slice(0, 4, 0),
               slice(0.5, 4), [0, 1, 2]]
BAD_CROPS = ["4x4", (0, 0, 4), (0, 0, 0, 4), (0, 0, 4, 0), (-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 4.0, 4), (0, 0, True, 4)]


def test_seq_refuses_bad_arguments_before_the_library_is_loaded(monkeypatch, tmp_path):
    import torch
    import libagmv_amd
    from libagmv_amd import seq

    def reached():
        raise AssertionError("the library was called")
    monkeypatch.setattr(seq, "load_library", reached)
    out, clip = str(tmp_path / "out.agmv"), _cpu_clip()
    for select in BAD_SELECTS:
        with pytest.raises(ValueError, match="encode_frames: select"):
            libagmv_amd.encode_frames(out, clip, select=select)
    for crop in BAD_CROPS:
        with pytest.raises(ValueError, match="encode_frames: crop"):
            libagmv_amd.encode_frames(out, clip, crop=crop)
    for kw in (dict(fit="crop"), dict(fit="crop", size=(8, 8), crop=(0, 0, 8, 8)), dict(fit="pad", size=(8, 8)), dict(fit=True, size=(8, 8))):
        with pytest.raises(ValueError, match="fit"):
            libagmv_amd.encode_frames(out, clip, **kw)
    # an empty selection, a window outside the frame: after the clip's geometry is known, still before the library
    for select in (range(13, 20), range(5, 5), slice(20, None), (13, 14, 1)):
        with pytest.raises(ValueError, match="takes no frame"):
            libagmv_amd.encode_frames(out, clip, select=select)
    for crop in ((0, 0, 25, 8), (0, 0, 8, 41), (20, 0, 5, 8), (0, 36, 8, 5)):
        with pytest.raises(ValueError, match="inside"):
            libagmv_amd.encode_frames(out, clip, crop=crop)
    # none of the three goes with a tensor clip
    model = _cpu_clip((N, 3, SH, SW), torch.float32)
    for kw in (dict(select=range(0, 8, 2)), dict(crop=(0, 0, 8, 8)), dict(select=slice(None, None, 4), crop=(0, 0, 8, 8))):
        with pytest.raises(ValueError, match="tensor clip"):
            libagmv_amd.encode_frames(out, model, **kw)
        with pytest.raises(ValueError, match="tensor clip"):
            libagmv_amd.encode_frames(out, model.half(), fmt="f16", **kw)
    # a good value goes on: to the device check, which a host tensor fails, before the library
    for kw in (dict(select=range(0, 8, 2)), dict(select=slice(None, None, 4)), dict(select=(1, 9, 3)), dict(crop=(1, 3, 8, 8)), dict(fit="crop", size=(16, 16))):
        with pytest.raises(ValueError, match="must be on"):
            libagmv_amd.encode_frames(out, clip, **kw)
    assert not os.path.exists(out)


SIZES = [(sh, sw, th, tw) for sh in (1, 2, 9, 24, 45, 1080) for sw in (1, 3, 16, 40, 1920) for th in (1, 3, 8, 16, 160, 240) for tw in (1, 4, 16, 240, 320)]


def test_fit_windows_against_a_search_without_divisions():
    from libagmv_amd import fit_window
    assert len(SIZES) >= 300
    seen_h, seen_w, seen_full = 0, 0, 0
    for sh, sw, th, tw in SIZES:
        want = VS.fit_window(sh, sw, th, tw)
        if 0 in want[2:]:
            with pytest.raises(ValueError, match="fit_window"):
                fit_window(sh, sw, th, tw)
            continue
        top, left, ch, cw = got = fit_window(sh, sw, th, tw)
        assert got == want and (ch, cw) == VS.fit_by_search(sh, sw, th, tw), (sh, sw, th, tw)
        # inside the source, centred to the pixel
        assert 0 <= top and top + ch <= sh and 0 <= left and left + cw <= sw
        assert 0 <= (sh - ch - top) - top <= 1 and 0 <= (sw - cw - left) - left <= 1
        # the aspect of the target to within one pixel of the axis that was cut, and never beyond it
        assert ch == sh or cw == sw
        if ch == sh:
            assert cw * th <= ch * tw < (cw + 1) * th or cw == sw
        if cw == sw:
            assert ch * tw <= cw * th < (ch + 1) * tw or ch == sh
        # the full frame where the aspects agree
        if sw * th == sh * tw:
            assert got == (0, 0, sh, sw)
            seen_full += 1
        seen_h += ch < sh
        seen_w += cw < sw
    assert seen_h > 20 and seen_w > 20 and seen_full > 5
    assert fit_window(1080, 1920, 240, 320) == (0, 240, 1080, 1440) and fit_window(1080, 1920, 160, 240) == (0, 150, 1080, 1620)
    assert fit_window(24, 40, 16, 16) == (0, 8, 24, 24)
    for bad in ((0, 4, 4, 4), (4, 4, 4, 0), (4.0, 4, 4, 4), (True, 4, 4, 4), (-1, 4, 4, 4)):
        with pytest.raises(ValueError, match="fit_window"):
            fit_window(*bad)


def test_the_statement_reads_each_layout_by_its_rule():
    """the numpy statement on a clip whose answer is known: the window of the packed clip, whatever the layout that held it"""
    import numpy as np
    import scale_cases as SC
    rng = np.random.default_rng(3)
    pix = rng.integers(0, 1 << 24, (5, 6, 8), dtype=np.uint32)
    for fmt in SC.BYTE_LAYOUTS:
        raw = SC.from_packed(fmt, pix)
        assert (VS.view(fmt, raw, 8, 6, 1, 0, 2, 3, 1, 4, 5) == pix[1::2, 1:6, 3:7]).all()
    for fmt in SC.YUV_PLAIN + SC.YUV_709F:
        raw = SC.from_packed(fmt, pix)
        full = SC.to_packed(fmt, raw, 8, 6)
        assert (VS.view(fmt, raw, 8, 6, 0, 2, 3, 1, 1, 3, 3) == full[0::3][:2, 1:4, 1:4]).all()
        # an odd window still takes the chroma of the source's 2 x 2 cells: pixels (1, 1) and (2, 2) lie in different cells
        assert VS.view(fmt, raw, 8, 6, x=1, y=1, width=3, height=3).shape == (5, 3, 3)
