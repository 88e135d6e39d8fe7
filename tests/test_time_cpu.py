"""What encoding at another frame rate (AGMV_EncodeViewRateDev of include/agmv.h, agmv_hip_time_frames_async of include/agmv_hip_time.h)
states and does before any GPU is touched: the numpy statement of tests/time_cases.py against what the header says follows from the
rule; the new header against its ctypes table, the way tests/test_view_source_cpu.py holds its header; the two structures against a
compiled offsetof program; what AGMV_EncodeViewRateDev refuses and in which order -- the expected values are the header's list,
written out here, the pointers are never read and no file is created; and the ValueErrors of encode_frames(rate=, time=), which
come before the library is loaded."""
import ctypes as C
import os

import numpy as np
import pytest

import hostlib as H
import time_cases as TC

FAKE = C.c_void_p(4096)                                                      # never dereferenced
NEAREST, AREA, BILINEAR = 1, 2, 3
FULL, PDIFS, ADAPTIVE = 1, 2, 3
RGB24, NV12, I420 = 2, 16, 17
N, SW, SH = 13, 40, 24                                                       # the clip of the baseline

PAIRS = TC.reduced_pairs(12)
AREA_PAIRS = [(s, d) for s, d in PAIRS if d <= s] + [(65535, 1), (65535, 65534)]
NEAREST_PAIRS = PAIRS + [(65535, 1), (65535, 65534), (2, 5)]


# ---- the statement ----
def _outputs(sn, dn, nv):
    """the j worth looking at: all of a short result, both ends and the middle of a long one"""
    m = nv * dn // sn
    return range(m) if m <= 64 else sorted(set(list(range(8)) + list(range(m // 2 - 4, m // 2 + 4)) + list(range(m - 8, m))))


@pytest.mark.parametrize("sn,dn", AREA_PAIRS, ids=["%d-%d" % p for p in AREA_PAIRS])
def test_area_weights(sn, dn):
    nv = 3 * sn + 1 if sn <= 12 else sn
    m = nv * dn // sn
    assert m >= 1 and (m + 1) * sn > nv * dn >= m * sn                          # the last target interval inside V, the next one not
    for j in _outputs(sn, dn, nv):
        w = TC.weights(sn, dn, j)
        assert sum(wt for _, wt in w) == sn and all(0 < wt <= dn for _, wt in w)
        ks = [k for k, _ in w]
        assert ks == list(range(ks[0], ks[-1] + 1)) and 0 <= ks[0] and ks[-1] < nv
        assert ks[0] == j * sn // dn and ks[-1] == ((j + 1) * sn - 1) // dn
    if sn <= 12:
        users = {}
        for j in range(m):
            for k, _ in TC.weights(sn, dn, j):
                users.setdefault(k, []).append(j)
        assert max(len(u) for u in users.values()) <= 2                        # a frame of V has weight in at most two frames of R
        reads = TC.frame_reads(nv, sn, dn, TC.AREA)
        assert reads == sum(len(u) for u in users.values()) <= nv + m - 1
        assert reads == m * sn // dn + m - m // dn                             # the closed form the library reports


@pytest.mark.parametrize("sn,dn", NEAREST_PAIRS, ids=["%d-%d" % p for p in NEAREST_PAIRS])
def test_nearest_index_equals_a_search_without_division(sn, dn):
    nv = 3 * sn + 1 if sn <= 12 else sn
    m = nv * dn // sn
    for j in (range(m) if m <= 64 else list(range(40)) + list(range(m - 40, m))):
        k = TC.nearest_index(sn, dn, j)
        if sn <= 12 or j < 3:
            assert k == TC.nearest_by_search(sn, dn, j)
        assert 0 <= k < nv and 2 * k * dn <= (2 * j + 1) * sn < 2 * (k + 1) * dn    # the centre of the target interval lies in frame k
    assert TC.frame_reads(nv, sn, dn, TC.NEAREST) == m


@pytest.fixture(scope="module")
def clip():
    v = TC.moving_packed(37, 8, 12, 5)
    v.setflags(write=False)
    return v


def test_one_to_one_is_the_identity(clip):
    for filt in (TC.AREA, TC.NEAREST):
        for src, dst in ((1, 1), (3, 3), (65535, 65535)):
            assert (TC.resample(clip, src, dst, filt) == clip).all()
    high = clip | np.uint32(0x7E000000)
    assert (TC.resample(high, 1, 1, TC.AREA) == clip).all()                    # bits 24 .. 31 of R are 0


@pytest.mark.parametrize("k", [2, 3, 4, 5, 12, 37])
def test_k_to_one(clip, k):
    m = clip.shape[0] // k
    ch = np.stack([(clip >> s) & 0xFF for s in (16, 8, 0)]).astype(np.uint64)[:, :m * k].reshape(3, m, k, *clip.shape[1:])
    mean = (ch.sum(axis=2) + k // 2) // k
    assert (TC.resample(clip, k, 1, TC.AREA) == (mean[0] << 16 | mean[1] << 8 | mean[2])).all()
    assert (TC.resample(clip, 2 * k, 2, TC.AREA) == TC.resample(clip, k, 1, TC.AREA)).all()       # reduced first
    assert (TC.resample(clip, k, 1, TC.NEAREST) == clip[k // 2::k][:m]).all()


@pytest.mark.parametrize("sn,dn", [p for p in PAIRS if p[1] <= p[0]], ids=lambda v: str(v))
def test_flat_pixels_stay_flat_and_outputs_lie_within_their_taps(clip, sn, dn):
    for filt in (TC.AREA, TC.NEAREST):
        r = TC.resample(clip, sn, dn, filt)
        assert r.shape[0] == TC.length(clip.shape[0], sn, dn) and (r >> 24 == 0).all()
        assert (r[(slice(None),) + TC.FLAT] == clip[(0,) + TC.FLAT]).all()
        for j in range(r.shape[0]):
            ks = [k for k, _ in TC.taps(sn, dn, filt, j)]
            for s in (16, 8, 0):
                t = (clip[ks] >> s) & 0xFF
                o = (r[j] >> s) & 0xFF
                assert (t.min(axis=0) <= o).all() and (o <= t.max(axis=0)).all()
    assert (clip[:, 0, 0] != clip[0, 0, 0]).any()                              # (the clip does move outside the flat region)


def test_the_accumulators_bound():
    white = TC.white_clip(65535, 1, 2)
    assert (TC.resample(white, 65535, 1, TC.AREA) == 0x00FFFFFF).all()
    assert 255 * 65535 + 32767 < 1 << 32
    assert TC.length(65535, 65535, 65534) == 65534
    for j in (0, 65533):
        assert (TC.resample(white, 65535, 65534, TC.AREA, j0=j, count=1) == 0x00FFFFFF).all()
    up = TC.resample(TC.moving_packed(4, 2, 2, 1), 2, 5, TC.NEAREST)
    assert up.shape[0] == 10 and [TC.nearest_index(2, 5, j) for j in range(10)] == [0, 0, 1, 1, 1, 2, 2, 3, 3, 3]


def test_the_statement_reads_each_layout_by_its_rule():
    import scale_cases as SC
    for fmt in SC.LAYOUTS + SC.YUV_709F:
        raw, packed = TC.moving_clip(fmt, 9, 8, 16, 7)
        got = TC.resample_source(fmt, raw, 16, 8, 1, 2, 3, 1, 9, 5, 4, 2, TC.AREA)
        v = packed[1::2, 1:6, 3:12]
        assert got.shape == (2, 5, 9) and (got == TC.resample(v, 2, 1, TC.AREA)).all()
        assert (packed[(slice(None),) + TC.FLAT] == packed[(0,) + TC.FLAT]).all() and (packed[1:] != packed[:-1]).any()


# ---- the headers ----
@pytest.fixture(scope="module")
def L():
    return H.lib()


def test_the_header_declares_the_entry_points_and_the_tables_hold_them(L):
    from libagmv_amd import abi
    hdr = open(os.path.join(H.ROOT, "include", "agmv.h")).read()
    for name in ("AGMV_EncodeViewRateDev", "AGMV_GetEncodeRateStats"):
        assert name + "(" in hdr and name in abi.AGMV and hasattr(L, name)
    for word in ("AGMV_TIME_AREA", "AGMV_TIME_NEAREST", "AGMV_RATE", "AGMV_ENCODE_RATE_STATS"):
        assert word in hdr
    assert "AGMV_EncodeViewRateDev" in open(os.path.join(H.ROOT, "include", "agmv_writer.h")).read()      # ... which says that it takes no rate


def test_the_time_header_and_its_table_state_each_other():
    """include/agmv_hip_time.h against abi.HIP_TIME: the same names, the header's return and parameter classes, the symbol exported
    and bound, a NULL context refused with its text before any HIP call; disjoint from the other tables"""
    import test_abi as TA
    from libagmv_amd import abi, build, hip
    name = "agmv_hip_time_frames_async"
    protos = TA._prototypes("agmv_hip_time.h")
    assert set(protos) == set(abi.HIP_TIME) == {name}
    assert not set(abi.HIP_TIME) & (set(abi.HIP) | set(abi.HIP_VIEW) | set(abi.HIP_VIEW_SOURCE) | set(abi.HIP_STABILISE) | set(abi.HIP_DEBLOCK))
    restype, argtypes = abi.HIP_TIME[name]
    ret, params = protos[name]
    assert len(params) == 20
    assert TA._ctypes_class(restype) == TA._c_class(ret, True)
    assert [TA._ctypes_class(a) for a in argtypes] == [TA._c_class(p) for p in params]
    build.build()
    G = hip.load_library()
    f = getattr(G, name)
    assert list(f.argtypes) == list(argtypes) and f.restype is C.c_int
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    for fmt in (1, 2, NV12):
        assert f(None, fmt, p, 4, 4, 4, 0, 1, 4, 0, 0, 4, 4, 2, 1, AREA, 0, 2, p, None) < 0 and b"NULL context" in G.agmv_hip_last_error()


def test_the_structures_have_the_headers_layout(tmp_path):
    import subprocess
    from libagmv_amd import abi
    structs = (abi.AGMV_RATE, abi.AGMV_ENCODE_RATE_STATS)
    assert [f[0] for f in abi.AGMV_RATE._fields_] == ["src", "dst", "filter"]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include \"agmv.h\"\nint main(void) {\n" + "".join(
        '    printf("%s %%zu%s\\n", sizeof(%s)%s);\n' % (s.__name__, " %zu" * len(s._fields_), s.__name__, "".join(", offsetof(%s, %s)" % (s.__name__, f[0]) for f in s._fields_))
        for s in structs) + '    printf("%d %d\\n", (int)AGMV_TIME_NEAREST, (int)AGMV_TIME_AREA);\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", str(src), "-I" + os.path.join(H.ROOT, "include"), "-o", exe], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert lines == ["%s %d%s" % (s.__name__, C.sizeof(s), "".join(" %d" % getattr(s, f[0]).offset for f in s._fields_)) for s in structs] + ["1 2"]
    from libagmv_amd import hip
    assert hip.TIME == {"nearest": TC.NEAREST, "area": TC.AREA} and (TC.NEAREST, TC.AREA) == (1, 2)


# ---- refusals: the header's list.  Baseline: 13 frames of 40 x 24 RGB24, the whole clip, 5 : 2 AREA (5 frames come out), no target,
# OPT_III, PDIFS -- which no case leaves as it is: every case below is refused before a device is opened.
def _view(first=0, count=0, step=1, x=0, y=0, width=0, height=0):
    from libagmv_amd import abi
    return abi.AGMV_VIEW(first, count, step, x, y, width, height)


WIN = dict(x=4, y=4, width=16, height=8)
REFUSALS = [
    # -1: the rate
    ("rate-src-0", dict(rate=(0, 2, AREA)), -1),
    ("rate-dst-0", dict(rate=(5, 0, AREA)), -1),
    ("rate-0-0", dict(rate=(0, 0, NEAREST)), -1),
    ("time-filter-0", dict(rate=(5, 2, 0)), -1),
    ("time-filter-3", dict(rate=(5, 2, 3)), -1),
    ("time-filter-0-at-1-1", dict(rate=(2, 2, 0)), -1),
    ("reduced-src-above-65535", dict(rate=(65537, 2, AREA)), -1),
    ("reduced-dst-above-65535", dict(rate=(2, 65537, NEAREST)), -1),
    ("area-raises-the-rate", dict(rate=(2, 5, AREA)), -1),
    ("area-raises-the-rate-by-one", dict(rate=(65534, 65535, AREA)), -1),
    # -1: what AGMV_EncodeViewDev refuses
    ("null-filename", dict(path=None), -1),
    ("null-frames", dict(src=None), -1),
    ("unknown-format", dict(fmt=6), -1),
    ("unknown-yuv-flag", dict(fmt=NV12 | 0x400), -1),
    ("opt-0", dict(opt=0), -1),
    ("quality-4", dict(quality=4), -1),
    ("compression-3", dict(compression=3), -1),
    ("schedule-4", dict(schedule=4), -1),
    ("bilinear-with-a-target", dict(w=16, h=8, filt=BILINEAR), -1),
    ("step-0", dict(view=dict(step=0)), -1),
    ("window-width-0", dict(view=dict(width=0, height=8)), -1),
    ("x-with-a-zero-window", dict(view=dict(x=4)), -1),
    # -5
    ("adaptive-with-a-track", dict(schedule=ADAPTIVE, track=True), -5),
    # -3
    ("source-width-0", dict(sw=0), -3),
    ("source-above-2^28", dict(sw=1 << 15, sh=(1 << 13) + 4), -3),
    ("window-past-the-right-edge", dict(view=dict(x=28, y=0, width=16, height=8)), -3),
    ("nv12-of-odd-width-with-a-window", dict(fmt=NV12, sw=41, view=WIN), -3),
    ("nv12-of-odd-width-consecutive-full-frames", dict(fmt=NV12, sw=41), -3),          # no exception with a rate: nothing is encoded in place
    ("i420-of-odd-height-consecutive-full-frames", dict(fmt=I420, sh=25, view=dict(first=1)), -3),
    ("window-width-no-multiple-of-4", dict(view=dict(x=0, y=0, width=10, height=8)), -3),
    ("target-no-multiple-of-4", dict(w=18, h=8, filt=AREA, view=WIN), -3),
    ("gba-with-a-target", dict(w=8, h=8, filt=NEAREST, opt=5, view=WIN), -3),
    ("area-wider-than-the-window", dict(w=20, h=8, filt=AREA, view=WIN), -3),
    # -2: judged on m
    ("13-frames-at-4-1-give-3", dict(rate=(4, 1, AREA)), -2),
    ("13-frames-at-4-1-nearest-give-3", dict(rate=(4, 1, NEAREST)), -2),
    ("13-frames-at-14-1-give-none", dict(rate=(14, 1, AREA), schedule=FULL), -2),
    ("a-view-of-9-at-5-2-gives-3", dict(view=dict(count=9)), -2),
    ("first-behind-the-end", dict(view=dict(first=13)), -2),
    ("one-frame-with-a-heavy-opt", dict(opt=1, rate=(13, 1, AREA)), -2),
    ("no-frame-with-a-target", dict(w=8, h=8, filt=AREA, view=dict(first=20, **WIN)), -2),
    # the order
    ("rate--1-before--5", dict(rate=(0, 2, AREA), schedule=ADAPTIVE, track=True), -1),
    ("rate--1-before--3", dict(rate=(2, 5, AREA), sw=0), -1),
    ("rate--1-before--2", dict(rate=(5, 2, 9), view=dict(first=13)), -1),
    ("-5-before--3", dict(schedule=ADAPTIVE, track=True, sw=0), -5),
    ("-5-before--2", dict(schedule=ADAPTIVE, track=True, rate=(14, 1, AREA)), -5),
    ("-3-before--2-the-source", dict(sh=0, rate=(14, 1, AREA)), -3),
    ("-3-before--2-the-odd-yuv-frame", dict(fmt=NV12, sh=25, rate=(14, 1, AREA)), -3),
    ("-3-before--2-the-target", dict(w=18, h=8, filt=AREA, view=dict(first=13, **WIN)), -3),
]


def _call(L, a, rate, view):
    if a["track"]:
        assert L.AGMV_SetAudioDev(FAKE, 1, 48000, 48000, 2) == 0
    return L.AGMV_EncodeViewRateDev(a["path"], a["src"], a["fmt"], a["n"], a["sw"], a["sh"], view, rate, a["w"], a["h"], a["filt"], 24, a["opt"], a["quality"],
                                    a["compression"], a["schedule"])


def _stats_are_zero(L):
    from libagmv_amd.abi import AGMV_ENCODE_RATE_STATS, AGMV_ENCODE_VIEW_STATS
    st, vs = AGMV_ENCODE_RATE_STATS(9, 9, 9), AGMV_ENCODE_VIEW_STATS(9, 9, 9)
    L.AGMV_GetEncodeRateStats(C.byref(st))
    L.AGMV_GetEncodeViewStats(C.byref(vs))
    return (st.frames_in, st.frames_out, st.frame_reads, vs.frames, vs.clip_bytes, vs.staging_bytes) == (0,) * 6


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_and_their_order(L, tmp_path, case):
    from libagmv_amd import abi
    _, change, code = case
    out = str(tmp_path / "out.agmv").encode()
    a = dict(dict(path=out, src=FAKE, fmt=RGB24, n=N, sw=SW, sh=SH, view={}, rate=(5, 2, AREA), w=0, h=0, filt=0, opt=3, quality=3, compression=1, schedule=PDIFS,
                  track=False), **change)
    rate, view = abi.AGMV_RATE(*a["rate"]), _view(**a["view"])
    assert _call(L, a, C.byref(rate), C.byref(view)) == code
    if not a["view"]:
        assert _call(L, a, C.byref(rate), None) == code                          # view == NULL is the whole clip
    if a["track"]:
        # the track is consumed whatever the call returns: the same call again, with a source nobody can encode, is no longer -5
        a["track"] = False
        assert L.AGMV_EncodeViewRateDev(out, FAKE, RGB24, N, 0, SH, None, C.byref(rate) if code == -5 else None, 0, 0, 0, 24, 3, 3, 1, ADAPTIVE) == -3
    assert _stats_are_zero(L)
    assert not os.path.exists(out)


def test_no_rate_and_one_to_one_are_refused_where_the_view_call_refuses():
    """rate == NULL and 2 : 2 with the arguments of every refusal tests/test_view_source_cpu.py lists for AGMV_EncodeViewDev: the same
    value, and that call's own value once more"""
    import test_view_source_cpu as TV
    from libagmv_amd import abi
    L = H.lib()
    out = b"/nonexistent-directory/out.agmv"
    assert len(TV.REFUSALS) >= 50
    for name, change, code in TV.REFUSALS:
        a = dict(dict(path=out, src=FAKE, fmt=RGB24, n=N, sw=SW, sh=SH, view={}, w=0, h=0, filt=0, opt=3, quality=3, compression=1, schedule=PDIFS, track=False), **change)
        view = _view(**a["view"])
        for rate in (None, abi.AGMV_RATE(2, 2, AREA), abi.AGMV_RATE(65535, 65535, NEAREST)):
            assert _call(L, a, C.byref(rate) if rate is not None else None, C.byref(view)) == code, name
            assert _stats_are_zero(L), name
        if a["track"]:
            assert L.AGMV_SetAudioDev(FAKE, 1, 48000, 48000, 2) == 0
        assert L.AGMV_EncodeViewDev(a["path"], a["src"], a["fmt"], a["n"], a["sw"], a["sh"], C.byref(view), a["w"], a["h"], a["filt"], 24, a["opt"], a["quality"],
                                    a["compression"], a["schedule"]) == code, name
    # an odd NV12 frame, consecutive full frames: refused by the rate alone (-3); without one it would go on to the device
    assert L.AGMV_EncodeViewRateDev(out, FAKE, NV12, N, 41, SH, None, C.byref(abi.AGMV_RATE(2, 1, AREA)), 0, 0, 0, 24, 3, 3, 1, PDIFS) == -3


# ---- encode_frames(rate=, time=) ----
def _cpu_clip(shape=(N, SH, SW, 3), dtype=None):
    import torch
    return torch.zeros(shape, dtype=dtype or torch.uint8)


BAD_RATES = [5, "5:2", (5,), (5, 2, 1), (5.0, 2), (5, 2.0), (True, 1), (5, None), (0, 1), (1, 0), (-5, 2), {5, 2}]


def test_seq_refuses_bad_rates_before_the_library_is_loaded(monkeypatch, tmp_path):
    import torch
    import libagmv_amd
    from libagmv_amd import seq

    def reached():
        raise AssertionError("the library was called")
    monkeypatch.setattr(seq, "load_library", reached)
    out, clip = str(tmp_path / "out.agmv"), _cpu_clip()
    for rate in BAD_RATES:
        with pytest.raises(ValueError, match="encode_frames: rate"):
            libagmv_amd.encode_frames(out, clip, rate=rate)
    for rate in ((2, 5), (1, 2), (65534, 65535)):
        with pytest.raises(ValueError, match="encode_frames: rate .*area"):
            libagmv_amd.encode_frames(out, clip, rate=rate)
        with pytest.raises(ValueError, match="encode_frames: rate .*area"):
            libagmv_amd.encode_frames(out, clip, rate=rate, time="area")
    for rate, time in (((65537, 2), "area"), ((2, 65537), "nearest"), ((65536, 1), "nearest")):
        with pytest.raises(ValueError, match="encode_frames: rate .*65535"):
            libagmv_amd.encode_frames(out, clip, rate=rate, time=time)
    for time in ("box", "linear", None, 2, b"area"):
        with pytest.raises(ValueError, match="encode_frames: time"):
            libagmv_amd.encode_frames(out, clip, rate=(5, 2), time=time)
    with pytest.raises(ValueError, match="encode_frames: time.*needs rate"):
        libagmv_amd.encode_frames(out, clip, time="nearest")
    model = _cpu_clip((N, 3, SH, SW), torch.float32)
    with pytest.raises(ValueError, match="rate= does not go with a tensor clip"):
        libagmv_amd.encode_frames(out, model, rate=(2, 1))
    # a good value goes on: to the device check, which a host tensor fails, before the library
    for kw in (dict(rate=(5, 2)), dict(rate=[4, 1], time="nearest"), dict(rate=(2, 5), time="nearest"), dict(rate=(131070, 2)), dict(rate=(3, 3)),
               dict(rate=(5, 2), select=range(1, 12, 2), crop=(1, 3, 8, 8)), dict(rate=(2, 1), fit="crop", size=(16, 16))):
        with pytest.raises(ValueError, match="must be on"):
            libagmv_amd.encode_frames(out, clip, **kw)
    assert not os.path.exists(out)


def test_a_writer_takes_no_rate(tmp_path):
    import libagmv_amd
    with pytest.raises(TypeError, match="rate"):
        libagmv_amd.Writer(str(tmp_path / "out.agmv"), 24, 40, rate=(5, 2))
    assert not os.path.exists(tmp_path / "out.agmv")
