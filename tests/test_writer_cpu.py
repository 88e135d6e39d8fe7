"""Writer sessions (include/agmv_writer.h) without a GPU: the PDIFS decision function (agmv_writer_groups of agmv_pipeline.h, exported
for this test) against an enumeration of encode_sequence's loop, everything AGMV_OpenWriterDev refuses -- the expected code is what
AGMV_EncodeFramesFmtDev / AGMV_EncodeFramesScaledDev / AGMV_EncodeFramesTensorDev return for the same arguments, never a number
written here -- the calls on no writer, the table abi.WRITER and the two structures against the header, and the ValueErrors of
libagmv_amd.Writer, which come before the library is loaded.  What needs an open writer (a write before any analyse, an analyse
after a write) needs a device and stands in tests/test_gpu_writer_files.py."""
import ctypes as C
import os
import subprocess

import pytest

import hostlib as H
import test_abi as TA
from libagmv_amd import abi

u32 = C.c_uint32
FAKE = 4096                                                      # never dereferenced
FULL, PDIFS, ADAPTIVE = 1, 2, 3


@pytest.fixture(scope="module")
def L():
    lib = abi.bind(H.lib(), abi.WRITER)
    return abi.bind(lib, {"agmv_writer_groups": (u32, (u32, C.c_int, C.c_int))})


# ---- the PDIFS schedule without the clip's end
def groups_of_the_loop(n, heavy):
    """encode_sequence's loop over the frames 1 .. n, as it stands there: the sources of the groups it pushes"""
    start_frame, end_frame, out = 1, n, []
    i = start_frame
    while i <= end_frame:
        if not heavy:
            out.append((i, i + 1, i + 2, i + 3))
            i += 4
        else:
            out.append((i, i + 1))
            i += 2
        if i + 4 >= end_frame:
            break
    return out


def test_the_groups_decided_are_those_of_the_one_shot_loop(L):
    for heavy in (0, 1):
        first = 2 if heavy else 4
        for n in range(0, 70):
            loop = groups_of_the_loop(n, heavy) if n >= first else []       # (fewer frames than the first group reads are refused, -2)
            for closed in (0, 1):
                assert L.agmv_writer_groups(n, heavy, closed) == len(loop), (n, heavy, closed)
            assert all(src <= n for g in loop for src in g), (n, heavy)      # the loop reads no frame behind the clip
            # a group starting at 0-based frame j behind the first is there exactly when frame j + 5 exists
            assert [g[0] - 1 for g in loop[1:]] == [j for j in range(first, n, first) if j + 5 < n], (n, heavy)
    # decided groups never go away when frames arrive: what is emitted early is what the one-shot call emits
    for heavy in (0, 1):
        counts = [L.agmv_writer_groups(n, heavy, 0) for n in range(0, 200)]
        assert counts == sorted(counts)


# ---- the refusals of an open: the one-shot calls' own, in their order
def desc(**kw):
    d = abi.AGMV_WRITER_DESC(fmt=2, src_width=64, src_height=48, frames_per_second=24, opt=3, quality=3, compression=1, schedule=FULL,
                             mean=(C.c_float * 3)(0, 0, 0), std=(C.c_float * 3)(1, 1, 1), type=2)
    for k, v in kw.items():
        setattr(d, k, (C.c_float * 3)(*v) if k in ("mean", "std") else v)
    return d


def one_shot(L, path, d, n=8):
    """what the one-shot call of the description's layout returns for its arguments, with a clip that is never read"""
    tail = (d.frames_per_second, d.opt, d.quality, d.compression, d.schedule)
    if d.tensor:
        return L.AGMV_EncodeFramesTensorDev(path, FAKE, d.type, d.mean, d.std, n, d.src_width, d.src_height, *tail)
    if d.width or d.height:
        return L.AGMV_EncodeFramesScaledDev(path, FAKE, d.fmt | d.yuv_flags, n, d.src_width, d.src_height, d.width, d.height, d.filter, *tail)
    return L.AGMV_EncodeFramesFmtDev(path, FAKE, d.fmt | d.yuv_flags, n, d.src_width, d.src_height, *tail)


# (class of the code, has a file name, changes to the description).  Singles, then every pair from two different classes that do not touch the same field.
BAD = ([("-1", False, {}), ("-1", True, dict(fmt=0)), ("-1", True, dict(fmt=6)), ("-1", True, dict(fmt=2, yuv_flags=0x100)), ("-1", True, dict(fmt=16, yuv_flags=0x400)),
        ("-1", True, dict(opt=0)), ("-1", True, dict(opt=9)), ("-1", True, dict(quality=0)), ("-1", True, dict(quality=4)), ("-1", True, dict(compression=0)),
        ("-1", True, dict(compression=3)), ("-1", True, dict(schedule=0)), ("-1", True, dict(schedule=7)),
        ("-1s", True, dict(width=32, height=24, filter=0)), ("-1s", True, dict(width=32, height=24, filter=3)),
        ("-1t", True, dict(tensor=1, type=0)), ("-1t", True, dict(tensor=1, type=4)), ("-1t", True, dict(tensor=1, std=(1.0, 0.0, 1.0))),
        ("-1t", True, dict(tensor=1, mean=(0.0, 2.0 ** 33, 0.0))),
        ("-3", True, dict(src_width=0)), ("-3", True, dict(src_height=0)), ("-3", True, dict(src_width=66)), ("-3", True, dict(src_height=50)),
        ("-3", True, dict(src_width=1 << 15, src_height=1 << 14)), ("-3", True, dict(opt=5, src_width=1)),
        ("-3s", True, dict(width=30, height=24, filter=2)), ("-3s", True, dict(width=32, height=0, filter=1)), ("-3s", True, dict(width=128, height=24, filter=2)),
        ("-3s", True, dict(width=32, height=24, filter=1, opt=6)), ("-3s", True, dict(width=32, height=24, filter=2, src_width=0))])


def cases():
    for k, f, c in BAD:
        yield f, c
    for a in range(len(BAD)):
        for b in range(a + 1, len(BAD)):
            (ka, fa, ca), (kb, fb, cb) = BAD[a], BAD[b]
            if ka[:2] != kb[:2] and not set(ca) & set(cb):
                yield fa and fb, dict(ca, **cb)


def test_an_open_refuses_what_the_one_shot_calls_refuse_with_their_codes(L, tmp_path):
    path = str(tmp_path / "never.agmv").encode()
    seen, count = set(), 0
    for named, changes in cases():
        d = desc(**changes)
        want = one_shot(L, path if named else None, d)
        assert want < 0, (named, changes, want)                  # (every case is refused before a device is opened)
        err = C.c_int(77)
        assert L.AGMV_OpenWriterDev(path if named else None, C.byref(d), C.byref(err)) is None and err.value == want, (named, changes, err.value, want)
        assert L.AGMV_OpenWriterDev(path if named else None, C.byref(d), None) is None
        seen.add(want)
        count += 1
    assert seen == {-1, -3} and count > 200, (seen, count)
    assert not os.path.exists(path)                              # no refused open creates the file
    err = C.c_int(77)                                            # no description at all: the code of a NULL argument
    assert L.AGMV_OpenWriterDev(path, None, C.byref(err)) is None and err.value == one_shot(L, None, desc())


def test_an_open_refuses_the_adaptive_schedule_as_an_unknown_enum_and_a_tensor_with_a_target(L, tmp_path):
    path = str(tmp_path / "never.agmv").encode()
    err = C.c_int(77)
    for changes in ({}, dict(tensor=1), dict(width=32, height=24, filter=2), dict(schedule=ADAPTIVE, src_width=66)):
        d = desc(**dict(dict(schedule=ADAPTIVE), **changes))
        assert one_shot(L, path, desc(**dict(changes, schedule=7))) == -1
        assert L.AGMV_OpenWriterDev(path, C.byref(d), C.byref(err)) is None and err.value == one_shot(L, path, desc(**dict(changes, schedule=7)))
    # a tensor writer takes no target size: the code of a refused geometry
    d = desc(tensor=1, width=32, height=24, filter=2)
    assert L.AGMV_OpenWriterDev(path, C.byref(d), C.byref(err)) is None and err.value == one_shot(L, path, desc(src_width=66)) == -3
    assert L.AGMV_OpenWriterDev(path, C.byref(desc(tensor=1, type=0, width=32, height=24, filter=2)), C.byref(err)) is None and err.value == -1      # ... behind the tensor's own checks
    assert not os.path.exists(path)


def test_the_count_checks_wait_for_the_close(L, tmp_path):
    """a frame count the one-shot call refuses (-2) is no reason to refuse an open, which does not know it: with everything else good the open
    goes on to the device, which this test must not reach -- so the claim is held on descriptions that are refused for another reason"""
    path = str(tmp_path / "never.agmv").encode()
    d = desc(schedule=PDIFS, src_width=66)
    assert one_shot(L, path, desc(schedule=PDIFS), n=3) == -2 and one_shot(L, path, d, n=3) == -2       # the one-shot call: the count first
    err = C.c_int(77)
    assert L.AGMV_OpenWriterDev(path, C.byref(d), C.byref(err)) is None and err.value == one_shot(L, path, d, n=8) == -3


def test_calls_on_no_writer_and_calls_of_nothing(L):
    st = abi.AGMV_WRITER_STATS(1, 2, 3, 4, 5, 6, 7)
    written = C.c_ulong(77)
    assert L.AGMV_WriterAnalyseDev(None, FAKE, 4) == -1 and L.AGMV_WriterAnalyseDev(None, None, 0) == -1
    assert L.AGMV_WriterWriteDev(None, FAKE, 4) == -1 and L.AGMV_WriterWriteDev(None, None, 0) == -1
    assert L.AGMV_CloseWriter(None, C.byref(written)) == 0 and written.value == 77 and L.AGMV_CloseWriter(None, None) == 0
    L.AGMV_GetWriterStats(None, C.byref(st))
    assert [getattr(st, k) for k, _ in st._fields_] == [0] * 7
    L.AGMV_GetWriterStats(None, None)


# ---- the table and the structures against the header
def test_the_writer_header_and_its_table_state_each_other(L):
    protos = TA._prototypes("agmv_writer.h")
    assert set(protos) == set(abi.WRITER) and len(protos) == 5
    for name, (restype, argtypes) in abi.WRITER.items():
        ret, params = protos[name]
        assert TA._ctypes_class(restype) == TA._c_class(ret, True), name
        assert [TA._ctypes_class(a) for a in argtypes] == [TA._c_class(p) for p in params], name
        f = getattr(L, name)
        assert list(f.argtypes) == list(argtypes) and f.restype is restype


def test_the_two_structures_have_the_headers_layout(tmp_path):
    structs = (abi.AGMV_WRITER_DESC, abi.AGMV_WRITER_STATS)
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"agmv_writer.h\"\nint main(void) {\n" + "".join(
        '    printf("%s %%zu%s\\n", sizeof(%s)%s);\n' % (s.__name__, " %zu" * len(s._fields_), s.__name__,
                                                     "".join(", offsetof(%s, %s)" % (s.__name__, f[0]) for f in s._fields_))
        for s in structs) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", str(src), "-I" + os.path.join(H.ROOT, "include"), "-o", exe], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert lines == ["%s %d%s" % (s.__name__, C.sizeof(s), "".join(" %d" % getattr(s, f[0]).offset for f in s._fields_)) for s in structs]


# ---- libagmv_amd.Writer
def test_writer_refuses_bad_arguments_before_the_library_is_loaded(monkeypatch):
    import libagmv_amd
    from libagmv_amd import seq

    def reached():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(seq, "load_library", reached)
    for kw, word in ((dict(height=0), "height"), (dict(width=True), "width"), (dict(width=64.0), "width"), (dict(ring_frames=0), "ring_frames"),
                     (dict(ring_frames="8"), "ring_frames"), (dict(schedule=seq.SCHEDULE_ADAPTIVE), "schedule"), (dict(schedule=0), "schedule"),
                     (dict(palette_refine=0), "palette_refine"), (dict(dither=65), "dither"), (dict(stabilise=True), "stabilise"),
                     (dict(scale="cubic"), "scale"), (dict(scale="nearest"), "size"), (dict(size=(0, 4)), "size"), (dict(fmt="rgb24", yuv="bt709"), "yuv"),
                     (dict(fmt="f16", full_range=True), "full_range"), (dict(fmt="f16", size=(24, 32)), "size"), (dict(fmt="rgb24", mean=0.5), "mean"),
                     (dict(fmt="xyz"), "xyz")):
        args = dict(dict(height=48, width=64), **kw)
        with pytest.raises(ValueError, match=word):
            libagmv_amd.Writer("nowhere.agmv", **args)
    assert not os.path.exists("nowhere.agmv")


def test_writer_turns_a_refused_open_into_an_error_and_opens_no_device(tmp_path):
    """a geometry and an opt that only the library refuses: ValueError with the code, and no file"""
    import libagmv_amd
    path = str(tmp_path / "never.agmv")
    with pytest.raises(ValueError, match=r"refused its arguments \(-3\)"):
        libagmv_amd.Writer(path, 50, 64)
    with pytest.raises(ValueError, match=r"refused its arguments \(-1\)"):
        libagmv_amd.Writer(path, 48, 64, opt=9)
    with pytest.raises(ValueError, match=r"refused its arguments \(-3\)"):
        libagmv_amd.Writer(path, 48, 64, size=(24, 128))
    assert not os.path.exists(path)
