"""Reader sessions (include/agmv_reader.h) without a GPU: the arithmetic of the seek index (agmv_reader_checkpoint of agmv_pipeline.h,
exported for this test) against its statement by enumeration, everything AGMV_OpenReaderDev and AGMV_ReaderReadDev refuse -- the
expected code of an open is what AGMV_DecodeViewDev / AGMV_DecodeViewTensorDev return for the same arguments, never a number written
here -- the table abi.READER and the two structures against the header, and the ValueErrors of libagmv_amd.Reader, which come
before the library is loaded."""
import ctypes as C
import os
import subprocess

import pytest

import hostlib as H
import test_abi as TA
from libagmv_amd import abi

u32 = C.c_uint32
FAKE = 4096                                                      # never dereferenced
GOOD = os.path.join(H.ROOT, "tests", "golden", "agmv_splash.agmv")


@pytest.fixture(scope="module")
def L():
    lib = abi.bind(H.lib(), abi.READER)
    return abi.bind(lib, {"agmv_reader_checkpoint": (u32, (u32, C.c_size_t, C.c_size_t, u32, C.POINTER(u32), C.POINTER(u32)))})


# ---- the seek index
def interval_of(nframes, lz_cap, budget):
    """the header's statement: the smallest multiple of 4 with ceil(nframes / interval) * lz_cap <= budget; below one lz_cap, checkpoint 0 alone"""
    if budget < lz_cap:
        return max(4, (nframes + 3) // 4 * 4)
    iv = 4
    while -(-max(nframes, 1) // iv) * lz_cap > budget:
        iv += 4
    return iv


def start_of(f, interval, recorded):
    """the greatest recorded checkpoint <= f & ~3; `recorded`: the set of checkpoint numbers, 0 always in it"""
    return max(k for k in recorded | {0} if k * interval <= (f & ~3)) * interval


def test_interval_is_the_smallest_that_fits_the_budget(L):
    lz_cap = 64 * 48 * 33 // 16 + 4096
    iv = u32()
    for nframes in range(1, 41):
        for budget in (1, lz_cap - 1, lz_cap, lz_cap + 1, 2 * lz_cap, 3 * lz_cap - 1, 3 * lz_cap, 5 * lz_cap, 10 * lz_cap, 10 * lz_cap + 7, 40 * lz_cap, 1 << 40):
            L.agmv_reader_checkpoint(nframes, lz_cap, budget, 0, None, C.byref(iv))
            assert iv.value == interval_of(nframes, lz_cap, budget), (nframes, budget)
            assert iv.value % 4 == 0 and iv.value >= 4
            if budget >= lz_cap:
                assert -(-nframes // iv.value) * lz_cap <= budget
    L.agmv_reader_checkpoint(256, 1920 * 1080 * 33 // 16 + 4096, 64 << 20, 0, None, C.byref(iv))
    assert iv.value == interval_of(256, 1920 * 1080 * 33 // 16 + 4096, 64 << 20) == 20
    L.agmv_reader_checkpoint(0xFFFFFFFF, 1 << 20, 1 << 20, 0, None, C.byref(iv))
    assert iv.value == 0xFFFFFFFC


def test_the_checkpoint_a_seek_starts_from_is_the_enumeration(L):
    """24 frames at interval 4: every set of recorded checkpoints 1 .. 5 (checkpoint 0 always exists, its bit set or not) and every frame"""
    lz_cap, nframes = 1000, 24
    budget = 6 * lz_cap
    iv = u32()
    for bits in range(64):
        word = (u32 * 1)(bits)
        recorded = {k for k in range(6) if bits >> k & 1}
        for f in list(range(0, 30)) + [1000, 0xFFFFFFFF]:
            got = L.agmv_reader_checkpoint(nframes, lz_cap, budget, f, word, C.byref(iv))
            assert iv.value == 4
            assert got == start_of(min(f, nframes - 1), 4, recorded), (bits, f, got)     # (a frame behind the file: as its last frame)
    for f in range(24):                                          # no bitmap: checkpoint 0
        assert L.agmv_reader_checkpoint(nframes, lz_cap, budget, f, None, None) == 0
    word = (u32 * 2)(0, 1 << 3)                                  # checkpoint 35 of a long file, in the second word
    assert L.agmv_reader_checkpoint(400, lz_cap, 100 * lz_cap, 35 * 4 + 2, word, C.byref(iv)) == 35 * 4 and iv.value == 4
    assert L.agmv_reader_checkpoint(400, lz_cap, 100 * lz_cap, 35 * 4 - 1, word, None) == 0


# ---- the refusals of an open: the view decoders' own, in their order
def desc(**kw):
    d = abi.AGMV_READER_DESC(fmt=2, step=1, mean=(C.c_float * 3)(0, 0, 0), std=(C.c_float * 3)(1, 1, 1), type=1)
    for k, v in kw.items():
        setattr(d, k, (C.c_float * 3)(*v) if k in ("mean", "std") else v)
    return d


def files(tmp):
    data = open(GOOD, "rb").read()
    w = int.from_bytes(data[8:12], "little")
    le = lambda v: v.to_bytes(4, "little")
    made = {"badfourcc": b"AGMX" + data[4:], "w6": data[:8] + le(6) + data[12:], "odd": data[:8] + le(w - 1) + data[12:],
            "huge": data[:8] + le(8192) + le(4096) + data[16:]}
    paths = {None: None, "good": GOOD.encode(), "missing": os.path.join(tmp, "missing.agmv").encode()}
    for name, content in made.items():
        paths[name] = os.path.join(tmp, name + ".agmv").encode()
        open(paths[name], "wb").write(content)
    return paths


# (class of the code, file, changes to the description).  Singles, then every pair from two different classes that do not touch the same field.
BAD = ([("-1", None, {}), ("-1", "good", dict(fmt=0)), ("-1", "good", dict(fmt=6)), ("-1", "good", dict(fmt=2, yuv_flags=0x100)),
        ("-1", "good", dict(fmt=16, yuv_flags=0x400)), ("-1", "good", dict(win_width=8)), ("-1", "good", dict(win_height=8)), ("-1", "good", dict(x=4)),
        ("-1", "good", dict(y=4)), ("-1", "good", dict(width=16, height=16, filter=0)), ("-1", "good", dict(width=16, height=16, filter=4)),
        ("-1t", "good", dict(tensor=1, type=0)), ("-1t", "good", dict(tensor=1, type=4)), ("-1t", "good", dict(tensor=1, std=(1.0, 0.0, 1.0))),
        ("-1t", "good", dict(tensor=1, mean=(0.0, 2.0 ** 33, 0.0))),
        ("-4", "good", dict(width=0, height=16, filter=1)), ("-4", "good", dict(width=16, height=0, filter=1)), ("-4", "good", dict(width=(1 << 28) + 4, height=1, filter=1)),
        ("-4", "good", dict(width=1 << 15, height=1 << 14, filter=3)),
        ("-Error", "missing", {}), ("-Error", "badfourcc", {}), ("-Error", "w6", {}),
        ("-4 of the file", "good", dict(x=0, y=0, win_width=100000, win_height=8)), ("-4 of the file", "good", dict(x=100000, y=0, win_width=8, win_height=8)),
        ("-4 of the file", "good", dict(width=4096, height=16, filter=2)), ("-4 of the file", "huge", dict(width=16, height=16, filter=2)),
        ("-4 of the file", "odd", dict(fmt=16)), ("-4 of the file", "odd", dict(fmt=17, yuv_flags=0x300)),
        ("-4 of the file", "good", dict(fmt=16, x=0, y=0, win_width=7, win_height=8))])


def cases():
    for k, f, c in BAD:
        yield f, c
    for a in range(len(BAD)):
        for b in range(a + 1, len(BAD)):
            (ka, fa, ca), (kb, fb, cb) = BAD[a], BAD[b]
            if ka != kb and not set(ca) & set(cb) and (fa == "good" or fb == "good" or fa == fb):
                yield (fb if fa == "good" else fa), dict(ca, **cb)


def view_call(L, path, d):
    """what the one-shot view decoder returns for the arguments of a description, with a destination that is never written"""
    v = abi.AGMV_VIEW(0, 0, d.step or 1, d.x, d.y, d.win_width, d.win_height)
    if d.tensor:
        return L.AGMV_DecodeViewTensorDev(path, FAKE, d.type, d.mean, d.std, d.width, d.height, d.filter, C.byref(v), 4, None)
    return L.AGMV_DecodeViewDev(path, FAKE, d.fmt | d.yuv_flags, d.width, d.height, d.filter, C.byref(v), 4, None)


def test_an_open_refuses_what_the_view_decoders_refuse_with_their_codes(L, tmp_path):
    paths = files(str(tmp_path))
    seen = set()
    count = 0
    for f, changes in cases():
        d = desc(**changes)
        want = view_call(L, paths[f], d)
        assert want < 0, (f, changes, want)                      # (every case is refused before a device is opened)
        err, info = C.c_int(77), abi.AGMV_INFO()
        r = L.AGMV_OpenReaderDev(paths[f], C.byref(d), C.byref(info), C.byref(err))
        assert r is None and err.value == want, (f, changes, err.value, want)
        assert L.AGMV_OpenReaderDev(paths[f], C.byref(d), None, None) is None
        seen.add(want)
        count += 1
    assert {-1, -4} < seen and count > 200, (seen, count)            # (the third: the Error of a file that cannot be read)
    err = C.c_int(77)                                            # no description at all
    assert L.AGMV_OpenReaderDev(paths["good"], None, None, C.byref(err)) is None and err.value == -1


def test_a_refused_open_fills_the_info_where_the_header_was_read(L, tmp_path):
    info, err = abi.AGMV_INFO(), C.c_int(0)
    d = desc(x=100000, y=0, win_width=8, win_height=8)
    assert L.AGMV_OpenReaderDev(GOOD.encode(), C.byref(d), C.byref(info), C.byref(err)) is None and err.value == -4
    assert info.number_of_frames > 1 and info.width > 0


def test_calls_on_no_reader_and_reads_of_nothing(L):
    st = abi.AGMV_READER_STATS(1, 2, 3, 4, 5, 6, 7, 8)
    assert L.AGMV_ReaderReadDev(None, FAKE, 4) == -1 and L.AGMV_ReaderReadDev(None, None, 0) == -1
    assert L.AGMV_ReaderSeek(None, 3) == -1 and L.AGMV_ReaderTell(None) == 0
    L.AGMV_GetReaderStats(None, C.byref(st))
    assert [getattr(st, k) for k, _ in st._fields_] == [0] * 8
    L.AGMV_GetReaderStats(None, None)
    L.AGMV_CloseReader(None)


# ---- the table and the structures against the header
def test_the_reader_header_and_its_table_state_each_other(L):
    protos = TA._prototypes("agmv_reader.h")
    assert set(protos) == set(abi.READER) and len(protos) == 6
    for name, (restype, argtypes) in abi.READER.items():
        ret, params = protos[name]
        assert TA._ctypes_class(restype) == TA._c_class(ret, True), name
        assert [TA._ctypes_class(a) for a in argtypes] == [TA._c_class(p) for p in params], name
        f = getattr(L, name)
        assert list(f.argtypes) == list(argtypes) and f.restype is restype


def test_the_two_structures_have_the_headers_layout(tmp_path):
    structs = (abi.AGMV_READER_DESC, abi.AGMV_READER_STATS)
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"agmv_reader.h\"\nint main(void) {\n" + "".join(
        '    printf("%s %%zu%s\\n", sizeof(%s)%s);\n' % (s.__name__, " %zu" * len(s._fields_), s.__name__,
                                                     "".join(", offsetof(%s, %s)" % (s.__name__, f[0]) for f in s._fields_))
        for s in structs) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", str(src), "-I" + os.path.join(H.ROOT, "include"), "-o", exe], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert lines == ["%s %d%s" % (s.__name__, C.sizeof(s), "".join(" %d" % getattr(s, f[0]).offset for f in s._fields_)) for s in structs]


# ---- libagmv_amd.Reader
def test_reader_refuses_bad_arguments_before_the_library_is_loaded(monkeypatch):
    import libagmv_amd
    from libagmv_amd import seq

    def reached():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(seq, "load_library", reached)
    for kw, word in ((dict(step=0), "step"), (dict(step=True), "step"), (dict(step=1.5), "step"), (dict(index_bytes=0), "index_bytes"),
                     (dict(index_bytes="1M"), "index_bytes"), (dict(crop=(0, 0, 0, 8)), "crop"), (dict(crop=(0, 0, 8)), "crop"),
                     (dict(scale="cubic"), "scale"), (dict(scale="area"), "size"), (dict(size=(0, 4)), "size"), (dict(fmt="rgb24", yuv="bt709"), "yuv"),
                     (dict(fmt="f16", full_range=True), "full_range"), (dict(fmt="rgb24", mean=0.5), "mean"), (dict(fmt="xyz"), "xyz"),
                     (dict(deblock=0), "deblock"), (dict(deblock=65), "deblock")):
        with pytest.raises(ValueError, match=word):
            libagmv_amd.Reader("nowhere.agmv", **kw)


def test_reader_turns_a_refused_open_into_an_error_and_opens_no_device():
    """a normalisation and a window that only the library refuses (-1, -4): ValueError; a file that is not there: RuntimeError"""
    import libagmv_amd
    with pytest.raises(ValueError, match="refused"):
        libagmv_amd.Reader(GOOD, fmt="f32", std=(1, 0, 1))
    with pytest.raises(ValueError, match="window"):
        libagmv_amd.Reader(GOOD, crop=(0, 0, 8, 100000))
    with pytest.raises(RuntimeError, match="Error"):
        libagmv_amd.Reader(os.path.join(H.ROOT, "tests", "golden", "no_such_file.agmv"))
