"""The deblocking before any GPU is touched: the numpy statement (tests/deblock_cases.py) pinned to lines computed by hand and to
the properties include/agmv.h lists as consequences of the rule; the crafted lines on both sides of either threshold; the cell-wise
evaluation the kernel uses against the two-stage one; include/agmv_hip_deblock.h against abi.HIP_DEBLOCK the way
tests/test_stabilise_cpu.py holds the stabilisation's header; the layout of AGMV_DEBLOCK_STATS from gcc; and the ValueErrors of
decode_frames(deblock=) and file_quality(deblock=), which come before the library is loaded."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deblock_cases as K
import hostlib as H


def line(p1, p0, q0, q1, s):
    """four RGB triples -> (the four triples of the result as lists, "none" | "weak" | "strong")"""
    o = K.filter_lines(*[np.array(v, np.int64) for v in (p1, p0, q0, q1)], s)
    return [o[i].tolist() for i in range(4)], "strong" if o[5] else "weak" if o[4] else "none"


def test_a_weak_line_by_hand():
    # side = 10 > 16 >> 2, step = 8: p0' = (90 + 200 + 108 + 2) >> 2 = 100, q0' = (100 + 216 + 120 + 2) >> 2 = 109 (438 >> 2)
    got, kind = line((90, 90, 90), (100, 100, 100), (108, 108, 108), (120, 120, 120), 16)
    assert kind == "weak" and got == [[90] * 3, [100] * 3, [109] * 3, [120] * 3]
    # per channel: R as above, G with the step the other way, B without a step
    got, kind = line((90, 50, 7), (100, 40, 7), (108, 32, 7), (120, 20, 7), 16)
    assert kind == "weak" and got == [[90, 50, 7], [100, (50 + 80 + 32 + 2) >> 2, 7], [109, (40 + 64 + 20 + 2) >> 2, 7], [120, 20, 7]]


def test_a_strong_line_by_hand():
    # a = 201, b = 217: (1407 + 217 + 8) >> 4 = 102, (5 * 201 + 3 * 217 + 8) >> 4 = 104, (603 + 1085 + 8) >> 4 = 106, (201 + 1519 + 8) >> 4 = 108
    got, kind = line((100, 0, 255), (101, 0, 255), (108, 0, 255), (109, 0, 255), 16)
    assert kind == "strong" and got == [[102, 0, 255], [104, 0, 255], [106, 0, 255], [108, 0, 255]]


@pytest.mark.parametrize("a,b", [(0, 1), (0, 64), (255, 191), (96, 104), (104, 96), (7, 8)])
def test_two_flat_blocks_become_the_ramp(a, b):
    got, kind = line((a,) * 3, (a,) * 3, (b,) * 3, (b,) * 3, 64)
    assert kind == "strong"
    assert [g[0] for g in got] == [(7 * a + b + 4) >> 3, (5 * a + 3 * b + 4) >> 3, (3 * a + 5 * b + 4) >> 3, (a + 7 * b + 4) >> 3]
    clip = K.flat_blocks(a, b)
    out, weak, strong = K.deblock(clip, 64)
    assert weak == 0 and strong == 16                           # 8 rows across x = 4, 8 columns across y = 4
    row = K.channels(out)[0, 0, :, 0].tolist()                   # row 0 lies outside every stage-2 line
    assert row == [a, a, (7 * a + b + 4) >> 3, (5 * a + 3 * b + 4) >> 3, (3 * a + 5 * b + 4) >> 3, (a + 7 * b + 4) >> 3, b, b]


@pytest.mark.parametrize("s", K.STRENGTHS)
def test_the_crafted_lines_fall_on_the_side_of_the_threshold_they_name(s):
    kinds = set()
    for name, ln, want in K.crafted_lines(s):
        got, kind = line(ln[0], ln[1], ln[2], ln[3], s)
        assert kind == want, (s, name, kind)
        assert np.min(got) >= 0 and np.max(got) <= 255, (s, name)
        if want == "none":
            assert got == ln.tolist(), (s, name)
        if want == "weak":
            assert got[0] == ln[0].tolist() and got[3] == ln[3].tolist(), (s, name)
        kinds.add(want)
    assert kinds == {"none", "weak", "strong"}


@pytest.mark.parametrize("s", K.STRENGTHS)
def test_the_thresholds(s):
    g = (100,) * 3
    assert line(g, g, (100 + s,) * 3, (100 + s,) * 3, s)[1] == "strong"                  # step == s filters
    assert line(g, g, (101 + s,) * 3, (101 + s,) * 3, s)[1] == "none"                    # step == s + 1 does not
    assert line((3,) * 3, g, g, (250,) * 3, s)[1] == "none"                              # step == 0 does not
    q = s >> 2
    assert line((100 - q,) * 3, g, (101,) * 3, (101,) * 3, s)[1] == "strong"             # side == s >> 2 is strong
    assert line((99 - q,) * 3, g, (101,) * 3, (101,) * 3, s)[1] == "weak"                # one more is weak
    assert line(g, g, (101, 101 + s, 101), (101, 101 + s, 101), s)[1] == "none"          # one channel alone over the limit vetoes the line


def test_the_ends_of_the_range_stay_in_range():
    for s in K.STRENGTHS:
        for p1 in (0, 255):
            for p0 in (0, 255):
                for q0 in (0, 1, 254, 255):
                    for q1 in (0, 255):
                        got, _ = line((p1,) * 3, (p0,) * 3, (q0,) * 3, (q1,) * 3, s)
                        assert 0 <= np.min(got) and np.max(got) <= 255
    rng = np.random.default_rng(3)
    clip = rng.integers(0, 2 ** 32, (3, 16, 24), dtype=np.uint64).astype(np.uint32)
    clip[0] &= np.uint32(0xFF0101FF)
    K.deblock(clip, 64)                                          # (asserts the range itself)


@pytest.mark.parametrize("s", K.STRENGTHS)
def test_the_top_byte_is_kept(s):
    clip = K.staircase_clip(2, 12, 20, 10 + s)
    out, weak, strong = K.deblock(clip, s)
    assert ((out ^ clip) & np.uint32(0xFF000000) == 0).all()
    assert len(np.unique(clip >> 24)) > 100                      # premise: the top bytes are busy
    assert (K.deblock(clip & np.uint32(0xFFFFFF), s)[0] == out & np.uint32(0xFFFFFF)).all()       # ... and decide nothing


@pytest.mark.parametrize("s", K.STRENGTHS)
def test_a_uniform_clip_and_a_4x4_clip_are_identities_with_zero_counts(s):
    uniform = np.full((3, 12, 20), 0xAB4D4D4D, np.uint32)
    for clip in (uniform, K.staircase_clip(3, 4, 4, s), np.random.default_rng(s).integers(0, 2 ** 32, (2, 4, 4), dtype=np.uint64).astype(np.uint32)):
        for f in (K.deblock, K.deblock_cells):
            out, weak, strong = f(clip, s)
            assert (out == clip).all() and weak == 0 and strong == 0


def test_a_clip_without_a_step_across_a_block_edge_comes_back_unchanged():
    """busy inside the blocks, equal across every edge: columns 3 | 4 and rows 3 | 4 of each pair are the same pixel"""
    rng = np.random.default_rng(9)
    c = rng.integers(0, 256, (2, 16, 16, 3)).astype(np.int64)
    for e in (4, 8, 12):
        c[:, :, e] = c[:, :, e - 1]
    for e in (4, 8, 12):
        c[:, e] = c[:, e - 1]
    clip = K.pack(c)
    out, weak, strong = K.deblock(clip, 64)
    assert (out == clip).all() and weak == 0 and strong == 0


SHAPES = [(1, 4, 4), (2, 4, 8), (2, 8, 4), (2, 8, 8), (2, 20, 12), (1, 8, 260), (3, 12, 20)]


@pytest.mark.parametrize("s", K.STRENGTHS)
def test_the_cell_wise_evaluation_equals_the_two_stages(s):
    for n, h, w in SHAPES:
        for clip in (K.staircase_clip(n, h, w, 100 + s), K.staircase_clip(n, h, w, 200 + s, levels=4, noise=9)):
            a, b = K.deblock(clip, s), K.deblock_cells(clip, s)
            assert (a[0] == b[0]).all() and a[1:] == b[1:], (s, n, h, w)
    a, b = K.deblock(K.crafted_clip(s), s), K.deblock_cells(K.crafted_clip(s), s)
    assert (a[0] == b[0]).all() and a[1:] == b[1:] and a[1] and a[2]            # (weak and strong lines both occur at every strength)


def test_a_cell_depends_on_its_own_pixels_alone():
    rng = np.random.default_rng(5)
    x = K.pack(rng.integers(100, 110, (1, 12, 12, 3)))
    y = K.pack(rng.integers(100, 110, (1, 12, 12, 3)))
    y[:, 2:6, 2:6] = x[:, 2:6, 2:6]
    y[:, 0:2, 10:12] = x[:, 0:2, 10:12]                          # a corner cell
    y[:, 6:10, 0:2] = x[:, 6:10, 0:2]                            # a rim cell
    a, b = K.deblock(x, 16)[0], K.deblock(y, 16)[0]
    assert (a != x).any()
    for ys, xs in ((slice(2, 6), slice(2, 6)), (slice(0, 2), slice(10, 12)), (slice(6, 10), slice(0, 2))):
        assert (a[:, ys, xs] == b[:, ys, xs]).all()
    assert (a[:, 0:2, 10:12] == x[:, 0:2, 10:12]).all()          # the four corner cells are copies


def test_the_counters_by_hand():
    """8 x 12, one frame: columns 0 .. 3 grey 100, columns 4 .. 7 grey 104, and in rows 4 .. 11 column 5 is 120: at s = 16 the edge
    x = 4 has 4 strong lines (rows 0 .. 3, sides 0) and 8 weak ones (side 16 > 4); stage 2 then meets rows 3 | 4, which differ in the
    columns stage 1 changed differently"""
    c = np.full((1, 12, 8, 3), 100, np.int64)
    c[:, :, 4:] = 104
    c[:, 4:, 5] = 120
    clip = K.pack(c)
    t, w1, s1 = K.stage(K.channels(clip), 16)
    assert (w1, s1) == (8, 4)
    out, weak, strong = K.deblock(clip, 16)
    _, w2, s2 = K.stage(np.ascontiguousarray(t.transpose(0, 2, 1, 3)), 16)
    assert (weak, strong) == (8 + w2, 4 + s2) and w2 + s2 > 0
    assert K.lines_examined(1, 12, 8) == 1 * 12 + 2 * 8 and K.lines_examined(3, 4, 4) == 0
    assert weak + strong <= K.lines_examined(1, 12, 8)


def test_the_statement_gives_the_issues_figures():
    """the numpy experiment that motivated the knob: a 64 x 48 gradient of flat blocks 8 levels apart, 36.5 dB -> 46.4 dB at
    strength 16 and unchanged at strength 4"""
    h, w = 48, 64
    yy, xx = np.mgrid[0:h, 0:w]
    src = np.stack([xx * 3 + yy, 255 - xx * 2 - yy, xx + yy * 3], -1)[None].clip(0, 255)
    blk = src.reshape(1, h // 4, 4, w // 4, 4, 3).mean((2, 4)).round().astype(np.int64) // 8 * 8 + 4
    dec = np.repeat(np.repeat(blk, 4, 1), 4, 2)
    psnr = lambda a: 10 * np.log10(255 ** 2 / np.mean((a.astype(float) - src) ** 2))
    o16, o4 = K.deblock(K.pack(dec), 16), K.deblock(K.pack(dec), 4)
    assert round(psnr(dec), 1) == 36.5 and round(psnr(K.channels(o16[0])), 1) == 46.4
    assert (o4[0] == K.pack(dec)).all() and o4[1:] == (0, 0)


def test_the_header_and_the_table_agree():
    import test_abi as TA
    from libagmv_amd import abi, build, hip
    protos = TA._prototypes("agmv_hip_deblock.h")
    name = "agmv_hip_deblock_frames_async"
    assert set(protos) == set(abi.HIP_DEBLOCK) == {name}
    assert not set(abi.HIP_DEBLOCK) & (set(abi.HIP) | set(abi.HIP_VIEW) | set(abi.HIP_STABILISE))
    restype, argtypes = abi.HIP_DEBLOCK[name]
    ret, params = protos[name]
    assert TA._ctypes_class(restype) == TA._c_class(ret, True)
    assert [TA._ctypes_class(a) for a in argtypes] == [TA._c_class(p) for p in params]
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "strength", "d_src", "w", "h", "n_frames", "d_dst", "d_counts", "stream"]
    build.build()
    G = hip.load_library()
    f = getattr(G, name)
    assert list(f.argtypes) == list(argtypes) and f.restype is C.c_int
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    assert f(None, 8, p, 4, 4, 2, p, None, None) != 0 and b"NULL context" in G.agmv_hip_last_error()
    assert buf.raw == bytes(4096)


def test_the_host_header_declares_the_knob_and_the_table_holds_it():
    from libagmv_amd import abi
    hdr = open(os.path.join(H.ROOT, "include", "agmv.h")).read()
    assert "void AGMV_SetDeblock(unsigned strength);" in hdr and "void AGMV_GetDeblockStats(AGMV_DEBLOCK_STATS* out);" in hdr
    L = H.lib()
    for name in ("AGMV_SetDeblock", "AGMV_GetDeblockStats"):
        assert name in abi.AGMV and hasattr(L, name)
    st = abi.AGMV_DEBLOCK_STATS(7, 7, 7, 7, 7)
    abi.bind(L, {"AGMV_GetDeblockStats": abi.AGMV["AGMV_GetDeblockStats"]})
    L.AGMV_GetDeblockStats(C.byref(st))
    assert (st.strength, st.frames, st.lines, st.weak, st.strong) == (0, 0, 0, 0, 0)      # no sequence was decoded in this process
    L.AGMV_GetDeblockStats(None)


def test_the_structure_has_the_headers_layout(tmp_path):
    from libagmv_amd import abi
    s = abi.AGMV_DEBLOCK_STATS
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include \"agmv.h\"\nint main(void) {\n"
                   '    printf("%%zu%s\\n", sizeof(%s)%s);\n' % (" %zu" * len(s._fields_), s.__name__, "".join(", offsetof(%s, %s)" % (s.__name__, f[0]) for f in s._fields_))
                   + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", str(src), "-I" + os.path.join(H.ROOT, "include"), "-o", exe], check=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip()
    assert got == "%d%s" % (C.sizeof(s), "".join(" %d" % getattr(s, f[0]).offset for f in s._fields_)) == "32 0 4 8 16 24"


@pytest.mark.parametrize("bad", (0, 65, True, 1.5), ids=repr)
def test_decode_frames_and_file_quality_refuse_deblock_before_the_library_is_loaded(bad, tmp_path, monkeypatch):
    import torch

    import libagmv_amd
    from libagmv_amd import seq

    def reached():
        raise AssertionError("the library was called")
    monkeypatch.setattr(seq, "load_library", reached)
    with pytest.raises(ValueError, match="deblock"):
        libagmv_amd.decode_frames(str(tmp_path / "no such file.agmv"), deblock=bad, scale="no such filter")
    with pytest.raises(ValueError, match="deblock"):
        libagmv_amd.file_quality(str(tmp_path / "no such file.agmv"), torch.zeros((4, 16, 16), dtype=torch.int32), deblock=bad)
