"""The temporal stabilisation before any GPU is touched: the properties of the numpy statement (tests/stabilise_cases.py) that
include/agmv.h lists as consequences of the rule; the premise of the knob, through the plain-C encoder of oracle/: on a noisy still
clip, stabilised at a strength at which the statement replaces every block, every P-frame is w * h / 16 COPY flags and nothing
else; include/agmv_hip_stabilise.h against abi.HIP_STABILISE the way tests/test_view_cpu.py holds the view's header; the layout of
AGMV_STABILISE_STATS from gcc; and the ValueErrors of encode_frames(stabilise=), which come before the library is loaded."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dither_cases as D
import hostlib as H
import oracles as O
import stabilise_cases as S

COPY_FLAG = 0x5E


@pytest.mark.parametrize("first_fc", (0, 1, 2, 3, 5))
@pytest.mark.parametrize("s", (1, 8, 64))
def test_the_statement_is_idempotent_and_leaves_i_frames_and_leading_frames_alone(s, first_fc):
    clip = S.random_clip(11, 12, 20, s, 40 + first_fc)
    out, examined, replaced = S.stabilise(clip, s, first_fc)
    again, examined2, replaced2 = S.stabilise(out, s, first_fc)
    assert (again == out).all() and examined2 == examined and replaced2 == replaced
    lead = (4 - (first_fc & 3)) & 3
    assert (out[:lead] == clip[:lead]).all()                                # no anchor in the batch
    assert (out[lead::4] == clip[lead::4]).all()                            # fc & 3 == 0
    assert examined == (11 - lead - len(range(lead, 11, 4))) * 15
    assert 0 < replaced < examined                                          # (the random clip has blocks of both kinds)
    # by hand, frame by frame and block by block, from the header's words
    for k in range(11):
        phase = (first_fc + k) & 3
        for by in range(3):
            for bx in range(5):
                blk = (slice(by * 4, by * 4 + 4), slice(bx * 4, bx * 4 + 4))
                if phase == 0 or k - phase < 0:
                    assert (out[k][blk] == clip[k][blk]).all()
                    continue
                a = clip[k - phase][blk]
                d = np.abs(D.channels(clip[k][blk]) - D.channels(a))
                if d.max() <= s and d.sum() <= 12 * s:
                    assert (out[k][blk] == (a & 0xFFFFFF)).all()
                else:
                    assert (out[k][blk] == clip[k][blk]).all()


@pytest.mark.parametrize("s", S.STRENGTHS)
def test_crafted_blocks_fall_on_the_side_they_were_made_for(s):
    clip, still, names = S.crafted_clip(s)
    out, examined, replaced = S.stabilise(clip, s, 0)
    assert examined == still.size and replaced == int(still.sum())
    assert (out[0] == clip[0]).all()
    for i, name in enumerate(names + ["an equal block"] * (still.size - len(names))):
        y, x = i // S.BLOCKS_PER_ROW * 4, i % S.BLOCKS_PER_ROW * 4
        got, a, p = out[1, y:y + 4, x:x + 4], clip[0, y:y + 4, x:x + 4], clip[1, y:y + 4, x:x + 4]
        if still[i // S.BLOCKS_PER_ROW, i % S.BLOCKS_PER_ROW]:
            assert (got == (a & 0xFFFFFF)).all() and (got >> 24 == 0).all(), name      # bits 24 .. 31 are zero in replaced pixels
        else:
            assert (got == p).all(), name                                              # ... and kept elsewhere
    high = names.index("differences in bits 24 .. 31 only")
    y, x = high // S.BLOCKS_PER_ROW * 4, high % S.BLOCKS_PER_ROW * 4
    assert ((clip[0, y:y + 4, x:x + 4] ^ clip[1, y:y + 4, x:x + 4]) == 0xFF000000).all()      # ignored by the test
    kept = names.index("bits 24 .. 31 of a block that is not still")
    y, x = kept // S.BLOCKS_PER_ROW * 4, kept % S.BLOCKS_PER_ROW * 4
    assert (out[1, y:y + 4, x:x + 4] >> 24 == clip[1, y:y + 4, x:x + 4] >> 24).all()


@pytest.mark.parametrize("mode512", (False, True), ids=("256", "512"))
def test_premise_a_stabilised_still_clip_is_copy_flags(mode512):
    noisy, _ = S.noisy_still_clip()
    n, h, w = noisy.shape
    out, examined, replaced = S.stabilise(noisy, S.NOISY_STRENGTH, 0)
    assert examined == replaced == (n - n // 4) * (w * h // 16)             # first: the statement replaces every block
    _, p0, p1 = D.fox()
    sizes = {}
    for name, clip in (("plain", noisy), ("stabilised", out)):
        enc = O.OracleEncoder(w, h, mode512, p0, p1, 0)
        sizes[name] = [enc.encode(clip[k]) for k in range(n)]
        enc.close()
    for k in range(n):
        if k & 3:
            assert len(sizes["stabilised"][k]) == w * h // 16 and (sizes["stabilised"][k] == COPY_FLAG).all(), k
            assert len(sizes["plain"][k]) > w * h // 16                     # (what the noise costs without the knob)
        else:
            assert (sizes["stabilised"][k] == sizes["plain"][k]).all()      # I-frames are untouched
    print("raw stream bytes of the %d frames: %d plain, %d stabilised" % (n, sum(map(len, sizes["plain"])), sum(map(len, sizes["stabilised"]))))


def test_the_header_and_its_table_state_each_other():
    """include/agmv_hip_stabilise.h against abi.HIP_STABILISE: the same names, the header's return and parameter classes, the
    symbol exported and bound, a NULL context refused with its text before any HIP call"""
    import test_abi as TA
    from libagmv_amd import abi, build, hip
    protos = TA._prototypes("agmv_hip_stabilise.h")
    name = "agmv_hip_stabilise_frames_async"
    assert set(protos) == set(abi.HIP_STABILISE) == {name} and not set(abi.HIP_STABILISE) & (set(abi.HIP) | set(abi.HIP_VIEW))
    restype, argtypes = abi.HIP_STABILISE[name]
    ret, params = protos[name]
    assert TA._ctypes_class(restype) == TA._c_class(ret, True)
    assert [TA._ctypes_class(a) for a in argtypes] == [TA._c_class(p) for p in params]
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "strength", "d_pix", "w", "h", "n_frames", "first_fc", "d_replaced", "stream"]
    build.build()
    G = hip.load_library()
    f = getattr(G, name)
    assert list(f.argtypes) == list(argtypes) and f.restype is C.c_int
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    assert f(None, 8, p, 4, 4, 2, 0, None, None) != 0 and b"NULL context" in G.agmv_hip_last_error()
    assert buf.raw == bytes(4096)


def test_the_host_header_declares_the_knob_and_the_table_holds_it():
    from libagmv_amd import abi
    hdr = open(os.path.join(H.ROOT, "include", "agmv.h")).read()
    assert "void AGMV_SetStabilise(unsigned strength);" in hdr and "void AGMV_GetStabiliseStats(AGMV_STABILISE_STATS* out);" in hdr
    L = H.lib()
    for name in ("AGMV_SetStabilise", "AGMV_GetStabiliseStats"):
        assert name in abi.AGMV and hasattr(L, name)
    st = abi.AGMV_STABILISE_STATS(7, 7)
    abi.bind(L, {"AGMV_GetStabiliseStats": abi.AGMV["AGMV_GetStabiliseStats"]})
    L.AGMV_GetStabiliseStats(C.byref(st))
    assert (st.examined, st.replaced) == (0, 0)                             # no sequence was encoded in this process
    L.AGMV_GetStabiliseStats(None)


def test_the_structure_has_the_headers_layout(tmp_path):
    from libagmv_amd import abi
    s = abi.AGMV_STABILISE_STATS
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include \"agmv.h\"\nint main(void) {\n"
                   '    printf("%%zu%s\\n", sizeof(%s)%s);\n' % (" %zu" * len(s._fields_), s.__name__, "".join(", offsetof(%s, %s)" % (s.__name__, f[0]) for f in s._fields_))
                   + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", str(src), "-I" + os.path.join(H.ROOT, "include"), "-o", exe], check=True)
    line = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip()
    assert line == "%d%s" % (C.sizeof(s), "".join(" %d" % getattr(s, f[0]).offset for f in s._fields_)) == "16 0 8"


@pytest.mark.parametrize("bad", (0, 65, True, 1.5), ids=repr)
def test_encode_frames_refuses_stabilise_before_the_library_is_loaded(bad, tmp_path, monkeypatch):
    import torch

    import libagmv_amd
    from libagmv_amd import seq

    def reached():
        raise AssertionError("the library was called")
    monkeypatch.setattr(seq, "load_library", reached)
    frames = torch.zeros((4, 16, 16), dtype=torch.int32)
    with pytest.raises(ValueError, match="stabilise"):
        libagmv_amd.encode_frames(str(tmp_path / "x.agmv"), frames, stabilise=bad, scale="no such filter")
    assert not (tmp_path / "x.agmv").exists()
