"""host side of the drop-in library (libagmv_amd/libagmv.so): LZ stage, palette build, BMP, synth.
CPU only; checked against the oracle restatement and -- where built -- the compiled reference."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import children as K
import hostlib as H
import oracles as O
import synth as S

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built here")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def lz_cases():
    rng = np.random.default_rng(12)
    yield np.zeros(0, np.uint8)
    yield np.array([7], np.uint8)
    yield rng.integers(0, 256, 3000, dtype=np.uint8)                  # incompressible
    yield rng.integers(0, 3, 5000, dtype=np.uint8)                    # many short matches, ties
    yield np.full(4000, 0x5E, np.uint8)                               # one long run (COPY-heavy P-frame)
    yield np.tile(rng.integers(0, 256, 17, dtype=np.uint8), 300)      # periodic: earliest-start tie rule
    a = np.full(3000, 0x5E, np.uint8)
    a[::97] = 0x4E
    a[1::97] = rng.integers(0, 256, len(a[1::97]), dtype=np.uint8)
    yield a                                                           # runs broken by FILL blocks
    yield np.concatenate([rng.integers(0, 256, 70000, dtype=np.uint8)[:200].repeat(2), np.arange(256, dtype=np.uint8)])


@pytest.mark.parametrize("case", range(8))
def test_fast_lz_matches_brute_force_oracle(case):
    x = list(lz_cases())[case]
    L = O.oracle()
    xin = np.concatenate([x, np.zeros(8, np.uint8)])
    for name, fast, slow in (("lzss", H.lzss, L.orc_lzss_compress), ("lz77", H.lz77, L.orc_lz77_compress)):
        out = np.zeros(4 * len(x) + 64, np.uint8)
        cs = C.c_uint32()
        n = slow(xin, len(x), out, C.byref(cs))
        got, gcs = fast(x)
        assert gcs == cs.value, name
        # the reference file keeps exactly csize payload bytes (the flushed partial byte is overwritten)
        assert (got == out[:cs.value]).all(), name
        assert n in (cs.value, cs.value + 1)


def test_lz_window_limit_and_long_input():
    """matches must start within 65535 bytes: a repeat 70000 bytes later must not be found."""
    rng = np.random.default_rng(5)
    block = rng.integers(0, 256, 64, dtype=np.uint8)
    x = np.concatenate([block, rng.integers(0, 256, 70000, dtype=np.uint8), block])
    L = O.oracle()
    out = np.zeros(4 * len(x) + 64, np.uint8)
    cs = C.c_uint32()
    L.orc_lzss_compress(np.concatenate([x, np.zeros(8, np.uint8)]), len(x), out, C.byref(cs))
    got, gcs = H.lzss(x)
    assert gcs == cs.value and (got == out[:gcs]).all()


def test_lz_golden(golden):
    frames = [S.synth_frame(320, 240, t) for t in range(2)]
    p0, p1 = S.content_palettes(frames)
    enc = O.OracleEncoder(320, 240, True, p0, p1)
    for k, f in enumerate(frames):
        o = enc.encode(f)
        for name, fast in (("lzss", H.lzss), ("lz77", H.lz77)):
            g = golden["lz_320x240"]["%s_%d" % (name, k)]
            got, cs = fast(o)
            assert cs == g["csize"]
            # golden holds the reference's full output incl. the flushed byte; compare the csize prefix hash-free
            assert len(got) == g["csize"]


def test_lz_decode_roundtrip_and_guard_bytes():
    rng = np.random.default_rng(3)
    x = np.tile(rng.integers(0, 256, 40, dtype=np.uint8), 60)
    for ver, fast in ((1, H.lzss), (3, H.lz77)):
        comp, cs = fast(x)
        payload = np.concatenate([comp, np.full(8, 0xFF, np.uint8), np.frombuffer(b"AGFC", np.uint8)])
        data = np.zeros(len(x) + 64, np.uint8)
        used = C.c_size_t(0)
        bpos = H.lib().agmv_lz_decode_mem(ver, payload, len(payload), len(x), cs, data, len(data), C.byref(used))
        d = O.oracle().orc_decoder_new(8, 8 * ((len(x) + 63) // 64 + 1), ver, np.zeros(256, np.uint32), np.zeros(256, np.uint32))
        dec = C.cast(d, C.POINTER(O._OrcDecoder)).contents
        used2 = O.oracle().orc_decoder_lz(d, payload.ctypes.data, len(payload), len(x), cs)
        assert bpos == dec.bpos and used.value == used2
        assert (data[:bpos] == np.ctypeslib.as_array(dec.bitstream, (bpos,))).all()
        O.oracle().orc_decoder_free(d)


def test_bubble_sort_is_the_stable_sort():
    rng = np.random.default_rng(8)
    n = 2000
    data = rng.integers(0, 20, n).astype(np.uint64)
    gram = np.arange(n, dtype=np.uint64)
    d2, g2 = data.copy(), gram.copy()
    H.lib().AGMV_BubbleSort(d2, g2, n)
    order = np.argsort(data, kind="stable")
    assert (d2 == data[order]).all() and (g2 == gram[order]).all()


def test_quantize_helpers():
    L = H.lib()
    for q, (rs, gs, bs) in ((1, (2, 2, 1)), (2, (3, 2, 2)), (3, (3, 2, 3))):
        for c in (0x000000, 0xFFFFFF, 0x123456, 0xFE01A7):
            r, g, b = c >> 16, (c >> 8) & 255, c & 255
            rb, gb, bb = 8 - rs, 8 - gs, 8 - bs
            code = (r >> rs) << (gb + bb) | (g >> gs) << bb | (b >> bs)
            assert L.AGMV_QuantizeColor(c, q) == code
            assert L.AGMV_ReverseQuantizeColor(code, q) == ((r >> rs << rs) << 16 | (g >> gs << gs) << 8 | (b >> bs << bs))
    assert [L.AGMV_GetVersionFromOPT(o, 1) for o in range(1, 9)] == [1, 2, 1, 2, 1, 2, 1, 1]
    assert [L.AGMV_GetVersionFromOPT(o, 2) for o in range(1, 9)] == [3, 4, 3, 4, 3, 4, 3, 3]


def test_host_synth_matches_numpy():
    for (W, H_) in ((320, 240), (68, 36)):
        for t in (0, 1, 9):
            out = np.zeros(W * H_, np.uint32)
            H.lib().AGMV_SynthFrame(out, W, H_, t, S.DEFAULT_SEED)
            assert (out.reshape(H_, W) == S.synth_frame(W, H_, t)).all()


def test_bmp_roundtrip(tmp_path):
    f = S.synth_frame(68, 36, 2)[:, :66].copy()       # width % 4 != 0 exercises AGIDL's padding rule
    p = str(tmp_path / "x.bmp")
    H.write_bmp(p, f)
    raw = open(p, "rb").read()
    assert len(raw) == 54 + (66 * 3 + 66 % 4) * 36 and raw[:2] == b"BM"
    pix = C.POINTER(C.c_uint32)()
    w, h = C.c_uint32(), C.c_uint32()
    assert H.lib().agmv_bmp_load(p.encode(), C.byref(pix), C.byref(w), C.byref(h)) == 0
    got = np.ctypeslib.as_array(pix, (h.value, w.value))
    assert (got == f).all()


@needs_ref
def test_palette_build_matches_reference_file(tmp_path):
    """the palette the reference's AGMV_EncodeAGMV writes into the header for a small synthetic clip
    (its real histogram + bubble sort + greedy pick + slot map) against AGMV_BuildPalette."""
    W, H_, T = 64, 48, 12
    d = tmp_path / "fr"
    d.mkdir()
    frames = [S.synth_frame(W, H_, t) for t in range(1, T + 1)]
    for t, f in enumerate(frames, 1):
        H.write_bmp(str(d / ("f%d.bmp" % t)), f)
    # run the reference driver in a child process (it frees its AGMV and writes into CWD)
    for opt, quality in ((3, 3), (2, 2)):
        assert K.drive_child(tmp_path, "agmv", T, W, H_, opt, quality, 1, out="ref.agmv", so=O.REF_SO).returncode == 0
        hdr = open(tmp_path / "ref.agmv", "rb").read()
        npal = 2 if opt == 3 else 1
        ref_pal = np.frombuffer(hdr[38:38 + 768 * npal], np.uint8).reshape(-1, 3).astype(np.uint32)
        ref_pal = ref_pal[:, 0] << 16 | ref_pal[:, 1] << 8 | ref_pal[:, 2]
        shifts = {3: (3, 2, 3, 11, 5), 2: (3, 2, 2, 12, 6)}[quality]
        allpx = np.concatenate([f.reshape(-1) for f in frames])
        r, g, b = (allpx >> 16) & 255, (allpx >> 8) & 255, allpx & 255
        code_ = ((r >> shifts[0]) << shifts[3]) | ((g >> shifts[1]) << shifts[4]) | (b >> shifts[2])
        hist = np.bincount(code_, minlength=1 << 19).astype(np.uint32)
        p0 = np.zeros(256, np.uint64)
        p1 = np.zeros(256, np.uint64)
        H.lib().AGMV_BuildPalette(hist, quality, opt, p0, p1)
        mine = np.concatenate([p0, p1])[:256 * npal].astype(np.uint32)
        assert (mine == ref_pal).all(), (opt, quality, int((mine != ref_pal).sum()))


def test_find_smallest_helpers_match_reference():
    """AGMV_FindSmallestColor / AGMV_FindSmallestEntry (reference src/agmv_utils.c:818-849, :897-914; unused by the
    library, part of its API): first 200 slots only, entry chosen by the smaller index."""
    rng = np.random.default_rng(11)
    p0 = rng.integers(0, 1 << 24, 256).astype(np.uint64)
    p1 = rng.integers(0, 1 << 24, 256).astype(np.uint64)
    p1[7] = p0[3]
    cols = [int(c) for c in rng.integers(0, 1 << 24, 200)] + [int(p0[3]), int(p0[250]), 0, 0xFFFFFF]
    libs = [H.lib()] + ([H.bind(C.CDLL(O.REF_SO), missing_ok=True)] if O.have_ref() else [])

    def smallest(pal, c):
        ch = lambda v, s: (v >> s) & 255
        d = [(ch(c, 16) - ch(int(q), 16)) ** 2 + (ch(c, 8) - ch(int(q), 8)) ** 2 + (ch(c, 0) - ch(int(q), 0)) ** 2 for q in pal[:200]]
        return int(np.argmin(d))

    for c in cols:
        want0, want1 = smallest(p0, c), smallest(p1, c)
        want = (0, want0) if want0 <= want1 else (1, want1)
        for L in libs:
            assert L.AGMV_FindSmallestColor(p0.ctypes.data, c) == want0
            e = L.AGMV_FindSmallestEntry(p0.ctypes.data, p1.ctypes.data, c)
            assert (e.pal_num, e.index) == want


def test_display_frame_and_header_export(tmp_path):
    L = H.lib()
    # AGMV_ExportAGMVToHeader: ./agmv.h, byte-identical to the reference's when it is built here
    src = tmp_path / "clip.agmv"
    src.write_bytes(bytes(range(256)) * 5 + b"tail")
    outs = []
    for so in [H.SO] + ([O.REF_SO] if O.have_ref() else []):
        d = tmp_path / ("o%d" % len(outs))
        d.mkdir()
        code = "import ctypes,os;os.chdir(%r);L=ctypes.CDLL(%r);L.AGMV_ExportAGMVToHeader(%r)" % (str(d), so, str(src).encode())
        assert os.system("%s -c %r" % (os.sys.executable, code)) == 0
        outs.append((d / "agmv.h").read_bytes())
    assert outs[0].startswith(b"#ifndef AGMV_H\n#define AGMV_H\n\n#define FILE_SIZE 1284\n\nconst unsigned char agmv_file[FILE_SIZE] = {\n0,1,2,")
    assert outs[0].count(b"\n") == 6 + 2 + 1 and outs[0].endswith(b"116,97,105,108,};\n#endif")
    assert all(o == outs[0] for o in outs)
    # PlotPixel clips; AGMV_DisplayFrame copies the frame into the top-left of a larger (or smaller) target
    vram = np.zeros(6 * 4, np.uint64)
    for (x, y) in ((-1, 0), (0, -1), (6, 0), (0, 4), (5, 3), (2, 1)):
        L.PlotPixel(vram.ctypes.data, x, y, 6, 4, 0xABCDEF)
    assert sorted(np.nonzero(vram)[0].tolist()) == [2 + 6, 5 + 18]


@pytest.mark.parametrize("seed", range(int(os.environ.get("AGMV_FUZZ_SEEDS", "24"))))
def test_lz_fuzz_vs_brute_force_oracle(seed):
    """seeded fuzz of the fast LZSS / LZ77 against the brute-force restatement: bitstream-like inputs (flag bytes,
    runs, repeated fragments at random distances, noise) of random length; also decode(fast encode) == input."""
    rng = np.random.default_rng(9000 + seed)
    n = int(rng.integers(1, 6000))
    parts, have = [], 0
    while have < n:
        kind = int(rng.integers(0, 5))
        ln = int(rng.integers(1, 400))
        if kind == 0:
            p = rng.integers(0, 256, ln, dtype=np.uint8)
        elif kind == 1:
            p = np.full(ln, [0x5E, 0x4E, 0x2F, 0, 0xFF][int(rng.integers(0, 5))], np.uint8)
        elif kind == 2 and parts:
            src = np.concatenate(parts)
            at = int(rng.integers(0, len(src)))
            p = src[at:at + ln].copy()
        elif kind == 3:
            p = np.tile(rng.integers(0, 256, int(rng.integers(1, 20)), dtype=np.uint8), ln // 4 + 1)[:ln]
        else:
            p = rng.integers(0, 4, ln, dtype=np.uint8) + np.uint8(0x4C)
        parts.append(p)
        have += len(p)
    x = np.concatenate(parts)[:n]
    L = O.oracle()
    xin = np.concatenate([x, np.zeros(8, np.uint8)])
    for name, fast, slow in (("lzss", H.lzss, L.orc_lzss_compress), ("lz77", H.lz77, L.orc_lz77_compress)):
        out = np.zeros(4 * len(x) + 64, np.uint8)
        cs = C.c_uint32()
        slow(xin, len(x), out, C.byref(cs))
        got, gcs = fast(x)
        assert gcs == cs.value, (name, seed)
        assert (got == out[:cs.value]).all(), (name, seed)
