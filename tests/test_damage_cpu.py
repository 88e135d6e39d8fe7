"""The oracle's DECODER against the compiled reference on damaged files (tests/damage_cases.py): against the recorded fixture
tests/golden/golden_damage.json everywhere, and live where oracle/_ref exists -- there also on seeded mixes beyond the fixture, the
numpy header against AGMV_EncodeHeader, and OracleEncoder against the reference's encoder on random content.  No GPU."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import damage_cases as D
import oracles as O
import synth as S

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = int(os.environ.get("AGMV_FUZZ_SEEDS", "24"))
needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built (no reference on this machine)")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "golden_damage.json")))


@pytest.fixture(scope="module")
def decoded():
    """every case through the oracle, once: name -> frames of oracle_decode_file(want_tables=True)"""
    out = {}
    for c in D.cases():
        err, info, fr = O.oracle_decode_file(D.file_image(c), want_tables=True)
        assert err == 0 and (info.w, info.h, info.version) == (c["w"], c["h"], c["version"])
        out[c["name"]] = fr
    return out


def same_as_reference(name, fr, rec):
    """oracle frames against [err, bpos, pixel sha, sha of bitstream[:bpos + 16]] of the reference"""
    assert len(fr) == len(rec) and all(r[0] == 0 for r in rec), "%s: the oracle decodes %d frames, the reference %d" % (name, len(fr), len(rec))
    for t, (f, r) in enumerate(zip(fr, rec)):
        assert f["bpos"] == r[1], "%s frame %d: bpos %d, the reference's %d" % (name, t, f["bpos"], r[1])
        assert sha(f["bitstream"]) == r[3], "%s frame %d: the buffer with its 16 stale bytes differs from the reference's" % (name, t)
        assert sha(f["pix"]) == r[2], "%s frame %d: pixels differ from the reference's" % (name, t)


def test_the_corpus_is_the_recorded_one(golden):
    assert sorted(golden) == sorted(c["name"] for c in D.cases()), "the corpus changed: run tests/golden/make_golden_damage.py"
    for c in D.cases():
        assert hashlib.sha256(D.file_image(c)).hexdigest() == golden[c["name"]]["file_sha"], \
            "the corpus changed (%s): this is not a decoder's fault; run tests/golden/make_golden_damage.py" % c["name"]
        assert len(D.layout(c)[1]) == len(golden[c["name"]]["frames"]) and 8 <= len(c["frames"]) <= 24


def test_oracle_decodes_damaged_files_as_the_reference_did(golden, decoded):
    for c in D.cases():
        same_as_reference(c["name"], decoded[c["name"]], golden[c["name"]]["frames"])


def fresh_decode(c, fr, lo, hi):
    """frames lo .. hi - 1 of a decoded case again from the fresh state (zeroed pixels, I-frame and buffer)"""
    dec = O.OracleDecoder(c["w"], c["h"], D.mode512(c["version"]), c["p0"], c["p1"])
    dec.set_state(frame_count=lo)
    out = [dec.decode(fr[t]["bitstream"][:fr[t]["bpos"]]) for t in range(lo, hi)]
    dec.close()
    return out


def test_the_corpus_reaches_what_it_claims(decoded):
    """from the oracle's tables alone, so that a later edit cannot hollow the corpus out"""
    by = {c["name"]: c for c in D.cases()}
    seen = dict.fromkeys(["not every block entered", "resync across bpos", "stale COPY changed pixels", "quirk colour", "GOP depends on prior",
                          "LZSS bpos > usize", "LZ77 bpos != usize", "bpos < usize", "empty payload", "a chunk lost to the scan"], 0)
    for name, fr in decoded.items():
        c = by[name]
        w, h, m512 = c["w"], c["h"], D.mode512(c["version"])
        nblk = w * h // 16
        seen["a chunk lost to the scan"] += len(fr) < len(c["frames"])
        dec = O.OracleDecoder(w, h, m512, c["p0"], c["p1"])
        for t, f in enumerate(fr):
            bp, ne, bits = f["bpos"], f["n_entered"], f["bitstream"]
            state = dec.state()
            pix = dec.decode(bits[:bp])                        # (the replay: the same buffer, so the same stale bytes)
            assert (pix == f["pix"]).all()
            seen["not every block entered"] += ne < nblk
            seen["empty payload"] += bp == 0
            if c["version"] in (1, 2):
                seen["LZSS bpos > usize"] += bp > f["usize"]
                seen["bpos < usize"] += bp < f["usize"]
            else:
                seen["LZ77 bpos != usize"] += bp != f["usize"]
            last = int(f["offsets"][ne - 1]) if ne else 0
            if ne and last < bp and not any(int(b) in (D.FILL, D.NORMAL, D.COPY) for b in bits[last:bp]):
                seen["resync across bpos"] += 1                # the last block entered found no flag before bpos
            if ne and ne < nblk + 1 and bits[bp] == D.COPY or (bp + 1 < len(bits) and bits[bp + 1] == D.COPY):
                zero = O.OracleDecoder(w, h, m512, c["p0"], c["p1"])
                buf = state[3].copy()
                buf[:bp] = bits[:bp]
                buf[bp:bp + 16] = 0
                zero.set_state(state[0].reshape(h, w), state[1].reshape(h, w), state[2], buf)
                seen["stale COPY changed pixels"] += bool((zero.decode(bits[:bp]) != pix).any())
                zero.close()
            if ne == nblk and int(bits[f["offsets"][nblk - 1]]) == D.FILL and f["offsets"][nblk - 1] + 2 <= bp:
                k = int(bits[f["offsets"][nblk - 1] + 1])
                own = (c["p1"] if k >> 7 else c["p0"])[k & 0x7F] if m512 and (k & 0x7F) < 127 else c["p0"][k] if not m512 else None
                seen["quirk colour"] += own is not None and int(pix[-1]) != int(own)
        dec.close()
        for lo in range(4, len(fr), 4):
            again = fresh_decode(c, fr, lo, min(lo + 4, len(fr)))
            seen["GOP depends on prior"] += any((a != fr[lo + i]["pix"]).any() for i, a in enumerate(again))
    assert all(seen.values()), seen
    dep = lambda n: any((a != decoded[n][8 + i]["pix"]).any() for i, a in enumerate(fresh_decode(by[n], decoded[n], 8, 12)))
    for m in ("m512", "m256"):
        assert dep("pframe_at_i_" + m) and dep("truncated_i_" + m) and not dep("clean_" + m)


def ref_frames(tmp_path, c):
    path = str(tmp_path / "d.agmv")
    open(path, "wb").write(D.file_image(c))
    err, geom, fr = O.ref_decode_file(path, want_bitstream=True)
    assert err == 0 and geom == (c["w"], c["h"], len(D.layout(c)[1]), c["version"])
    return [[f["err"], f["bpos"], sha(f["pix"]), sha(f["bitstream"])] for f in fr]


@needs_ref
def test_oracle_against_the_reference_live(tmp_path, golden, decoded):
    for c in D.cases():
        rec = ref_frames(tmp_path, c)
        assert rec == golden[c["name"]]["frames"], "%s: the fixture is not what the reference gives today" % c["name"]
        same_as_reference(c["name"], decoded[c["name"]], rec)


@needs_ref
@pytest.mark.parametrize("seed", range(SEEDS))
def test_seeded_mixes_beyond_the_fixture(tmp_path, seed):
    rng = np.random.default_rng(88000 + seed)
    w, h = 4 * int(rng.integers(1, 33)), 4 * int(rng.integers(1, 25))
    c = D.try_mix_case("live_%d" % seed, 88000 + seed, w, h, 1 + seed % 4, "content" if rng.integers(0, 2) else "random")
    if c is None:                                              # the draw broke a bound of the corpus: nothing the reference may be given
        return
    err, info, fr = O.oracle_decode_file(D.file_image(c), want_tables=True)
    assert err == 0
    same_as_reference(c["name"], fr, ref_frames(tmp_path, c))


@needs_ref
@pytest.mark.parametrize("version", [1, 2, 3, 4])
def test_numpy_header_is_the_reference_encoders(tmp_path, version):
    p0, p1 = S.random_palettes(version)
    a = O.ref().refshim_create(68, 36, O.OPT_III if D.mode512(version) else O.OPT_II, O.LZSS if version < 3 else O.LZ77, p0, p1)
    path = str(tmp_path / "h.agmv")
    O.ref().refshim_write_header(a, path.encode())
    O.ref().refshim_destroy(a)
    ref = open(path, "rb").read()
    le = lambda at, n: int.from_bytes(ref[at:at + n], "little")
    assert ref[17] == version
    mine = D.header(le(4, 4), 68, 36, version, p0, p1, fps=le(18, 4), total_audio_duration=le(22, 4), sample_rate=le(26, 4), audio_size=le(30, 4),
                    channels=le(34, 2), bits_per_sample=le(36, 2))
    assert mine == ref


@needs_ref
@pytest.mark.parametrize("seed", range(SEEDS))
def test_oracle_encoder_against_the_reference_on_random_content(seed):
    """the content kinds and geometries of test_fuzz_encode_decode_vs_oracle (tests/test_gpu_hotpath.py), frames capped at 128 x 96"""
    rng = np.random.default_rng(99000 + seed)
    w, h = 4 * int(rng.integers(1, 33)), 4 * int(rng.integers(1, 25))
    n, m512, fc = int(rng.integers(1, 10)), bool(rng.integers(0, 2)), int(rng.choice([0, 1, 4, 6]))
    frames = D.content_frames(rng, w, h, n)
    p0, p1 = S.content_palettes(frames[:4]) if rng.integers(0, 2) else S.random_palettes(int(rng.integers(0, 1 << 30)))
    a, b = O.OracleEncoder(w, h, m512, p0, p1, fc), O.RefEncoder(w, h, m512, p0, p1, fc)
    if fc % 4:                                                 # a clip that starts on a P-frame: the I-frame plane is the zeroed one the oracle starts
        O.ref().refshim_set_iframe_entries.argtypes = [C.c_void_p, O.u16p]            # from (the reference's is malloc'ed and never set)
        O.ref().refshim_set_iframe_entries(b.p, np.zeros(w * h, np.uint16))
    for t, f in enumerate(frames):
        (sa, ea), (sb, eb) = a.encode(f, True), b.encode(f, True)
        assert (ea == eb).all(), "entries, frame %d of %dx%d mode512=%s first_fc=%d" % (t, w, h, m512, fc)
        assert len(sa) == len(sb) and (sa == sb).all(), "stream, frame %d of %dx%d mode512=%s first_fc=%d" % (t, w, h, m512, fc)
    a.close()
    b.close()
