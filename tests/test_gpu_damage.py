"""The decode kernels against the REFERENCE's pixels on damaged streams: the corpus of tests/damage_cases.py, whose decode by the
compiled reference is recorded in tests/golden/golden_damage.json.  The per-frame buffers with their 16 stale bytes come from the
oracle, which tests/test_damage_cpu.py holds to the same record; the pixel hashes asserted here are the reference's.  Both decode
forms (test_gpu_hotpath.gpu_decode), batches cut with carried state, the three parser forms, and the decoder's account of prior
dependence.  Needs an MI355X."""
import hashlib
import json
import os

import numpy as np
import pytest

import damage_cases as D
import oracles as O
import test_gpu_hotpath as HP
from test_gpu_hotpath import hip, torch  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def corpus():
    """[(case, the oracle's frames, the reference's pixel hashes)], computed once"""
    golden = json.load(open(os.path.join(HERE, "golden", "golden_damage.json")))
    out = []
    for c in D.cases():
        err, _, fr = O.oracle_decode_file(D.file_image(c), want_tables=True)
        rec = golden[c["name"]]["frames"]
        assert err == 0 and len(fr) == len(rec)
        out.append((c, fr, [r[2] for r in rec]))
    return out


def decode(torch, hip, c, fr, lo, hi):
    """frames lo .. hi - 1 as one batch, the state before them carried in: (pixels, nentered)"""
    bits = [f["bitstream"][:f["bpos"]] for f in fr[lo:hi]]
    pads = [f["bitstream"][f["bpos"]:] for f in fr[lo:hi]]
    shape = (c["h"], c["w"])
    prev = fr[lo - 1]["pix"].reshape(shape) if lo else None
    previ = fr[(lo - 1) // 4 * 4]["pix"].reshape(shape) if lo else None
    got, _, nent = HP.gpu_decode(torch, hip, bits, pads, c["w"], c["h"], first_fc=lo, prev=prev, prev_iframe=previ)
    return got, nent


def check(c, fr, want, lo, got, nent, how=""):
    for i in range(len(got)):
        t = lo + i
        assert int(nent[i]) == fr[t]["n_entered"], "%s%s frame %d: nentered %d, the oracle's %d" % (c["name"], how, t, nent[i], fr[t]["n_entered"])
        assert sha(got[i]) == want[t], "%s%s frame %d: pixels differ from the reference's" % (c["name"], how, t)


def test_streams_decode_to_the_references_pixels(torch, hip, corpus):
    for c, fr, want in corpus:
        hip.set_palette(c["p0"], c["p1"], D.mode512(c["version"]))
        got, nent = decode(torch, hip, c, fr, 0, len(fr))
        check(c, fr, want, 0, got, nent)


def test_batches_cut_with_carried_state(torch, hip, corpus):
    """one cut at a time, prev / prev_iframe carried: every index for the 4 x 4 and 4 x 24 cases, 3 seeded cuts for the others"""
    rng = np.random.default_rng(4242)
    for c, fr, want in corpus:
        n = len(fr)
        cuts = range(1, n) if c["w"] == 4 else sorted({int(x) for x in rng.integers(1, n, 3)})
        hip.set_palette(c["p0"], c["p1"], D.mode512(c["version"]))
        for cut in cuts:
            for lo, hi in ((0, cut), (cut, n)):
                got, nent = decode(torch, hip, c, fr, lo, hi)
                check(c, fr, want, lo, got, nent, " (batch %d..%d)" % (lo, hi))


@pytest.mark.parametrize("how", ["fast", "robust", "serial"])
def test_parser_forms(torch, hip, corpus, monkeypatch, how):
    if how == "fast":
        monkeypatch.delenv("AGMV_HIP_PARSE", raising=False)
    else:
        monkeypatch.setenv("AGMV_HIP_PARSE", how)
    for c, fr, want in corpus:
        hip.set_palette(c["p0"], c["p1"], D.mode512(c["version"]))
        got, nent = decode(torch, hip, c, fr, 0, len(fr))
        check(c, fr, want, 0, got, nent, " (AGMV_HIP_PARSE=%s)" % how)


def test_the_fast_parser_gives_the_4e_frame_up(torch, hip, corpus, monkeypatch):
    monkeypatch.delenv("AGMV_HIP_PARSE", raising=False)
    for name, given_up in (("run4e_m512", True), ("run4e_m256", True), ("clean_m512", False), ("clean_m256", False)):
        c, fr, _ = next(x for x in corpus if x[0]["name"] == name)
        n = len(fr)
        stride = (max(f["bpos"] for f in fr) + 16 + 255) & ~255
        bits = np.zeros((n, stride), np.uint8)
        for t, f in enumerate(fr):
            bits[t, :f["bpos"] + 16] = f["bitstream"]
        bpos = np.array([f["bpos"] for f in fr], np.int32)
        hip.set_palette(c["p0"], c["p1"], D.mode512(c["version"]))
        _, nent = hip.parse_dev(torch.from_numpy(bits).cuda(), torch.from_numpy(bpos).cuda(), n, c["w"], c["h"])
        torch.cuda.synchronize()
        assert (hip.parse_fallback_frames() > 0) == given_up, (name, hip.parse_fallback_frames())
        assert nent.cpu().tolist() == [f["n_entered"] for f in fr]


def test_prior_dependence_of_gop_2(torch, hip, corpus):
    """a batch that starts at frame 8 from the file's state: where frame 8 holds a P-frame's stream or half an I-frame the decoder says
    that its pixels derive from the state before it, on the clean control it says they do not"""
    for m in ("m512", "m256"):
        for name, dep in (("pframe_at_i_" + m, True), ("truncated_i_" + m, True), ("clean_" + m, False)):
            c, fr, want = next(x for x in corpus if x[0]["name"] == name)
            hip.set_palette(c["p0"], c["p1"], D.mode512(c["version"]))
            bits = [f["bitstream"][:f["bpos"]] for f in fr[8:12]]
            pads = [f["bitstream"][f["bpos"]:] for f in fr[8:12]]
            n, stride = 4, (max(len(b) for b in bits) + 16 + 255) & ~255
            buf = np.zeros((n, stride), np.uint8)
            for i, (b, p) in enumerate(zip(bits, pads)):
                buf[i, :len(b)], buf[i, len(b):len(b) + 16] = b, p
            dbits, dbpos = torch.from_numpy(buf).cuda(), torch.from_numpy(np.array([len(b) for b in bits], np.int32)).cuda()
            offs, nent = hip.parse_dev(dbits, dbpos, n, c["w"], c["h"])
            shape = (c["h"], c["w"])
            out = hip.decode_dev(dbits, dbpos, offs, nent, n, c["w"], c["h"], 8, prev=HP.dev_u32(torch, fr[7]["pix"].reshape(shape)),
                                 prev_iframe=HP.dev_u32(torch, fr[4]["pix"].reshape(shape)))
            torch.cuda.synchronize()
            assert hip.decode_depends_on_prior(c["w"], c["h"]) is dep, name
            check(c, fr, want, 8, HP.to_u32(out).reshape(n, -1), nent.cpu().numpy(), " (GOP 2)")
