"""Whole files from and to clips in the caller's pixel layout: AGMV_EncodeFramesFmtDev / AGMV_DecodeFramesFmtDev of
libagmv_amd/libagmv.so, and libagmv_amd.seq on torch tensors.

Encode: the clips of the file goldens, converted to RGB24 / BGR24 / RGBA32 / planar RGB8 in numpy (tests/pixfmt_cases.py) and
uploaded with agmv_hip_malloc, must become the files the compiled reference wrote (sha256 in tests/golden/golden.json and
tests/golden/golden_memseq.json): the palette then comes from agmv_hip_histogram_fmt_dev, plain frames from
agmv_hip_pixels_to_xrgb_dev, scaled ones from agmv_hip_gather_fmt_dev, midpoints from both, and on the mixed clip the counts
of agmv_hip_similarity_fmt_dev decide which frames exist.  Decode: the frames, converted back in numpy, must be the pixels of
the goldens and of AGMV_DecodeFramesDev.  Child processes and batches of 8 frames as in tests/test_gpu_memseq.py.  Needs an MI355X."""
import functools
import hashlib
import json
import os
import tempfile
import textwrap

import numpy as np
import pytest

import children as K
import hostlib as H
import memseq_cases as MC
import pixfmt_cases as P
import synth as S

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(TESTS, "golden")
SCHEDULE = {"full": 1, "agmv": 2, "video": 3}
FIRST = "agmv_opt3_low_lzss_160x128"

CHILD = textwrap.dedent("""
    import pixfmt_cases as P
    L.AGMV_SetBatchFrames(job["batch"])
    res = {"enc_rc": [], "dec": [], "bad_rc": []}

    for e in job.get("enc", []):
        fr = np.load("frames.npy")
        n, h, w = fr.shape
        alpha = np.random.default_rng(5).integers(0, 256, (n, h * w), dtype=np.uint8)
        raw = np.ascontiguousarray(P.from_packed(e["fmt"], fr.reshape(n, h * w), alpha=alpha))
        d = upload(raw)
        res["enc_rc"].append(L.AGMV_EncodeFramesFmtDev(e["out"].encode(), d, e["fmt"], n, w, h, 24, e["opt"], e["quality"], e["compression"], e["schedule"]))
        free(d)
    for a in job.get("bad", []):             # [filename, fmt, n, w, h, opt, quality, compression, schedule] on a real clip
        d = upload(np.zeros(8 * 16 * 16 * 4, np.uint8))
        res["bad_rc"].append(L.AGMV_EncodeFramesFmtDev(a[0].encode(), d, a[1], *a[2:5], 24, *a[5:]))
        free(d)
    for e in job.get("dec", []):             # fmt 0: AGMV_DecodeFramesDev
        path = e["path"].encode()
        info = INFO()
        rc_info = L.AGMV_DecodeFramesFmtDev(path, None, e["fmt"] or 1, 0, C.byref(info))
        n, w, h = info.number_of_frames, info.width, info.height
        nbytes = n * P.frame_bytes(e["fmt"] or 1, w * h)
        d = poisoned(nbytes)                                            # what a frame that is not decoded keeps
        cap = e.get("cap", n)
        rc = L.AGMV_DecodeFramesFmtDev(path, d, e["fmt"], cap, None) if e["fmt"] else L.AGMV_DecodeFramesDev(path, d, cap, None)
        np.save(e["out"], download(d, nbytes))
        free(d)
        res["dec"].append({"info_rc": rc_info, "rc": rc, "n": n, "w": w, "h": h})
    print(json.dumps(res))
""")

# libagmv_amd.seq on torch tensors, in a child as well (the drivers keep process-wide state)
SEQ_CHILD = textwrap.dedent("""
    import json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    fr = torch.from_numpy(np.load("frames.npy").astype(np.int64)).cuda()                # [n, h, w] 0x00RRGGBB
    rgb = torch.stack([(fr >> 16) & 255, (fr >> 8) & 255, fr & 255], dim=3).to(torch.uint8).contiguous()
    libagmv_amd.encode_frames("hwc.agmv", rgb)                                          # uint8 [n, h, w, 3]: rgb24
    libagmv_amd.encode_frames("chw.agmv", rgb.permute(0, 3, 1, 2).contiguous())         # uint8 [n, 3, h, w]: rgb8p
    packed, info = libagmv_amd.decode_frames("hwc.agmv")
    out, _ = libagmv_amd.decode_frames("hwc.agmv", fmt="rgb24")
    planes, _ = libagmv_amd.decode_frames("hwc.agmv", fmt="rgb8p")
    rgba, _ = libagmv_amd.decode_frames("hwc.agmv", fmt="rgba32")
    p = packed.to(torch.int64)
    exp = torch.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], dim=3).to(torch.uint8)
    print(json.dumps({"rgb24": [str(out.dtype), list(out.shape), bool((out == exp).all())],
                      "rgb8p": [str(planes.dtype), list(planes.shape), bool((planes == exp.permute(0, 3, 1, 2)).all())],
                      "rgba32": [str(rgba.dtype), list(rgba.shape), bool((rgba[..., :3] == exp).all() and (rgba[..., 3] == 255).all())],
                      "packed": [str(packed.dtype), list(packed.shape)], "frames": int(info.number_of_frames)}))
""")


def run_child(cwd, job, env=None, script=CHILD):
    return K.run_child(cwd, script, job, env, prelude="" if script is SEQ_CHILD else K.PRELUDE)


@functools.lru_cache(maxsize=None)
def clip(W, Hh, T):
    """frames 1..T of the canonical clip through the library's C statement of it (tests/test_hostlib.py holds it to tests/synth.py)"""
    L = H.lib()
    out = np.empty((T, Hh, W), np.uint32)
    for t in range(1, T + 1):
        L.AGMV_SynthFrame(out[t - 1].reshape(-1), W, Hh, t, S.DEFAULT_SEED)
    out.setflags(write=False)
    return out


def golden_of(name):
    if name in MC.MIXED_CASES:
        return json.load(open(os.path.join(GOLDEN, "golden_memseq.json")))[name], MC.mixed_clip()
    g = json.load(open(os.path.join(GOLDEN, "golden.json")))["files"][name]
    return g, clip(g["W"], g["H"], g["T"])


@functools.lru_cache(maxsize=None)
def encoded(name, fmt, lz_device=False):
    """the clip of golden `name` in layout fmt -> AGMV_EncodeFramesFmtDev in a child; run once"""
    g, frames = golden_of(name)
    env = {"AGMV_LZ_DEVICE": "1"} if lz_device else {}
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "frames.npy"), frames)
        res = run_child(d, {"batch": 8, "enc": [dict(g, fmt=fmt, schedule=SCHEDULE[g["driver"]], out="out.agmv")]}, env)
        assert res["enc_rc"] == [0]
        data = open(os.path.join(d, "out.agmv"), "rb").read()
    return g, data


def check_file(data, g):
    assert int.from_bytes(data[4:8], "little") == g["frames"]
    assert int.from_bytes(data[18:22], "little") == g["fps_field"]
    assert len(data) == g["file_len"]
    assert hashlib.sha256(data).hexdigest() == g["file_sha"], "the .agmv file differs from the reference's"


RGB24_CASES = [FIRST, "agmv_opt1_mid_lzss_160x128", "agmv_opt2_low_lz77_160x128", "full_opt3_high_lzss_160x128",
               "video_opt3_low_lzss_160x128", "agmv_gba1_low_lzss_320x240", "agmv_nds_low_lzss_320x240"]
ENCODE = ([(P.RGB24, n) for n in RGB24_CASES] + [(f, n) for f in (P.BGR24, P.RGBA32, P.RGB8P) for n in (FIRST, "agmv_gba1_low_lzss_320x240")] +
          [(f, "mixed_video_opt3_low_lzss_160x128") for f in P.NEW])


@pytest.mark.parametrize("fmt,name", ENCODE, ids=["%s-%s" % (P.NAMES[f], n) for f, n in ENCODE])
def test_encode_from_clip_in_format_matches_reference(fmt, name):
    g, data = encoded(name, fmt)
    if name in MC.MIXED_CASES:
        assert g["chain"].count(1) >= 2 and g["chain"].count(0) >= 2            # the adaptive chain takes both branches
    check_file(data, g)


def test_encode_with_the_lz_stage_on_the_device():
    g, data = encoded(FIRST, P.RGB24, True)
    check_file(data, g)


def pix_sha(frame):
    return hashlib.sha256(np.ascontiguousarray(frame, np.uint32).tobytes()).hexdigest()


@pytest.mark.parametrize("fmt", P.NEW, ids=[P.NAMES[f] for f in P.NEW])
def test_decode_into_clip_in_format(fmt, tmp_path):
    """three files and a capped decode in one child: the encoder's own file (against AGMV_DecodeFramesDev in the same child), the
    reference's agmv_splash (escape frames and stale tails: the state must come from the packed double buffer, not from the
    caller's bytes) and FOXLOGO (AGAC chunks between the frames), both against the pix_sha goldens"""
    g, data = encoded(FIRST, P.RGB24)
    open(tmp_path / "first.agmv", "wb").write(data)
    files = {"first": "first.agmv", "splash": os.path.join(GOLDEN, "agmv_splash.agmv"), "fox": os.path.join(GOLDEN, "FOXLOGO.agmv")}
    jobs = [{"path": files["first"], "fmt": 0, "out": "first_packed.npy"}, {"path": files["first"], "fmt": fmt, "out": "first.npy"},
            {"path": files["splash"], "fmt": fmt, "out": "splash.npy"}, {"path": files["fox"], "fmt": fmt, "out": "fox.npy"},
            {"path": files["first"], "fmt": fmt, "cap": 11, "out": "cap.npy"}]
    res = run_child(tmp_path, {"batch": 8, "dec": jobs})["dec"]
    gold = {"splash": json.load(open(os.path.join(GOLDEN, "golden.json")))["agmv_splash"],
            "fox": json.load(open(os.path.join(GOLDEN, "golden_foxlogo.json")))["FOXLOGO"]}

    def frames_of(r, out):
        n, npx = r["n"], r["w"] * r["h"]
        raw = np.load(tmp_path / out).reshape(n, P.frame_bytes(fmt, npx))
        pix, alpha = P.to_packed(fmt, raw, npx)
        return raw, pix, alpha

    for r in res:
        assert r["info_rc"] == 0
    # the encoder's own file
    n, npx = res[0]["n"], res[0]["w"] * res[0]["h"]
    assert res[0]["rc"] == res[1]["rc"] == n == g["frames"]
    packed = np.load(tmp_path / "first_packed.npy").view(np.uint32).reshape(n, npx)
    _, pix, alpha = frames_of(res[1], "first.npy")
    assert (pix == packed).all(), "frames differ from AGMV_DecodeFramesDev's: %s" % sorted(set(np.argwhere(pix != packed)[:, 0]))[:8]
    if fmt == P.RGBA32:
        assert (alpha == 0xFF).all()
    # the reference's files
    for k, which in ((2, "splash"), (3, "fox")):
        assert res[k]["rc"] == res[k]["n"] == gold[which]["n"]
        _, pix, alpha = frames_of(res[k], which + ".npy")
        bad = [f for f in range(pix.shape[0]) if pix_sha(pix[f]) != gold[which]["pix_sha"][f]]
        assert not bad, "%s: frames %s differ from the goldens" % (which, bad[:8])
        if fmt == P.RGBA32:
            assert (alpha == 0xFF).all()
    # cap_frames = 11: every later byte keeps its 0xA5
    assert res[4]["rc"] == 11 and res[4]["n"] == g["frames"] > 11
    raw, pix, _ = frames_of(res[4], "cap.npy")
    assert (pix[:11] == packed[:11]).all()
    assert (raw[11:] == 0xA5).all(), "frames behind cap_frames were written"


def test_unknown_format_is_refused_before_a_file_exists(tmp_path):
    ok = ["x.agmv", 2, 8, 16, 16, 3, 3, 1, 2]
    bad = [ok[:1] + [0] + ok[2:], ok[:1] + [6] + ok[2:], ok[:1] + [-1] + ok[2:]]
    res = run_child(tmp_path, {"batch": 8, "bad": bad})
    assert res["bad_rc"] == [-1, -1, -1]
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".agmv")]


def test_seq_infers_the_format_and_returns_the_tensor_of_the_format(tmp_path):
    g, frames = golden_of(FIRST)
    np.save(tmp_path / "frames.npy", frames)
    res = run_child(tmp_path, {"batch": 8}, {"AGMV_BATCH_FRAMES": "8"}, SEQ_CHILD)
    for name in ("hwc.agmv", "chw.agmv"):
        check_file(open(tmp_path / name, "rb").read(), g)
    n = g["frames"]
    assert res["frames"] == n and res["packed"] == ["torch.int32", [n, 128, 160]]
    assert res["rgb24"] == ["torch.uint8", [n, 128, 160, 3], True]
    assert res["rgb8p"] == ["torch.uint8", [n, 3, 128, 160], True]
    assert res["rgba32"] == ["torch.uint8", [n, 128, 160, 4], True]
