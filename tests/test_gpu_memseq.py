"""Sequences from and to frames in GPU memory: AGMV_EncodeFramesDev / AGMV_DecodeFramesDev of libagmv_amd/libagmv.so.

Encode: clips uploaded with agmv_hip_malloc / agmv_hip_memcpy_h2d must become, byte for byte, the files the compiled reference
wrote for BMP files of the same frames (hashes in tests/golden/golden.json and tests/golden/golden_memseq.json).  Decode: the
frames must be the pixels of the BMPs AGMV_DecodeAGMV exports for the same file in the same process, and the reference's where
its decode is trusted.  Each case runs in a child process like tests/test_gpu_files.py (the drivers write into the CWD and keep
process-wide state), in batches of 8 frames so that a file spans several batches.  Needs an MI355X."""
import functools
import hashlib
import json
import os
import struct
import tempfile
import textwrap

import numpy as np
import pytest

import children as K
import hostlib as H
import memseq_cases as MC
import synth as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCHEDULE = {"full": 1, "agmv": 2, "video": 3}

CHILD = textwrap.dedent("""
    L.AGMV_SetBatchFrames(job["batch"])
    res = {}

    if "enc" in job:
        e = job["enc"]
        fr = np.load("frames.npy")
        n, h, w = fr.shape
        d = upload(fr)
        res["enc_rc"] = L.AGMV_EncodeFramesDev(b"out.agmv", d, n, w, h, 24, e["opt"], e["quality"], e["compression"], e["schedule"])
        free(d)
    if "bmp_video" in job:                 # the existing BMP driver over fr/f<t>.bmp of the same frames
        e = job["bmp_video"]
        L.AGMV_EncodeVideo(b"bmp.agmv", b"fr", b"f", 1, 1, e["T"], e["W"], e["H"], 24, e["opt"], e["quality"], e["compression"])
    if "bad_args" in job:                  # [filename or None, null pointer?, n, w, h, opt, quality, compression, schedule]
        fr = np.zeros((8, 16, 16), np.uint32)
        d = upload(fr)
        res["bad_rc"] = [L.AGMV_EncodeFramesDev(a[0].encode() if a[0] else None, None if a[1] else d, *a[2:5], 24, *a[5:]) for a in job["bad_args"]]
        free(d)
    if "dec" in job:
        e = job["dec"]
        path = e["path"].encode()
        info = INFO()
        res["info_rc"] = L.AGMV_DecodeFramesDev(path, None, 0, C.byref(info))
        n, w, h = info.number_of_frames, info.width, info.height
        res["info"] = [n, w, h, info.version]
        d = poisoned(4 * n * h * w)                                     # what a frame that is not decoded keeps
        res["dec_rc"] = L.AGMV_DecodeFramesDev(path, d, e.get("cap", n), None)
        np.save("dec.npy", download(d, 4 * n * h * w).view(np.uint32).reshape(n, h, w))
        free(d)
        if e.get("bmps"):
            res["bmp_rc"] = L.AGMV_DecodeAGMV(path, 1, 1)
    print(json.dumps(res))
""")


def run_child(cwd, job, env=None):
    return K.run_child(cwd, CHILD, job, env)


@functools.lru_cache(maxsize=None)
def clip(W, Hh, T):
    """frames 1..T of the canonical clip through the library's C statement of it (tests/test_hostlib.py holds it to tests/synth.py)"""
    L = H.lib()
    out = np.empty((T, Hh, W), np.uint32)
    for t in range(1, T + 1):
        L.AGMV_SynthFrame(out[t - 1].reshape(-1), W, Hh, t, S.DEFAULT_SEED)
    out.setflags(write=False)
    return out


def bmp_file_bytes(frame):
    """the 24-bit BMP the library exports for a frame (libagmv_amd/csrc/agmv_bmp.c: rows in file order, B,G,R, row padding W % 4)"""
    h, w = frame.shape
    hdr = struct.pack("<HIHHIIIIHHIIIIII", 0x4d42, 54 + w * h * 3, 0, 0, 54, 40, w, h, 1, 24, 0, w * h * 3, 0, 0, 0, 0)
    rows = np.zeros((h, w * 3 + w % 4), np.uint8)
    rows[:, 0:w * 3:3] = frame & 255
    rows[:, 1:w * 3:3] = (frame >> 8) & 255
    rows[:, 2:w * 3:3] = (frame >> 16) & 255
    return hdr + rows.tobytes()


def exported_pixels(d, k, w, h):
    raw = open(os.path.join(d, "quick_export_%d.bmp" % k), "rb").read()
    px = np.frombuffer(raw[54:], np.uint8).reshape(h, -1)[:, :w * 3].reshape(h, w, 3).astype(np.uint32)
    return px[..., 2] << 16 | px[..., 1] << 8 | px[..., 0]


def check_decode(d, res, frames):
    """the frames AGMV_DecodeFramesDev gave against the BMPs AGMV_DecodeAGMV exported in the same child"""
    n, w, h, _ = res["info"]
    assert res["info_rc"] == 0 and res["dec_rc"] == n == frames and res["bmp_rc"] == 0
    dec = np.load(os.path.join(d, "dec.npy"))
    for k in range(n):
        assert (dec[k] == exported_pixels(d, k + 1, w, h)).all(), "frame %d differs from quick_export_%d.bmp" % (k, k + 1)
    return dec


@functools.lru_cache(maxsize=None)
def golden_case(name, lz_device=False):
    """clip of golden.json files[name] -> AGMV_EncodeFramesDev -> AGMV_DecodeFramesDev + AGMV_DecodeAGMV in one child; run once"""
    g = json.load(open(os.path.join(GOLDEN, "golden.json")))["files"][name]
    env = {"AGMV_LZ_DEVICE": "1", "AGMV_LZ77_DEVICE": "1", "AGMV_LZ_DECODE_DEVICE": "1"} if lz_device else {}
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "frames.npy"), clip(g["W"], g["H"], g["T"]))
        res = run_child(d, {"batch": 8, "enc": dict(g, schedule=SCHEDULE[g["driver"]]), "dec": {"path": "out.agmv", "bmps": True}}, env)
        assert res["enc_rc"] == 0
        data = open(os.path.join(d, "out.agmv"), "rb").read()
        assert not os.path.exists(os.path.join(d, "GBA_GEN_AGMV.h"))
        dec = check_decode(d, res, g["frames"])
    return g, data, dec


ENCODE_CASES = ["agmv_opt3_low_lzss_160x128", "agmv_opt1_mid_lzss_160x128", "agmv_opt2_low_lz77_160x128", "full_opt3_high_lzss_160x128",
                "video_opt3_low_lzss_160x128", "agmv_gba1_low_lzss_320x240", "agmv_nds_low_lzss_320x240",
                "c5_agmv_opt3_low_lzss_1280x720", "c4_agmv_gba1_low_lzss_1920x1080"]
UNSCALED = [n for n in ENCODE_CASES if "gba" not in n and "nds" not in n]


def check_file(data, g):
    assert int.from_bytes(data[4:8], "little") == g["frames"]
    assert int.from_bytes(data[18:22], "little") == g["fps_field"]
    assert len(data) == g["file_len"]
    assert hashlib.sha256(data).hexdigest() == g["file_sha"], "the .agmv file differs from the reference's"


@pytest.mark.parametrize("name", ENCODE_CASES)
def test_encode_from_device_frames_matches_reference(name):
    g, data, _ = golden_case(name)
    check_file(data, g)


@pytest.mark.parametrize("name", UNSCALED)
def test_decode_to_device_frames_matches_reference(name):
    """(equality with the BMPs of AGMV_DecodeAGMV in the same child is asserted inside golden_case)"""
    g, _, dec = golden_case(name)
    assert dec.shape[0] == g["frames"]
    if g["decode_trusted"]:
        h = hashlib.sha256()
        for f in dec:
            h.update(bmp_file_bytes(f))
        assert h.hexdigest() == g["decoded_bmps_sha"], "decoded frames differ from the reference's"


@pytest.mark.parametrize("name", ["agmv_opt3_low_lzss_160x128", "agmv_opt2_low_lz77_160x128"])
def test_device_lz_stages_give_the_same_file_and_pixels(name):
    """AGMV_LZ_DEVICE / AGMV_LZ77_DEVICE on encode and AGMV_LZ_DECODE_DEVICE on decode act on the memory sequences as on the BMP drivers"""
    g, data, dec = golden_case(name, True)
    check_file(data, g)
    assert (dec == golden_case(name)[2]).all()


@pytest.mark.parametrize("name", sorted(MC.MIXED_CASES))
def test_mixed_adaptive_clip_both_sources(name, tmp_path):
    """frame skipping that takes both branches (tests/golden/make_golden_memseq.py): the device source decides from one
    agmv_hip_similarity_dev launch, the BMP source on the host; both must write the reference's file"""
    g = json.load(open(os.path.join(GOLDEN, "golden_memseq.json")))[name]
    assert g["chain"].count(1) >= 2 and g["chain"].count(0) >= 2
    fr = MC.mixed_clip()
    np.save(tmp_path / "frames.npy", fr)
    (tmp_path / "fr").mkdir()
    for t in range(1, g["T"] + 1):
        H.write_bmp(str(tmp_path / "fr" / ("f%d.bmp" % t)), fr[t - 1])
    res = run_child(tmp_path, {"batch": 8, "enc": dict(g, schedule=SCHEDULE["video"]), "bmp_video": g})
    assert res["enc_rc"] == 0
    check_file(open(tmp_path / "out.agmv", "rb").read(), g)
    check_file(open(tmp_path / "bmp.agmv", "rb").read(), g)


@pytest.mark.parametrize("which,frames", [("agmv_splash", 119), ("FOXLOGO", None)])
def test_decode_sample_files_to_device_frames(which, frames, tmp_path):
    """the reference's own files: escape frames and stale tails (agmv_splash), AGAC chunks between the frames (FOXLOGO)"""
    res = run_child(tmp_path, {"batch": 8, "dec": {"path": os.path.join(GOLDEN, which + ".agmv"), "bmps": True}})
    dec = check_decode(tmp_path, res, frames or res["info"][0])
    gold = (json.load(open(os.path.join(GOLDEN, "golden.json")))["agmv_splash"] if which == "agmv_splash"
            else json.load(open(os.path.join(GOLDEN, "golden_foxlogo.json")))[which])
    assert dec.shape[0] == gold["n"]
    for k in range(dec.shape[0]):
        assert hashlib.sha256(np.ascontiguousarray(dec[k]).tobytes()).hexdigest() == gold["pix_sha"][k], k


def test_cap_frames_decodes_exactly_that_many(tmp_path):
    g, data, full = golden_case("agmv_opt3_low_lzss_160x128")
    open(tmp_path / "out.agmv", "wb").write(data)
    res = run_child(tmp_path, {"batch": 8, "dec": {"path": "out.agmv", "cap": 11}})
    assert res["dec_rc"] == 11 and res["info"][0] == g["frames"] > 11
    dec = np.load(tmp_path / "dec.npy")
    assert (dec[:11] == full[:11]).all()
    assert (dec[11:] == 0xA5A5A5A5).all(), "frames behind cap_frames were written"


def test_null_destination_fills_info_only(tmp_path):
    g, data, _ = golden_case("agmv_opt3_low_lzss_160x128")
    open(tmp_path / "out.agmv", "wb").write(data)
    res = run_child(tmp_path, {"batch": 8, "dec": {"path": "out.agmv", "cap": 0}})
    assert res["info_rc"] == 0 and res["info"] == [g["frames"], 160, 128, 1]       # (version 1: 512 colours, LZSS)
    assert res["dec_rc"] == 0 and (np.load(tmp_path / "dec.npy") == 0xA5A5A5A5).all()


def test_arguments_that_cannot_be_encoded_are_refused_before_a_file_exists(tmp_path):
    ok = ["x.agmv", 0, 8, 16, 16, 3, 3, 1, 2]
    bad = [[None] + ok[1:],                                      # no filename
           ok[:1] + [1] + ok[2:],                                # NULL frames
           ok[:2] + [3] + ok[3:],                                # light PDIFS reads 4 frames
           ok[:2] + [3] + ok[3:8] + [3],                         # so does the light adaptive form
           ok[:2] + [1, 16, 16, 1, 3, 1, 2],                     # heavy PDIFS reads 2
           ok[:2] + [1, 16, 16, 1, 3, 1, 3],
           ok[:2] + [0, 16, 16, 3, 3, 1, 1],                     # FULL needs a frame
           ok[:2] + [8, 18, 16, 3, 3, 1, 2],                     # width not a multiple of 4, unscaled opt
           ok[:2] + [8, 16, 14, 2, 3, 1, 1]]                     # height
    res = run_child(tmp_path, {"batch": 8, "bad_args": bad})
    assert len(res["bad_rc"]) == len(bad) and all(rc < 0 for rc in res["bad_rc"]), res["bad_rc"]
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".agmv")]
