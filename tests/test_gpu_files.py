"""File level, through the libagmv-compatible C API of libagmv_amd/libagmv.so (host C + GPU hot path):
synthetic BMP clips -> AGMV_Encode{AGMV,FullAGMV,Video} -> .agmv -> AGMV_DecodeAGMV -> BMPs, byte-identical
to what the compiled reference produced for the same inputs (hashes in tests/golden/golden.json, made by
tests/golden/make_golden.py).  Each case runs in a child process because the drivers write into the CWD and,
like the reference's, free the caller's AGMV object.  Needs an MI355X."""
import hashlib
import os
import subprocess

import pytest

import children as K
import hostlib as H
import synth as S

pytestmark = pytest.mark.gpu

CASES = ["agmv_opt3_low_lzss_160x128", "agmv_opt1_mid_lzss_160x128", "agmv_opt2_low_lz77_160x128", "full_opt3_high_lzss_160x128",
         "agmv_gba1_low_lzss_320x240", "agmv_nds_low_lzss_320x240", "video_opt3_low_lzss_160x128",
         "c2_agmv_opt3_low_lzss_320x240",
         # BASELINE.json configs 4 / 5 in shape (tests/golden/make_golden_large.py): a 1080p source through the GBA scaler
         # (121x81 read as 120x80, heavy PDIFS) and a 1280x720 OPT_III clip through AGMV_EncodeAGMV
         "c4_agmv_gba1_low_lzss_1920x1080", "c5_agmv_opt3_low_lzss_1280x720",
         # config 4 at 256 source frames of 1080p (tests/golden/make_golden_r3.py): 127 encoded GBA frames, 1.6 GB of BMPs
         "c4_256_agmv_gba1_low_lzss_1920x1080",
         # config 5's shape at 48 source frames of 1280x720 (33 encoded frames; the reference's own LZSS needs ~10 s per frame)
         "c5_48_agmv_opt3_low_lzss_1280x720"]
# BASELINE.json config 4 at its STATED size: 1024 source frames of 1920x1080 through AGMV_EncodeAGMV / OPT_GBA_I -> 510 encoded
# 120x80 frames (golden made with tests/golden/make_golden.py's file_goldens on that case; 11 minutes of the reference here).
# 6.4 GB of BMP files and ~3 minutes of frame synthesis: opt-in (AGMV_BIG_CASES=1); profiles/r03/README.md records the run.
if os.environ.get("AGMV_BIG_CASES"):
    CASES.append("c4_1024_agmv_gba1_low_lzss_1920x1080")


@pytest.mark.parametrize("name", CASES)
def test_file_roundtrip_matches_reference(golden, tmp_path, name):
    g = golden["files"][name]
    H.lib()
    T, W, Hh = g["T"], g["W"], g["H"]
    (tmp_path / "fr").mkdir()
    for t in range(1, T + 1):
        H.write_bmp(str(tmp_path / "fr" / ("f%d.bmp" % t)), S.synth_frame(W, Hh, t))
    batch = 8 if T < 100 else 64          # small batches: several GPU batches + decoder state hand-over per file
    r = K.drive_child(tmp_path, g["driver"], T, W, Hh, g["opt"], g["quality"], g["compression"], batch, decode=True)
    # (the reference itself crashes in DestroyAGMV after exporting the last frame when driven this way -- its decoder
    #  frees the uninitialised agmv->iframe_entries, src/agmv_decode.c:532,644 -- so golden decode_rc is not compared)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    data = open(tmp_path / "out.agmv", "rb").read()
    assert int.from_bytes(data[4:8], "little") == g["frames"]
    assert int.from_bytes(data[18:22], "little") == g["fps_field"]
    assert len(data) == g["file_len"]
    assert hashlib.sha256(data).hexdigest() == g["file_sha"], "the .agmv file differs from the reference's"
    h = hashlib.sha256()
    for k in range(1, g["frames"] + 1):
        h.update(open(tmp_path / ("quick_export_%d.bmp" % k), "rb").read())
    if g["decode_trusted"]:
        assert h.hexdigest() == g["decoded_bmps_sha"], "decoded BMPs differ from the reference's"
    if g["opt"] in (5, 6, 7):
        assert os.path.exists(tmp_path / "GBA_GEN_AGMV.h")


def test_two_devices_write_the_same_file(golden, tmp_path):
    """AGMV_DEVICES=2 (agmv_pipeline.c: batches round-robin over the devices' worker pairs, chunks written in frame order, a
    palette table per device): config 2 in batches of 8 frames must give the one-device file.  On a one-GPU box both
    "devices" are card 0 (AGMV_DEVICES_OVERSUBSCRIBE=1); on a node with two cards they are two cards."""
    g = golden["files"]["c2_agmv_opt3_low_lzss_320x240"]
    H.lib()
    T, W, Hh = g["T"], g["W"], g["H"]
    (tmp_path / "fr").mkdir()
    for t in range(1, T + 1):
        H.write_bmp(str(tmp_path / "fr" / ("f%d.bmp" % t)), S.synth_frame(W, Hh, t))
    env = dict(AGMV_DEVICES="2", AGMV_DEVICES_OVERSUBSCRIBE="1", AGMV_TRACE="1")
    r = K.drive_child(tmp_path, g["driver"], T, W, Hh, g["opt"], g["quality"], g["compression"], 8, decode=True, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"4 GPU workers" in r.stderr, r.stderr.decode()[-2000:]      # two worker pairs were really opened
    data = open(tmp_path / "out.agmv", "rb").read()
    assert hashlib.sha256(data).hexdigest() == g["file_sha"], "the two-device .agmv file differs from the reference's"


def test_foxlogo_212_through_encodevideo(golden_dir, tmp_path):
    """SURVEY.md section 4's real-content known answers: the reference's AGMV_EncodeVideo over its own 212 foxlogo frames
    (OPT_III, LOW quality, LZSS) writes a 156-frame file with sha ad91dc37..., which decodes to BMPs with sha ae2330f7....
    The frames travel as pixels (tests/golden/foxlogo212.npz); the hashes are the compiled reference's."""
    import json
    import numpy as np
    g = json.load(open(os.path.join(golden_dir, "golden_r3.json")))["encodevideo_212"]
    assert g["file_sha"].startswith("ad91dc37") and g["decoded_bmps_sha"].startswith("ae2330f7")
    H.lib()
    rgb = np.load(os.path.join(golden_dir, "foxlogo212.npz"))["rgb"].astype(np.uint32)
    frames = rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2]
    (tmp_path / "fr").mkdir()
    for k in range(212):
        H.write_bmp(str(tmp_path / "fr" / ("f%d.bmp" % (k + 1))), frames[k])
    r = K.drive_child(tmp_path, "video", 212, 320, 240, 3, 3, 1, 64, decode=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    data = open(tmp_path / "out.agmv", "rb").read()
    assert len(data) == g["file_len"] and int.from_bytes(data[4:8], "little") == g["frames"] == 156
    assert hashlib.sha256(data).hexdigest() == g["file_sha"], "the .agmv file differs from the reference's"
    h = hashlib.sha256()
    for k in range(1, g["frames"] + 1):
        h.update(open(tmp_path / ("quick_export_%d.bmp" % k), "rb").read())
    assert h.hexdigest() == g["decoded_bmps_sha"], "decoded BMPs differ from the reference's"


def test_foxlogo_through_the_readme_flow(golden_fox, foxlogo, tmp_path):
    """real content through the drop-in API: the first 24 frames of the reference's foxlogo sample -> CreateAGMV +
    AGMV_EncodeAGMV (OPT_III / LOW / LZSS, the README flow) -> AGMV_DecodeAGMV; file and decoded BMPs as the compiled
    reference makes them (tests/golden/make_golden_foxlogo.py)"""
    g = golden_fox["encodeagmv_24"]
    H.lib()
    (tmp_path / "fr").mkdir()
    for k, f in enumerate(foxlogo["frames"]):
        H.write_bmp(str(tmp_path / "fr" / ("f%d.bmp" % (k + 1))), f)
    r = K.drive_child(tmp_path, "agmv", 24, 320, 240, g["opt"], g["quality"], g["compression"], 8, decode=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    data = open(tmp_path / "out.agmv", "rb").read()
    assert (int.from_bytes(data[4:8], "little"), int.from_bytes(data[18:22], "little"), len(data)) == (g["frames"], g["fps_field"], g["file_len"])
    assert hashlib.sha256(data).hexdigest() == g["file_sha"], "the .agmv file differs from the reference's"
    h = hashlib.sha256()
    for k in range(1, g["frames"] + 1):
        h.update(open(tmp_path / ("quick_export_%d.bmp" % k), "rb").read())
    assert h.hexdigest() == g["decoded_bmps_sha"], "decoded BMPs differ from the reference's"


@pytest.mark.parametrize("which", ["FOXLOGO"])
def test_decode_sample_with_audio_chunks_via_c_api(golden_fox, golden_dir, tmp_path, which):
    """AGMV_DecodeAGMV on a stream with AGAC chunks between the frames (audio itself is out of scope: the chunks are skipped)"""
    import numpy as np
    g = golden_fox[which]
    r = K.decode_child(tmp_path, os.path.join(golden_dir, which + ".agmv"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    for k in (1, 2, 40, 64, g["n"]):
        raw = open(tmp_path / ("quick_export_%d.bmp" % k), "rb").read()
        px = np.frombuffer(raw[54:], np.uint8).reshape(-1, 3).astype(np.uint32)
        pix = px[:, 2] << 16 | px[:, 1] << 8 | px[:, 0]
        assert hashlib.sha256(pix.astype(np.uint32).tobytes()).hexdigest() == g["pix_sha"][k - 1], k


def test_decode_reference_sample_file_via_c_api(golden, golden_dir, tmp_path):
    """config 1 through the drop-in API: AGMV_DecodeAGMV(agmv_splash.agmv) -> 119 BMPs whose pixels are the golden ones"""
    import numpy as np
    g = golden["agmv_splash"]
    r = K.decode_child(tmp_path, os.path.join(golden_dir, "agmv_splash.agmv"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    for k in (1, 2, 37, 60, 119):
        raw = open(tmp_path / ("quick_export_%d.bmp" % k), "rb").read()
        px = np.frombuffer(raw[54:], np.uint8).reshape(-1, 3).astype(np.uint32)
        pix = px[:, 2] << 16 | px[:, 1] << 8 | px[:, 0]
        assert hashlib.sha256(pix.astype(np.uint32).tobytes()).hexdigest() == g["pix_sha"][k - 1], k


def test_decode_batches_cut_where_a_chunk_is_not_where_it_was_assumed(golden_dir, tmp_path):
    """The decode driver decompresses the frames of a batch in parallel after locating their chunks as if every bit reader
    stopped right behind its payload, and cuts the batch at the first chunk that was not there.  Files that defeat the
    assumption: the reference's splash file with the csize field of some chunks raised past the next chunk's header (the
    reader stops when usize bytes are out, src/agmv_decode.c:171-198, so the frames are the same).  Decoding with batches of
    8 frames must give the BMPs of decoding frame by frame (batches of one frame locate nothing ahead)."""
    data = bytearray(open(os.path.join(golden_dir, "agmv_splash.agmv"), "rb").read())
    chunks = []
    pos = 0
    while True:
        c = data.find(b"AGFC", pos)
        if c < 0:
            break
        chunks.append(c)
        pos = c + 16 + int.from_bytes(data[c + 12:c + 16], "little")
    assert len(chunks) == 119
    for k in (3, 4, 17, 40, 41, 42, 100):                      # csize now reaches into the chunk after the next one
        c, nxt = chunks[k], chunks[k + 2]
        data[c + 12:c + 16] = (nxt + 40 - (c + 16)).to_bytes(4, "little")
    open(tmp_path / "patched.agmv", "wb").write(bytes(data))
    H.lib()
    sums = []
    for batch in (1, 8):
        d = tmp_path / ("b%d" % batch)
        d.mkdir()
        r = K.decode_child(d, tmp_path / "patched.agmv", batch)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        h = hashlib.sha256()
        names = sorted(f for f in os.listdir(d) if f.startswith("quick_export_"))
        for f in names:                                        # (a reader that runs on past its payload may swallow the next chunk)
            h.update(f.encode())
            h.update(open(d / f, "rb").read())
        sums.append((len(names), h.hexdigest()))
    assert sums[0][0] >= 100 and sums[0] == sums[1]


def test_c_example_runs(tmp_path):
    """examples/encode_decode.c (the reference's README flow) end to end on the GPU"""
    exe = str(tmp_path / "agmv_example")
    H.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["gcc", os.path.join(root, "examples", "encode_decode.c"), "-I" + os.path.join(root, "include"),
                    "-L" + os.path.join(root, "libagmv_amd"), "-lagmv", "-lagmv_hip",
                    "-Wl,-rpath," + os.path.join(root, "libagmv_amd"), "-o", exe], check=True)
    r = subprocess.run([exe], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"NO ERROR" in r.stdout
    data = open(tmp_path / "example.agmv", "rb").read()
    n = int.from_bytes(data[4:8], "little")
    assert n == 18 and os.path.exists(tmp_path / ("quick_export_%d.bmp" % n))


def test_per_frame_file_api_matches_reference(golden, tmp_path):
    """AGMV_EncodeHeader + AGMV_EncodeFrame per frame (8-byte u32 pixels, FILE* protocol) must write the file the
    reference's own AGMV_EncodeFrame writes; then AGMV_DecodeFrameChunk per frame must give the oracle's pixels."""
    import ctypes as C
    import numpy as np
    import oracles as O
    L = H.lib()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    for key, g in golden["per_frame_api"].items():
        opt, comp = int(key[3]), int(key[-1])
        W, Hh, T = g["W"], g["H"], g["T"]
        frames = [S.synth_frame(W, Hh, t) for t in range(T)]
        p0, p1 = S.content_palettes(frames[:4])
        path = str(tmp_path / (key + ".agmv")).encode()
        a = L.CreateAGMV(1, W, Hh, 24)
        L.AGMV_SetOPT(a, opt)
        L.AGMV_SetCompression(a, comp)
        L.AGMV_SetICP0(a, p0.astype(np.uint64))
        L.AGMV_SetICP1(a, p1.astype(np.uint64))
        f = libc.fopen(path, b"wb")
        L.AGMV_EncodeHeader(f, a)
        for fr in frames:
            L.AGMV_EncodeFrame(f, a, np.ascontiguousarray(fr.reshape(-1)).astype(np.uint64))
        libc.fclose(f)
        L.DestroyAGMV(a)
        data = open(path, "rb").read()
        assert len(data) == g["file_len"] and hashlib.sha256(data).hexdigest() == g["file_sha"], key
        # decode frame by frame through the FILE* API; the file header says num_of_frames = 1, so drive the loop by T
        err, info, ofr = O.oracle_decode_file(data[:4] + T.to_bytes(4, "little") + data[8:])
        assert err == 0 and len(ofr) == T
        d = L.CreateAGMV(1, W, Hh, 24)
        f = libc.fopen(path, b"rb")
        assert L.AGMV_DecodeHeader(f, d) == 0
        for t in range(T):
            L.AGMV_FindNextFrameChunk(f)
            assert L.AGMV_DecodeFrameChunk(f, d) == 0
            frame_ptr = C.c_void_p.from_address(d + 4200).value                  # agmv->frame (offset checked against the reference headers)
            img = C.c_void_p.from_address(frame_ptr + 16).value                  # ->img_data, 8 bytes per pixel
            pix = np.ctypeslib.as_array(C.cast(img, C.POINTER(C.c_uint64)), (W * Hh,)).astype(np.uint32)
            assert (pix == ofr[t]["pix"]).all(), (key, t)
        libc.fclose(f)
        L.DestroyAGMV(d)
