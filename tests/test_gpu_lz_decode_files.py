"""AGMV_DecodeAGMV with AGMV_LZ_DECODE_DEVICE=1 (the LZ stage on the GPU, agmv_decode_stream) writes the same BMPs as without
it, and the reference's where golden hashes exist: LZSS and LZ77 files written by this library, the reference's splash file
(also with raised csize fields, which cut batches), the sample with audio chunks and a 1080p file of several batches.  Each
decode runs in a child process (the drivers write into the CWD)."""
import hashlib
import os

import numpy as np
import pytest

import children as K
import hostlib as H
import synth as S

pytestmark = pytest.mark.gpu

def decode(path, where, batch, device, trace=False):
    """AGMV_DecodeAGMV in a child; returns (number of BMPs, sha256 over their names and bytes, stderr)"""
    os.makedirs(where, exist_ok=True)
    r = K.decode_child(where, path, batch, {"AGMV_LZ_DECODE_DEVICE": "1" if device else None, "AGMV_TRACE": "1" if trace else None})
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    names = sorted((f for f in os.listdir(where) if f.startswith("quick_export_")), key=lambda f: int(f[13:-4]))
    h = hashlib.sha256()
    for f in names:
        h.update(f.encode())
        h.update(open(os.path.join(where, f), "rb").read())
    return len(names), h.hexdigest(), r.stderr.decode()


def bmp_sha(path):
    raw = open(path, "rb").read()
    px = np.frombuffer(raw[54:], np.uint8).reshape(-1, 3).astype(np.uint32)
    return hashlib.sha256((px[:, 2] << 16 | px[:, 1] << 8 | px[:, 0]).astype(np.uint32).tobytes()).hexdigest()


def encode(tmp_path, drv, T, W, Hh, opt, q, comp):
    H.lib()
    (tmp_path / "fr").mkdir()
    for t in range(1, T + 1):
        H.write_bmp(str(tmp_path / "fr" / ("f%d.bmp" % t)), S.synth_frame(W, Hh, t))
    r = K.drive_child(tmp_path, drv, T, W, Hh, opt, q, comp, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return tmp_path / "out.agmv"


@pytest.mark.parametrize("name", ["agmv_opt3_low_lzss_160x128", "agmv_opt2_low_lz77_160x128", "agmv_gba1_low_lzss_320x240"])
def test_golden_files_decode_the_same_with_the_device_lz_stage(golden, tmp_path, name):
    g = golden["files"][name]
    f = encode(tmp_path, g["driver"], g["T"], g["W"], g["H"], g["opt"], g["quality"], g["compression"])
    assert hashlib.sha256(open(f, "rb").read()).hexdigest() == g["file_sha"]
    host = decode(f, tmp_path / "host", 8, False)
    dev = decode(f, tmp_path / "dev", 8, True, trace=True)
    assert host[:2] == dev[:2] and dev[0] == g["frames"]
    assert "LZ stage device" in dev[2], dev[2][-2000:]
    if g["decode_trusted"]:
        h = hashlib.sha256()
        for k in range(1, g["frames"] + 1):
            h.update(open(tmp_path / "dev" / ("quick_export_%d.bmp" % k), "rb").read())
        assert h.hexdigest() == g["decoded_bmps_sha"]


@pytest.mark.parametrize("shape", [(64, 48, 9, 2), (320, 240, 14, 4), (200, 120, 11, 2)])
def test_lz77_files_of_other_sizes(tmp_path, shape):
    W, Hh, T, opt = shape
    f = encode(tmp_path, "agmv", T, W, Hh, opt, 1, 2)
    assert decode(f, tmp_path / "host", 4, False)[:2] == decode(f, tmp_path / "dev", 4, True)[:2]


def test_reference_splash_file_with_the_golden_pixels(golden, golden_dir, tmp_path):
    g = golden["agmv_splash"]
    n, _, _ = decode(os.path.join(golden_dir, "agmv_splash.agmv"), tmp_path, 16, True)
    assert n == g["n"]
    for k in range(1, n + 1):
        assert bmp_sha(tmp_path / ("quick_export_%d.bmp" % k)) == g["pix_sha"][k - 1], k


def test_sample_with_audio_chunks(golden_fox, golden_dir, tmp_path):
    g = golden_fox["FOXLOGO"]
    n, sha, _ = decode(os.path.join(golden_dir, "FOXLOGO.agmv"), tmp_path / "dev", 32, True)
    assert n == g["n"]
    for k in range(1, n + 1):
        assert bmp_sha(tmp_path / "dev" / ("quick_export_%d.bmp" % k)) == g["pix_sha"][k - 1], k
    assert decode(os.path.join(golden_dir, "FOXLOGO.agmv"), tmp_path / "host", 32, False)[:2] == (n, sha)


def test_raised_csize_fields_cut_batches(golden_dir, tmp_path):
    """the splash file with some csize fields raised past the next chunk's header (as in test_gpu_files.py): the
    readers stop when usize bytes are out, so the batch is cut where a chunk is not where it was assumed"""
    data = bytearray(open(os.path.join(golden_dir, "agmv_splash.agmv"), "rb").read())
    chunks, pos = [], 0
    while True:
        c = data.find(b"AGFC", pos)
        if c < 0:
            break
        chunks.append(c)
        pos = c + 16 + int.from_bytes(data[c + 12:c + 16], "little")
    for k in (3, 4, 17, 40, 41, 42, 100):
        c, nxt = chunks[k], chunks[k + 2]
        data[c + 12:c + 16] = (nxt + 40 - (c + 16)).to_bytes(4, "little")
    f = tmp_path / "patched.agmv"
    f.write_bytes(bytes(data))
    ref = decode(f, tmp_path / "h1", 1, False)
    assert ref[0] >= 100
    for batch in (8, 1):
        assert decode(f, tmp_path / ("d%d" % batch), batch, True)[:2] == ref[:2], batch


def test_1080p_file_of_several_batches(tmp_path):
    f = encode(tmp_path, "agmv", 26, 1920, 1080, 3, 1, 1)
    n = int.from_bytes(open(f, "rb").read()[4:8], "little")             # (OPT_III interpolates: fewer frames than sources)
    host = decode(f, tmp_path / "host", 8, False)
    assert host[0] == n and n > 16
    assert decode(f, tmp_path / "dev", 8, True)[:2] == host[:2]
