"""File level with AGMV_LZ_DEVICE=1 (agmv_pipeline.c: the LZSS stage on the GPU workers): every file golden of
tests/test_gpu_files.py must come out byte-identical, on one device and on two; LZ77 files are unaffected by the knob."""
import hashlib

import pytest

import children as K
import hostlib as H
import synth as S
import test_gpu_files as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", F.CASES)
def test_file_roundtrip_with_device_lzss(golden, tmp_path, monkeypatch, name):
    monkeypatch.setenv("AGMV_LZ_DEVICE", "1")
    F.test_file_roundtrip_matches_reference(golden, tmp_path, name)


def test_foxlogo_212_through_encodevideo_with_device_lzss(golden_dir, tmp_path, monkeypatch):
    monkeypatch.setenv("AGMV_LZ_DEVICE", "1")
    F.test_foxlogo_212_through_encodevideo(golden_dir, tmp_path)


def test_two_devices_with_device_lzss(golden, tmp_path, monkeypatch):
    monkeypatch.setenv("AGMV_LZ_DEVICE", "1")
    F.test_two_devices_write_the_same_file(golden, tmp_path)


@pytest.mark.parametrize("name", ["c2_agmv_opt3_low_lzss_320x240", "agmv_opt2_low_lz77_160x128"])
def test_knob_takes_the_device_path_for_lzss_only(golden, tmp_path, name):
    g = golden["files"][name]
    H.lib()
    T, W, Hh = g["T"], g["W"], g["H"]
    (tmp_path / "fr").mkdir()
    for t in range(1, T + 1):
        H.write_bmp(str(tmp_path / "fr" / ("f%d.bmp" % t)), S.synth_frame(W, Hh, t))
    r = K.drive_child(tmp_path, g["driver"], T, W, Hh, g["opt"], g["quality"], g["compression"], 8, decode=True,
                      env=dict(AGMV_LZ_DEVICE="1", AGMV_TRACE="1"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lz77 = g["compression"] != 1
    assert (b"LZ (host)" if lz77 else b"LZ (device)") in r.stderr, r.stderr.decode()[-2000:]
    assert hashlib.sha256(open(tmp_path / "out.agmv", "rb").read()).hexdigest() == g["file_sha"]
