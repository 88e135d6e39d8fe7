"""What the memory sequences do before they touch the GPU: the two entry points exist, refuse arguments that cannot be
encoded, read a header into AGMV_INFO, and the scale table of the GBA / NDS opts holds the reference's quirks."""
import ctypes as C
import os
import re

import numpy as np

import hostlib as H

ROOT = H.ROOT


def entry_points():
    L = H.lib()
    from libagmv_amd.seq import AGMV_INFO
    return L, AGMV_INFO


def test_header_declares_the_entry_points_and_the_package_exports_them():
    hdr = open(os.path.join(ROOT, "include", "agmv.h")).read()
    assert re.search(r"\bint AGMV_EncodeFramesDev\(", hdr) and re.search(r"\bint AGMV_DecodeFramesDev\(", hdr)
    assert "AGMV_SCHEDULE_FULL = 0x1, AGMV_SCHEDULE_PDIFS = 0x2, AGMV_SCHEDULE_ADAPTIVE = 0x3" in hdr
    import libagmv_amd
    assert (libagmv_amd.SCHEDULE_FULL, libagmv_amd.SCHEDULE_PDIFS, libagmv_amd.SCHEDULE_ADAPTIVE) == (1, 2, 3)
    assert callable(libagmv_amd.encode_frames) and callable(libagmv_amd.decode_frames)


def test_unencodable_arguments_are_refused_before_the_gpu_is_opened(tmp_path):
    """(the pointer is never read: every one of these returns before the library opens a device)"""
    L, _ = entry_points()
    out = str(tmp_path / "x.agmv").encode()
    d = C.c_void_p(4096)
    ok = [8, 16, 16, 24, 3, 3, 1, 2]                              # n, w, h, fps, opt, quality, compression, schedule
    assert L.AGMV_EncodeFramesDev(None, d, *ok) < 0
    assert L.AGMV_EncodeFramesDev(out, None, *ok) < 0
    for n, opt, schedule in ((3, 3, 2), (3, 2, 3), (3, 8, 2), (1, 1, 2), (1, 4, 3), (1, 5, 2), (0, 3, 1)):
        assert L.AGMV_EncodeFramesDev(out, d, n, 16, 16, 24, opt, 3, 1, schedule) < 0, (n, opt, schedule)
    for w, h in ((18, 16), (16, 14), (0, 16)):
        assert L.AGMV_EncodeFramesDev(out, d, 8, w, h, 24, 3, 3, 1, 2) < 0, (w, h)
    assert L.AGMV_EncodeFramesDev(out, d, 8, 16, 16, 24, 3, 3, 1, 4) < 0       # no such schedule
    assert not os.listdir(tmp_path)


def test_null_destination_reads_the_header_only(golden, golden_dir):
    L, AGMV_INFO = entry_points()
    g = golden["agmv_splash"]
    info = AGMV_INFO()
    assert L.AGMV_DecodeFramesDev(os.path.join(golden_dir, "agmv_splash.agmv").encode(), None, 0, C.byref(info)) == 0
    assert (info.width, info.height, info.number_of_frames, info.version) == (g["w"], g["h"], g["n"], g["version"])
    assert L.AGMV_DecodeFramesDev(os.path.join(golden_dir, "no_such_file.agmv").encode(), None, 0, C.byref(info)) == -2     # FILE_NOT_FOUND_ERR
    assert L.AGMV_DecodeFramesDev(os.path.join(golden_dir, "agmv_spash_header.bin").encode(), None, 0, None) == -1         # old layout


def source_index(sw, sh, scale_w, scale_h, w, h):
    L = H.lib()
    p = L.agmv_source_index(sw, sh, scale_w, scale_h, w, h)
    out = np.ctypeslib.as_array(p, (w * h,)).copy()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(p)
    return out


def restated_index(sw, sh, scale_w, scale_h):
    """numpy float32 statement of the reference's scaler (extern/agidl/src/agidl_imgp_scale.c:262-291 as src/agmv_encode.c:2707-2721
    calls it) followed by the linear read of scale_w * scale_h pixels"""
    f32 = np.float32
    W2, H2 = int(f32(sw) * (f32(scale_w) / f32(sw) + f32(0.001))), int(f32(sh) * (f32(scale_h) / f32(sh) + f32(0.001)))
    k = np.arange(scale_w * scale_h)
    x2 = (f32(sw - 1) / f32(W2) * (k % W2).astype(f32)).astype(np.int64)
    y2 = (f32(sh - 1) / f32(H2) * (k // W2).astype(f32)).astype(np.int64)
    idx = np.where((x2 < sw) & (y2 < sh) & (k < W2 * H2), y2 * sw + x2, 0xFFFFFFFF)
    return (W2, H2), idx.astype(np.uint32)


def test_scale_table_reads_a_121x81_image_as_120x80():
    """a 1920x1080 source scales to 121x81 (the factor is 120 / 1920 + 0.001 in float) and the encoder reads the first 120 * 80
    pixels of that image linearly: entry k of the table is pixel (k % 121, k // 121) of the scaled image"""
    size, exp = restated_index(1920, 1080, 120, 80)
    idx = source_index(1920, 1080, 120, 80, 120, 80)
    assert size == (121, 81) and (idx == exp).all()
    assert idx[120] == 1903 and idx[121] == 13 * 1920             # the 121st column of row 0, then the start of row 1


def test_scale_table_of_other_sources():
    for sw, sh, tw, th in ((320, 240, 120, 80), (320, 240, 128, 96), (100, 100, 128, 96), (121, 81, 120, 80)):
        _, exp = restated_index(sw, sh, tw, th)
        idx = source_index(sw, sh, tw, th, tw, th)
        assert (idx == exp).all(), (sw, sh, tw, th)
        assert idx[idx != 0xFFFFFFFF].max() < sw * sh
