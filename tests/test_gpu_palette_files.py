"""Whole files with the refined palette: libagmv_amd.encode_frames(..., palette_refine=n) and AGMV_SetPaletteRefine of
libagmv_amd/libagmv.so.  The golden clip (tests/golden/foxlogo.npz, 24 frames of 320 x 240, every frame coded: AGMV_SCHEDULE_FULL)
at 256 and 512 colours, HIGH and LOW quality: the header's palettes must be the statement's (tests/palette_cases.py: numpy
histogram, AGMV_BuildPalette's pick, numpy refinement, slot map), the decoded clip must be closer to the source than without the
refinement, and with the refinement off the file must be the one AGMV_EncodeFramesFmtDev writes.  A 64 x 48 clip of 8 frames
through the BMP driver and through the rgb24 and nv12 device sources must give one and the same refined file.  The drivers keep
process-wide state, so each group runs in a child process, once.  Needs an MI355X."""
import functools
import os
import tempfile
import textwrap

import children as K
import numpy as np
import pytest

import hostlib as H
import palette_cases as PC
import synth as S
import yuv_cases as Y

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
FULL = 1
RUNS = [(opt, quality) for opt in (PC.OPT_II, PC.OPT_III) for quality in (PC.HIGH, PC.LOW)]
RUN_IDS = ["opt%d-%s" % (o, "high" if q == PC.HIGH else "low") for o, q in RUNS]

# the golden clip: per run the refined file, the plain file through encode_frames and through the library directly, both decoded
FOX_CHILD = textwrap.dedent("""
    import ctypes as C, json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    from libagmv_amd import seq
    src = np.load(job["clip"])["frames"].astype(np.int64)
    fr = torch.from_numpy(src.astype(np.uint32).view(np.int32)).cuda()
    n, h, w = fr.shape

    def sq_err(path):
        out, info = libagmv_amd.decode_frames(path)
        assert info.number_of_frames == n and tuple(out.shape) == (n, h, w)
        d = out.cpu().numpy().view(np.uint32).astype(np.int64)
        return int(sum((((d >> s) & 255) - ((src >> s) & 255)) ** 2 for s in (16, 8, 0)).sum())

    res = {}
    for opt, quality in job["runs"]:
        tag = "%d_%d" % (opt, quality)
        libagmv_amd.encode_frames("refined_%s.agmv" % tag, fr, opt=opt, quality=quality, schedule=1, palette_refine=16)
        libagmv_amd.encode_frames("plain_%s.agmv" % tag, fr, opt=opt, quality=quality, schedule=1)
        rc = seq.load_library().AGMV_EncodeFramesFmtDev(("direct_%s.agmv" % tag).encode(), fr.data_ptr(), 1, n, w, h, 24, opt, quality, 1, 1)
        res[tag] = {"direct_rc": rc, "refined_err": sq_err("refined_%s.agmv" % tag), "plain_err": sq_err("plain_%s.agmv" % tag)}
    print(json.dumps(res))
""")

# the small clip: the BMP driver under AGMV_SetPaletteRefine(8), then encode_frames(palette_refine=8) on three sources, each followed
# by an encode that leaves palette_refine alone -- which must be the plain file again: the knob went back to 0
SMALL_CHILD = textwrap.dedent("""
    import ctypes as C, json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    from libagmv_amd import seq
    L = seq.load_library()
    T, W, Hh, opt, quality = job["T"], job["W"], job["H"], job["opt"], job["quality"]

    def bmp(path, rounds):
        L.AGMV_SetPaletteRefine(rounds)
        L.AGMV_EncodeFullAGMV(L.CreateAGMV(T, W, Hh, 24), path.encode(), b"fr", b"f", 1, 1, T, W, Hh, 24, opt, quality, 1)
        L.AGMV_SetPaletteRefine(0)

    bmp("bmp_refined.agmv", 8)
    bmp("bmp_plain.agmv", 0)
    packed = torch.from_numpy(np.load("frames.npy").view(np.int32)).cuda()
    p = packed.to(torch.int64)
    rgb = torch.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], dim=3).to(torch.uint8).contiguous()
    nv12 = torch.from_numpy(np.load("nv12.npy")).cuda().reshape(T, Hh * 3 // 2, W)
    stands = torch.from_numpy(np.load("nv12_stands_for.npy").view(np.int32)).cuda()
    for name, clip, kw in (("xrgb32", packed, {}), ("rgb24", rgb, {}), ("nv12", nv12, {"fmt": "nv12"}), ("nv12_stands_for", stands, {})):
        libagmv_amd.encode_frames(name + "_refined.agmv", clip, opt=opt, quality=quality, schedule=1, palette_refine=8, **kw)
        libagmv_amd.encode_frames(name + "_after.agmv", clip, opt=opt, quality=quality, schedule=1, **kw)
    print(json.dumps({"ok": True}))
""")


def run_child(cwd, script, job):
    return K.run_child(cwd, script, job, {"AGMV_PALETTE_REFINE": None, "AGMV_TRACE": None}, prelude="")


@functools.lru_cache(maxsize=None)
def fox_files():
    """-> (the child's answer, {file name: bytes}); run once"""
    with tempfile.TemporaryDirectory() as d:
        res = run_child(d, FOX_CHILD, {"clip": os.path.join(TESTS, "golden", "foxlogo.npz"), "runs": RUNS})
        return res, {f: open(os.path.join(d, f), "rb").read() for f in os.listdir(d) if f.endswith(".agmv")}


def header_palettes(data, mode512):
    """the palettes of a file's header (38 bytes of fields, then 256 x R, G, B per palette) as uint32 0x00RRGGBB"""
    def pal(off):
        b = np.frombuffer(data, np.uint8, 768, off).reshape(256, 3).astype(np.uint32)
        return b[:, 0] << 16 | b[:, 1] << 8 | b[:, 2]
    return pal(38), pal(38 + 768) if mode512 else np.zeros(256, np.uint32)


def psnr(sq_err, n_samples):
    return 10 * np.log10(255.0 ** 2 * n_samples / sq_err)


@pytest.mark.parametrize("opt,quality", RUNS, ids=RUN_IDS)
def test_header_palettes_are_the_statements(opt, quality):
    _, files = fox_files()
    mode512 = opt == PC.OPT_III
    _, run = PC.fox_run(quality, 512 if mode512 else 256)           # 16 rounds from the pick over the numpy histogram of the clip
    want0, want1 = PC.slots(run["pal"], mode512)
    got0, got1 = header_palettes(files["refined_%d_%d.agmv" % (opt, quality)], mode512)
    assert (got0 == want0).all(), np.flatnonzero(got0 != want0)[:8]
    assert (got1 == want1).all(), np.flatnonzero(got1 != want1)[:8]
    plain0, plain1 = header_palettes(files["plain_%d_%d.agmv" % (opt, quality)], mode512)
    lib0, lib1 = PC.build_palette(PC.fox_hist(quality), quality, opt)
    assert (plain0 == lib0).all() and (plain1 == (lib1 if mode512 else 0)).all()
    assert (got0 != plain0).any()


@pytest.mark.parametrize("opt,quality", RUNS, ids=RUN_IDS)
def test_decoded_clip_is_closer_to_the_source(opt, quality):
    res, files = fox_files()
    tag = "%d_%d" % (opt, quality)
    r, samples = res[tag], 3 * PC.fox_frames().size
    print("opt %d quality %d: PSNR %.2f dB -> %.2f dB, file %d -> %d bytes" % (opt, quality, psnr(r["plain_err"], samples), psnr(r["refined_err"], samples),
                                                                            len(files["plain_%s.agmv" % tag]), len(files["refined_%s.agmv" % tag])))
    assert r["refined_err"] < r["plain_err"]


@pytest.mark.parametrize("opt,quality", RUNS, ids=RUN_IDS)
def test_refinement_off_changes_nothing(opt, quality):
    res, files = fox_files()
    tag = "%d_%d" % (opt, quality)
    assert res[tag]["direct_rc"] == 0
    assert files["plain_%s.agmv" % tag] == files["direct_%s.agmv" % tag]
    assert files["plain_%s.agmv" % tag] != files["refined_%s.agmv" % tag]


@functools.lru_cache(maxsize=None)
def small_files():
    W, Hh, T, opt, quality = 64, 48, 8, PC.OPT_III, PC.HIGH
    L = H.lib()
    frames = np.empty((T, Hh, W), np.uint32)
    for t in range(1, T + 1):
        L.AGMV_SynthFrame(frames[t - 1].reshape(-1), W, Hh, t, S.DEFAULT_SEED)
    nv12 = Y.from_packed(Y.NV12, frames, W, Hh)
    with tempfile.TemporaryDirectory() as d:
        os.mkdir(os.path.join(d, "fr"))
        for t in range(1, T + 1):
            H.write_bmp(os.path.join(d, "fr", "f%d.bmp" % t), frames[t - 1])
        np.save(os.path.join(d, "frames.npy"), frames)
        np.save(os.path.join(d, "nv12.npy"), nv12)
        np.save(os.path.join(d, "nv12_stands_for.npy"), Y.to_packed(Y.NV12, nv12, W, Hh))
        run_child(d, SMALL_CHILD, {"T": T, "W": W, "H": Hh, "opt": opt, "quality": quality})
        files = {f: open(os.path.join(d, f), "rb").read() for f in os.listdir(d) if f.endswith(".agmv")}
    return frames, opt, quality, files


def test_bmp_driver_under_the_knob_writes_the_refined_file():
    frames, opt, quality, files = small_files()
    assert files["bmp_refined.agmv"] == files["xrgb32_refined.agmv"]
    assert files["bmp_plain.agmv"] == files["xrgb32_after.agmv"] != files["bmp_refined.agmv"]      # ... and the knob went back to 0
    want0, want1, run = PC.refined_palettes(PC.histogram(frames, quality), quality, opt, 8)
    got0, got1 = header_palettes(files["bmp_refined.agmv"], True)
    assert run["rounds"] >= 1 and (got0 == want0).all() and (got1 == want1).all()


def test_rgb24_source_writes_the_same_refined_file():
    _, _, _, files = small_files()
    assert files["rgb24_refined.agmv"] == files["xrgb32_refined.agmv"]
    assert files["rgb24_after.agmv"] == files["bmp_plain.agmv"]


def test_nv12_source_writes_the_file_of_the_clip_it_stands_for():
    _, _, _, files = small_files()
    assert files["nv12_refined.agmv"] == files["nv12_stands_for_refined.agmv"] != files["nv12_after.agmv"]
    assert files["nv12_after.agmv"] == files["nv12_stands_for_after.agmv"]
