"""Whole files with sound: libagmv_amd.encode_frames(..., audio=, sample_rate=), the BMP drivers on an object that holds a track,
the files the compiled reference's drivers wrote for the same track (tests/golden/audio/ref_*.agmv, recorded by
tests/golden/make_golden_audio.py like the other goldens of this suite), and libagmv_amd.decode_audio.  The clip is 16 frames of 32 x 32 cut from the
golden clip.  Three files must be the same bytes: the one from the int16 tensor in GPU memory, the one of this library's BMP driver
with the track set through the setters and AGMV_SyncAudioTrack, and the reference's from that same object.

Two tracks.  LONG is 2500 sample frames of 1 kHz stereo (duration 2).  AGMV_SCHEDULE_PDIFS writes 9 chunks of (u32)(5000 / 11.0f) =
454 codes from it and stays inside the track.  AGMV_SCHEDULE_FULL cannot: the reference divides by end_frame - start_frame = 15
(src/agmv_encode.c:4024) and writes 16 chunks, 16 * 333 = 5328 codes of a 5000-sample track, the last 328 from memory it never
set.  No track of a whole second at 1 kHz fits 16 frames that way (size * 16 <= audio_size needs audio_size < 15 * 15).  So FULL
is run with both: SHORT, 112 sample frames of 100 Hz stereo (duration 1, 16 * 14 = 224 = audio_size), where the reference stays
inside its buffers and the files must be equal byte for byte; and LONG, where they must be equal except for those last 328
codes, which are zeros in this library's files.  Both conditions are asserted from the files.

The drivers keep process-wide state and free the caller's object, so this library's runs share one child process.  The reference's
files are recorded, not written next to this library's: its drivers read memory they never set (the bitstream buffer CreateAGMV
does not clear, behind the longest frame so far; the recorder zeroes it), and run live beside this test on another machine they
wrote other bytes than on the machine that built them.  LOW quality: its palette build sorts the whole histogram.  Needs an MI355X."""
import functools
import os
import tempfile
import textwrap

import numpy as np
import pytest

import audio_cases as A
import children as K
import dither_cases as D
import hostlib as H

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio")

T, W, HH, Y0, X0 = 16, 32, 32, 96, 128
FULL, PDIFS, ADAPTIVE = 1, 2, 3
LONG, SHORT = (2500, 1000), (112, 100)              # (sample frames, rate) of the two stereo tracks
# (name, schedule, opt, compression, track): a 512-colour and a 256-colour opt, LZSS (1) and LZ77 (2)
CASES = [("pdifs_3_lzss", PDIFS, 3, 1, "long"), ("pdifs_2_lz77", PDIFS, 2, 2, "long"), ("full_3_lzss", FULL, 3, 1, "short"), ("full_2_lz77", FULL, 2, 2, "short"),
         ("full_3_lzss_long", FULL, 3, 1, "long")]

# both children: an AGMV object of library L with the track `pcm` (int16 / uint8 [n, ch]) through a BMP driver
DRIVE = textwrap.dedent("""
    import ctypes as C, json, sys
    import numpy as np
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"]); sys.path.insert(0, job["tests"])
    import audio_cases as A

    def drive(L, name, schedule, opt, comp, pcm, rate):
        A.bind(L)
        a = L.CreateAGMV(job["T"], job["W"], job["H"], 24)
        t = A.Track(a)
        t.atsample(None); t.satsample(None)
        # the reference's CreateAGMV does not clear its bitstream buffer, and its LZ77 reads the byte behind a frame's stream there
        # (src/agmv_encode.c:222): zero it, as tests/test_capi_hotpath.py does, so that the longest frame so far reads a 0
        bs = C.c_void_p.from_address(a + 4192).value
        C.memset(C.c_void_p.from_address(bs).value, 0, C.c_ulong.from_address(bs + 8).value)
        if pcm is not None:
            A.set_track(L, A.libc(), a, pcm, rate)
        (L.AGMV_EncodeFullAGMV if schedule == 1 else L.AGMV_EncodeAGMV)(a, name.encode(), b"fr", b"f", 1, 1, job["T"], job["W"], job["H"], 24, opt, 3, comp)

    tracks = {"long": (np.load("long.npy"), job["long_rate"]), "short": (np.load("short.npy"), job["short_rate"])}
    pcm8 = np.load("pcm8.npy")
""")

OURS_CHILD = DRIVE + textwrap.dedent("""
    import torch
    import libagmv_amd
    from libagmv_amd import seq
    L = seq.load_library()
    frames = torch.from_numpy(np.load("frames.npy").view(np.int32)).cuda()
    res = {}
    for name, schedule, opt, comp, track in job["cases"]:
        pcm, rate = tracks[track]
        kw = dict(opt=opt, quality=3, compression=comp, schedule=schedule)
        libagmv_amd.encode_frames("dev_%s.agmv" % name, frames, audio=torch.from_numpy(pcm).cuda(), sample_rate=rate, **kw)
        libagmv_amd.encode_frames("silent_%s.agmv" % name, frames, **kw)              # the track was consumed: silent again
        drive(L, "bmp_%s.agmv" % name, schedule, opt, comp, pcm, rate)
        drive(L, "bmpsilent_%s.agmv" % name, schedule, opt, comp, None, 0)
    pcm, rate = tracks["long"]
    kw = dict(opt=3, quality=3, compression=1, schedule=2)
    x = np.load("float.npy")
    libagmv_amd.encode_frames("dev_f32.agmv", frames, audio=torch.from_numpy(x).cuda(), sample_rate=rate, **kw)
    libagmv_amd.encode_frames("dev_f32_as_s16.agmv", frames, audio=torch.from_numpy(np.ascontiguousarray(A.from_f32(x).view(np.int16).T)).cuda(), sample_rate=rate, **kw)
    libagmv_amd.encode_frames("dev_u8.agmv", frames, audio=torch.from_numpy(pcm8).cuda(), sample_rate=rate, **kw)

    # ADAPTIVE with a track: refused, no file; and the refused track does not stick to the next call
    try:
        libagmv_amd.encode_frames("adaptive.agmv", frames, audio=torch.from_numpy(pcm).cuda(), sample_rate=rate, opt=3, quality=3, schedule=3)
        res["adaptive"] = "encoded"
    except ValueError as e:
        res["adaptive"] = str(e)
    L.AGMV_SetAudioDev(torch.from_numpy(pcm).cuda().data_ptr(), 1, len(pcm), rate, 2)
    res["adaptive_rc"] = L.AGMV_EncodeFramesFmtDev(b"adaptive2.agmv", frames.data_ptr(), 1, job["T"], job["W"], job["H"], 24, 3, 3, 1, 3)
    libagmv_amd.encode_frames("after_refusal.agmv", frames, **kw)
    for bad in ({"audio": torch.from_numpy(pcm[:900].copy()).cuda(), "sample_rate": rate}, {"audio": torch.from_numpy(pcm).cuda()},
                {"audio": torch.from_numpy(pcm), "sample_rate": rate}, {"audio": torch.from_numpy(pcm).cuda()[:, :1], "sample_rate": rate},
                {"audio": torch.from_numpy(pcm.astype(np.int32)).cuda(), "sample_rate": rate}, {"sample_rate": rate}):
        try:
            libagmv_amd.encode_frames("bad.agmv", frames, **bad, **kw)
            res.setdefault("accepted", []).append(sorted(bad))
        except ValueError:
            pass

    # the decoder: every file of a case in the layouts its track allows, whole and capped; both goldens
    def dec(path, out, fmt, cap=None):
        t, info = libagmv_amd.decode_audio(path, fmt, cap_samples=cap)
        a = t.cpu().numpy()
        np.save(out, a.view(np.uint32) if fmt == "f32p" else a)
        res.setdefault("info", {})[out] = [int(info.total_audio_duration), int(info.sample_rate), int(info.audio_size), int(info.number_of_channels), int(info.bits_per_sample)]
    for name, _, _, _, _ in job["cases"]:
        for fmt in ("s16", "f32p"):
            dec("dev_%s.agmv" % name, "dec_%s_%s.npy" % (name, fmt), fmt)
    dec("dev_pdifs_3_lzss.agmv", "dec_cap_s16.npy", "s16", 1001)
    dec("dev_pdifs_3_lzss.agmv", "dec_cap_f32p.npy", "f32p", 1001)
    dec("dev_u8.agmv", "dec_u8.npy", "u8")
    dec("dev_u8.agmv", "dec_cap_u8.npy", "u8", 333)
    dec("silent_pdifs_3_lzss.agmv", "dec_silent.npy", "s16")
    for g in ("fox", "splash"):
        for fmt in ("s16", "f32p"):
            dec(job[g], "dec_%s_%s.npy" % (g, fmt), fmt)
        dec(job[g], "dec_%s_cap.npy" % g, "s16", 100001)
    for fmt, path in (("u8", "dev_pdifs_3_lzss.agmv"), ("s16", "dev_u8.agmv"), ("f32p", "dev_u8.agmv")):
        try:
            libagmv_amd.decode_audio(path, fmt)
            res.setdefault("decoded_wrong_depth", []).append(fmt)
        except RuntimeError:
            pass
    # the video of a file with sound is the video of the file without
    a, _ = libagmv_amd.decode_frames("dev_pdifs_3_lzss.agmv")
    b, _ = libagmv_amd.decode_frames("silent_pdifs_3_lzss.agmv")
    res["same_video"] = bool(a.shape == b.shape and (a == b).all()) and int(a.shape[0])
    print(json.dumps(res))
""")


def clip():
    return np.ascontiguousarray(D.fox()[0][:T, Y0:Y0 + HH, X0:X0 + W])


def tracks():
    long_, short = A.tone(LONG[0], 2, LONG[1]), A.tone(SHORT[0], 2, SHORT[1], seed=6)
    pcm8 = ((long_.astype(np.int32) >> 8) + 128).astype(np.uint8)
    x = np.random.default_rng(12).uniform(-1.02, 1.02, (2, LONG[0])).astype(np.float32)
    return long_, short, pcm8, x


@functools.lru_cache(maxsize=None)
def files():
    """-> (the child's answer, {file name: bytes}, the reference's recorded files included, {name: decoded array}); runs once"""
    import torch  # noqa: F401  (torch's HIP runtime first, as in libagmv_amd.seq)
    H.lib()
    frames = clip()
    long_, short, pcm8, x = tracks()
    job = {"T": T, "W": W, "H": HH, "cases": CASES, "long_rate": LONG[1], "short_rate": SHORT[1], "fox": A.FOXLOGO, "splash": A.SPLASH}
    with tempfile.TemporaryDirectory() as d:
        os.mkdir(os.path.join(d, "fr"))
        for t in range(1, T + 1):
            H.write_bmp(os.path.join(d, "fr", "f%d.bmp" % t), frames[t - 1])
        for name, a in (("frames", frames), ("long", long_), ("short", short), ("pcm8", pcm8), ("float", x)):
            np.save(os.path.join(d, name + ".npy"), a)
        res = K.run_child(d, OURS_CHILD, job, {"AGMV_DITHER": None, "AGMV_PALETTE_REFINE": None, "AGMV_TRACE": None}, prelude="")
        data = {f: open(os.path.join(d, f), "rb").read() for f in os.listdir(d) if f.endswith(".agmv")}
        data.update({f: open(os.path.join(GOLDEN, f), "rb").read() for f in os.listdir(GOLDEN) if f.endswith(".agmv")})
        dec = {f[4:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.startswith("dec_")}
    return res, data, dec


def track_of(name):
    long_, short, _, _ = tracks()
    return (long_, LONG[1]) if name == "long" else (short, SHORT[1])


def expected_codes(data, codes):
    """what the chunks of the file `data` hold of a track's `codes`: size codes per chunk from a running start, zeros past the end"""
    sizes = [s for s, _ in A.file_chunks(data)]
    want = np.zeros(sum(sizes), np.uint8)
    n = min(len(want), len(codes))
    want[:n] = codes[:n]
    return sizes, want


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_three_files_are_the_same_bytes(case):
    name, schedule, opt, comp, track = case
    _, data, _ = files()
    dev, bmp, ref = data["dev_%s.agmv" % name], data["bmp_%s.agmv" % name], data["ref_%s.agmv" % name]
    pcm, rate = track_of(track)
    frames, duration, frate, size, channels, bits = A.header_audio(dev)
    assert (duration, frate, size, channels, bits) == (len(pcm) // rate, rate, pcm.size, 2, 16) and duration >= 1
    sizes, want = expected_codes(dev, A.compand(pcm.view(np.uint16)).reshape(-1))
    assert len(sizes) == frames and len(set(sizes)) == 1 and sizes[0] == A.chunk_size(size, 11 if schedule == PDIFS else T - 1)
    assert (A.file_codes(dev) == want).all()                                      # the file holds the statement's codes
    assert dev == bmp
    inside = sizes[0] * len(sizes) <= size
    assert inside == (track == "short" or schedule == PDIFS)                      # where the reference stays inside its own buffers ...
    if inside:
        assert dev == ref                                                         # ... its file is this one, byte for byte
    else:
        # ... and where it does not, the files agree in everything but the codes past audio_size, which it read from memory it never set
        assert len(ref) == len(dev)
        past = sizes[0] * len(sizes) - size
        mine, theirs = A.file_codes(dev), A.file_codes(ref)
        assert (mine[:size] == theirs[:size]).all() and not mine[size:].any() and len(mine) - size == past
        diff = np.flatnonzero(np.frombuffer(dev, np.uint8) != np.frombuffer(ref, np.uint8))
        assert len(diff) <= past                                                  # nothing else differs
    assert data["silent_%s.agmv" % name] == data["bmpsilent_%s.agmv" % name] and A.header_audio(data["silent_%s.agmv" % name])[1:4] == (0, 0, 0)


def test_float_tensor_gives_the_file_of_its_int16_conversion():
    _, data, _ = files()
    _, _, _, x = tracks()
    assert data["dev_f32.agmv"] == data["dev_f32_as_s16.agmv"]
    assert (A.file_codes(data["dev_f32.agmv"]) == expected_codes(data["dev_f32.agmv"], A.compand(A.from_f32(x)).T.reshape(-1))[1]).all()


def test_uint8_tensor_gives_the_reference_eight_bit_file():
    _, data, _ = files()
    _, _, pcm8, _ = tracks()
    dev = data["dev_u8.agmv"]
    assert A.header_audio(dev)[1:] == (2, LONG[1], pcm8.size, 2, 8)
    sizes, want = expected_codes(dev, pcm8.reshape(-1))
    assert sizes[0] * len(sizes) <= pcm8.size and (A.file_codes(dev) == want).all()
    assert dev == data["ref_u8.agmv"]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_decode_audio_is_the_expansion_of_the_chunks(case):
    res, data, dec = files()
    name, track = case[0], case[4]
    pcm, rate = track_of(track)
    codes = A.file_codes(data["dev_%s.agmv" % name])[:pcm.size]                   # at most audio_size samples
    codes = codes[:len(codes) // 2 * 2].reshape(-1, 2)
    s16, f32p = dec["%s_s16" % name], dec["%s_f32p" % name]
    assert s16.dtype == np.int16 and s16.shape == codes.shape and (s16.view(np.uint16) == A.expand(codes)).all()
    assert f32p.shape == codes.shape[::-1] and (f32p == A.to_f32(A.expand(codes)).T.view(np.uint32)).all()
    assert res["info"]["dec_%s_s16.npy" % name] == [len(pcm) // rate, rate, pcm.size, 2, 16]
    assert int(np.abs(s16.view(np.uint16).astype(np.int64) - pcm[:len(s16)].view(np.uint16).astype(np.int64)).max()) <= 256      # the codec's worst error


def test_decode_audio_capped_eight_bit_and_silent():
    res, data, dec = files()
    codes = A.file_codes(data["dev_pdifs_3_lzss.agmv"])
    assert dec["cap_s16"].shape == (500, 2) and (dec["cap_s16"].view(np.uint16).reshape(-1) == A.expand(codes[:1000])).all()      # 1001 rounds down to whole sample frames
    assert dec["cap_f32p"].shape == (2, 500) and (dec["cap_f32p"] == A.to_f32(A.expand(codes[:1000].reshape(-1, 2))).T.view(np.uint32)).all()
    u8 = A.file_codes(data["dev_u8.agmv"])
    assert dec["u8"].dtype == np.uint8 and (dec["u8"].reshape(-1) == u8).all() and len(u8) > 4000
    assert dec["cap_u8"].shape == (166, 2) and (dec["cap_u8"].reshape(-1) == u8[:332]).all()
    assert dec["silent"].shape == (0, 1) or dec["silent"].size == 0
    assert "decoded_wrong_depth" not in res


@pytest.mark.parametrize("which,path", (("fox", A.FOXLOGO), ("splash", A.SPLASH)), ids=("fox", "splash"))
def test_decode_audio_of_the_golden_files(which, path):
    _, _, dec = files()
    data = open(path, "rb").read()
    _, _, _, size, channels, bits = A.header_audio(data)
    codes = A.file_codes(data)[:size]
    codes = codes[:len(codes) // channels * channels].reshape(-1, channels)
    assert bits == 16 and channels == 2 and len(codes) > 400000
    assert (dec["%s_s16" % which].view(np.uint16) == A.expand(codes)).all() and dec["%s_s16" % which].shape == codes.shape
    assert (dec["%s_f32p" % which] == A.to_f32(A.expand(codes)).T.view(np.uint32)).all()
    assert dec["%s_cap" % which].shape == (50000, 2) and (dec["%s_cap" % which].view(np.uint16) == A.expand(codes[:50000])).all()


def test_video_schedule_refusal_and_consumed_track():
    res, data, _ = files()
    assert res["same_video"] == 9                                                 # decode_frames on the file with sound: the same 9 frames
    assert "refused" in res["adaptive"] and res["adaptive_rc"] == -5 and "adaptive.agmv" not in data and "adaptive2.agmv" not in data
    assert data["after_refusal.agmv"] == data["silent_pdifs_3_lzss.agmv"]         # the refused call consumed its track
    assert "accepted" not in res and "bad.agmv" not in data
