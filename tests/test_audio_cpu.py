"""Audio tracks on the host, without a GPU: the companding of libagmv_amd/libagmv.so against the numpy statement
(tests/audio_cases.py) and against the compiled reference (oracle/_ref/libagmv_ref.so, where it was built), the WAV importer,
the three exporters, the chunk walk over both golden files, AGMV_DecodeAudio, the bounds of the two chunk functions, the exported
symbols and the refusals of AGMV_SetAudioDev (which stores its arguments and opens no device)."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import audio_cases as A
import hostlib as H
import oracles as O

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref is not built")
vp = C.c_void_p


def ours():
    return A.bind(H.lib())


def ref():
    return A.bind(O.ref())


def libs():
    return [("ours", ours())] + ([("reference", ref())] if O.have_ref() else [])


def compress_all(L):
    """AGMV_CompressAudio over the track 0 .. 65535"""
    libc = A.libc()
    a = L.CreateAGMV(1, 4, 4, 1)
    t = A.set_track(L, libc, a, np.arange(65536, dtype=np.uint16).reshape(-1, 1), 1000)
    t.atsample(libc.calloc(65536, 1))
    L.AGMV_CompressAudio(a)
    codes = A.as_array(t.atsample(), 65536, np.uint8)
    L.DestroyAGMV(a)
    return codes


def test_the_statement_has_the_properties_measured_on_the_reference():
    s = np.arange(65536)
    codes = A.compand(s)
    assert int((codes & 1).sum()) == 36728
    assert int(np.abs(A.expand(codes).astype(np.int64) - s).max()) == 256


def test_compand_all_samples_is_the_statement():
    got, want = compress_all(ours()), A.compand(np.arange(65536))
    assert (got == want).all(), np.flatnonzero(got != want)[:8]


@needs_ref
def test_compand_all_samples_of_the_reference_is_the_statement():
    got, want = compress_all(ref()), A.compand(np.arange(65536))
    assert (got == want).all(), np.flatnonzero(got != want)[:8]


def decode_chunk_of(L, codes, bits, audio_size, start=0, slack=64):
    """one AGAC chunk holding `codes` through AGMV_DecodeAudioChunk into a zeroed track of audio_size samples (+ slack, which must
    stay zero) -> (rc, samples incl. slack, start_point)"""
    import tempfile
    libc = A.libc()
    with tempfile.NamedTemporaryFile(suffix=".agac") as tmp:
        tmp.write(b"AGAC" + struct.pack("<I", len(codes)) + bytes(codes))
        tmp.flush()
        a = L.CreateAGMV(1, 4, 4, 1)
        L.AGMV_SetBitsPerSample(a, bits)
        L.AGMV_SetAudioSize(a, audio_size)
        L.AGMV_SetTotalAudioDuration(a, 1)
        t = A.Track(a)
        (t.pcm if bits == 16 else t.pcm8)(libc.calloc(audio_size + slack, bits // 8))
        t.start_point(start)
        f = libc.fopen(tmp.name.encode(), b"rb")
        rc = L.AGMV_DecodeAudioChunk(f, a)
        libc.fclose(f)
        out = A.as_array(t.pcm() if bits == 16 else t.pcm8(), audio_size + slack, np.uint16 if bits == 16 else np.uint8)
        sp = t.start_point()
        L.DestroyAGMV(a)
    return rc, out, sp


def test_expand_all_codes_is_the_statement():
    rc, out, sp = decode_chunk_of(ours(), np.arange(256, dtype=np.uint8), 16, 256)
    assert rc == 0 and sp == 256
    assert (out[:256] == A.expand(np.arange(256))).all() and not out[256:].any()


@needs_ref
def test_expand_tables_of_the_reference_are_the_statement():
    R = O.ref()
    sqr = np.array((C.c_uint16 * 256).in_dll(R, "AGMV_SQR_TABLE"))
    shift = np.array((C.c_uint16 * 256).in_dll(R, "AGMV_SHIFT_TABLE"))
    c = np.arange(256)
    assert (np.where(c & 1, shift, sqr) == A.expand(c)).all()
    assert (sqr == (c * c).astype(np.uint16)).all() and (shift == ((c << 8) & 0xFFFF)).all()


def test_eight_bit_chunks_pass_through():
    codes = np.random.default_rng(3).integers(0, 256, 300).astype(np.uint8)
    rc, out, sp = decode_chunk_of(ours(), codes, 8, 300)
    assert rc == 0 and sp == 300 and (out[:300] == codes).all() and not out[300:].any()


@pytest.mark.parametrize("bits", (16, 8))
def test_decode_chunk_never_writes_past_audio_size(bits):
    codes = np.full(100, 0xFE, np.uint8)
    rc, out, sp = decode_chunk_of(ours(), codes, bits, 40, start=10)
    assert rc == 0 and sp == 110                                                   # start_point advances as the reference's does
    want = A.expand(codes) if bits == 16 else codes
    assert not out[:10].any() and (out[10:40] == want[:30]).all() and not out[40:].any()


def test_decode_chunk_without_a_buffer_seeks_over_the_payload(tmp_path):
    L, libc = ours(), A.libc()
    p = tmp_path / "c.agac"
    p.write_bytes(b"AGAC" + struct.pack("<I", 5) + b"\x01\x02\x03\x04\x05" + b"tail")
    libc.ftell.restype, libc.ftell.argtypes = C.c_long, [vp]
    a = L.CreateAGMV(1, 4, 4, 1)
    f = libc.fopen(str(p).encode(), b"rb")
    assert L.AGMV_DecodeAudioChunk(f, a) == 0 and libc.ftell(f) == 13 and A.Track(a).start_point() == 0
    libc.fclose(f)
    L.DestroyAGMV(a)


def test_encode_chunk_writes_zeros_past_audio_size(tmp_path):
    L, libc = ours(), A.libc()
    a = L.CreateAGMV(1, 4, 4, 1)
    L.AGMV_SetAudioSize(a, 10)
    L.AGMV_SetTotalAudioDuration(a, 1)
    t = A.Track(a)
    t.atsample(libc.calloc(10, 1))
    C.memmove(t.atsample(), bytes(range(1, 11)), 10)
    C.c_ulong.from_address(t.chunk + 8).value = 8                                  # audio_chunk->size
    f = libc.fopen(str(tmp_path / "o.bin").encode(), b"wb")
    L.AGMV_EncodeAudioChunk(f, a)
    L.AGMV_EncodeAudioChunk(f, a)
    L.AGMV_EncodeAudioChunk(f, a)
    libc.fclose(f)
    assert t.start_point() == 24
    L.DestroyAGMV(a)
    hdr = b"AGAC" + struct.pack("<I", 8)
    assert (tmp_path / "o.bin").read_bytes() == hdr + bytes(range(1, 9)) + hdr + bytes([9, 10, 0, 0, 0, 0, 0, 0]) + hdr + bytes(8)


def import_wav(L, path):
    a = L.CreateAGMV(1, 4, 4, 1)
    L.AGMV_WavToAudioTrack(str(path).encode(), a)
    t = A.Track(a)
    fields = (L.AGMV_GetTotalAudioDuration(a), L.AGMV_GetSampleRate(a), L.AGMV_GetAudioSize(a), L.AGMV_GetNumberOfChannels(a), L.AGMV_GetBitsPerSample(a))
    bits = fields[4]
    samples = A.as_array(t.pcm() if bits == 16 else t.pcm8(), fields[2], np.uint16 if bits == 16 else np.uint8)
    return a, fields, samples


WAVS = [(16, 1), (16, 2), (8, 1), (8, 2)]


@pytest.mark.parametrize("bits,channels", WAVS)
def test_wav_import(tmp_path, bits, channels):
    """header fields as the reference's; the samples the file really holds; what it does not hold is zero here"""
    n, rate = 2600, 1000
    pcm = A.tone(n, channels)
    if bits == 8:
        pcm = ((pcm.astype(np.int32) >> 8) + 128).astype(np.uint8)
    A.write_wav(tmp_path / "t.wav", pcm, rate)
    held = n * channels
    riff = 36 + held * bits // 8
    got = {}
    for name, L in libs():
        a, fields, samples = import_wav(L, tmp_path / "t.wav")
        got[name] = (fields, samples[:held].copy())
        if name == "ours":
            assert not samples[held:].any() and len(samples) - held == 36 * 8 // bits      # the RIFF size stands in for the data size
        L.DestroyAGMV(a)
    fields, samples = got["ours"]
    assert fields == (riff // (rate * channels * (bits // 8)), rate, riff if bits == 8 else riff // 2, channels, bits)
    assert (samples == pcm.reshape(-1).view(np.uint16 if bits == 16 else np.uint8)).all()
    if "reference" in got:
        assert got["reference"][0] == fields and (got["reference"][1] == samples).all()


def test_wav_import_of_a_missing_file_leaves_the_object_alone(tmp_path):
    L = ours()
    a = L.CreateAGMV(1, 4, 4, 1)
    L.AGMV_WavToAudioTrack(str(tmp_path / "none.wav").encode(), a)
    assert L.AGMV_GetTotalAudioDuration(a) == 0 and L.AGMV_GetAudioSize(a) == 0 and A.Track(a).pcm() is None
    L.DestroyAGMV(a)


def export(L, pcm, rate, kind, path):
    libc = A.libc()
    a = L.CreateAGMV(1, 4, 4, 1)
    A.set_track(L, libc, a, pcm, rate)
    f = libc.fopen(str(path).encode(), b"wb")
    L.AGMV_ExportAudioType(f, a, kind)
    libc.fclose(f)
    L.DestroyAGMV(a)
    return open(path, "rb").read()


@pytest.mark.parametrize("bits,channels", WAVS)
@pytest.mark.parametrize("kind", (A.AUDIO_WAV, A.AUDIO_AIFF, A.AUDIO_AIFC), ids=("wav", "aiff", "aifc"))
def test_export(tmp_path, kind, bits, channels):
    n, rate = 1500, 44100 if channels == 2 else 11025
    pcm = A.tone(n, channels, seed=9)
    if bits == 8:
        pcm = ((pcm.astype(np.int32) >> 8) + 128).astype(np.uint8)
    mine = export(ours(), pcm, rate, kind, tmp_path / "ours.bin")
    size, raw = n * channels, pcm.tobytes()
    if kind == A.AUDIO_WAV:
        want = (b"RIFF" + struct.pack("<I", len(raw)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, channels, rate, 75600, channels * bits // 8, bits) +
                b"data" + struct.pack("<I", len(raw)) + raw)
        assert mine == want
    else:
        assert mine[:4] == b"FORM" and mine[8:12] == (b"AIFC" if kind == A.AUDIO_AIFF else b"AIFF")      # the reference's swapped names
        body = pcm.astype(">i2").tobytes() if bits == 16 else (pcm.astype(np.int32) - 128).astype(np.int8).tobytes()
        assert mine.endswith(b"SSND" + struct.pack(">I", len(raw)) + bytes(8) + body) and struct.unpack(">I", mine[4:8])[0] == len(raw) + 32
        assert struct.pack(">HIH", channels, size // channels, bits) + {44100: b"\x40\x0E\xAC\x44", 11025: b"\x40\x0C\xAC\x44"}[rate] + bytes(6) in mine
    if O.have_ref():
        assert export(ref(), pcm, rate, kind, tmp_path / "ref.bin") == mine


def walk_chunks(L, path):
    """the Player pattern of tests/test_capi_hotpath.py: a calloc'd track, then every audio chunk through AGMV_DecodeAudioChunk"""
    libc = A.libc()
    a = L.CreateAGMV(1, 4, 4, 1)
    f = libc.fopen(path.encode(), b"rb")
    assert L.AGMV_DecodeHeader(f, a) == 0
    size, frames = L.AGMV_GetAudioSize(a), L.AGMV_GetNumberOfFrames(a)
    assert L.AGMV_GetBitsPerSample(a) == 16 and L.AGMV_GetTotalAudioDuration(a) != 0
    t = A.Track(a)
    t.pcm(libc.calloc(2 * size + 64, 2))
    t.pcm8(None)
    t.atsample(None)
    t.start_point(0)
    points = []
    for _ in range(frames):
        L.AGMV_FindNextFrameChunk(f)
        L.AGMV_SkipFrameChunk(f)
        L.AGMV_FindNextAudioChunk(f)
        assert L.AGMV_DecodeAudioChunk(f, a) == 0
        points.append((t.start_point(), t.chunk_size()))
    samples = A.as_array(t.pcm(), size, np.uint16)
    libc.fclose(f)
    L.DestroyAGMV(a)
    return size, points, samples


@pytest.mark.parametrize("path", (A.FOXLOGO, A.SPLASH), ids=("foxlogo", "splash"))
def test_golden_files_chunk_by_chunk(path):
    data = open(path, "rb").read()
    codes = A.file_codes(data)
    chunks = A.file_chunks(data)
    size, points, samples = walk_chunks(ours(), path)
    assert len(chunks) == len(points) == A.header_audio(data)[0]
    assert [p[0] for p in points] == list(np.cumsum([c[0] for c in chunks])) and [p[1] for p in points] == [c[0] for c in chunks]
    n = min(size, len(codes))
    assert n > 800000 and (samples[:n] == A.expand(codes[:n])).all() and not samples[n:].any()
    if O.have_ref():
        rsize, rpoints, rsamples = walk_chunks(ref(), path)
        assert rsize == size and rpoints == points and (rsamples[:n] == samples[:n]).all()


def test_decode_audio_writes_the_track_as_wav(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    data = open(A.FOXLOGO, "rb").read()
    frames, duration, rate, size, channels, bits = A.header_audio(data)
    codes = A.file_codes(data)
    assert len(codes) == 809445 and len(A.file_chunks(data)) == frames and A.file_chunks(data)[0][0] == 7709 and size > len(codes)
    assert ours().AGMV_DecodeAudio(A.FOXLOGO.encode(), A.AUDIO_WAV) == 0
    wav = (tmp_path / "quick_export.wav").read_bytes()
    track = np.zeros(size, np.uint16)
    track[:len(codes)] = A.expand(codes)
    want = (b"RIFF" + struct.pack("<I", size * 2) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, channels, rate, 75600, channels * bits // 8, bits) +
            b"data" + struct.pack("<I", size * 2) + track.tobytes())
    assert wav == want
    assert ours().AGMV_DecodeAudio(str(tmp_path / "none.agmv").encode(), A.AUDIO_WAV) == 2      # FILE_NOT_FOUND_ERR


@pytest.mark.parametrize("cut", ("payload", "size field", "fourcc", "frame chunk"))
def test_decode_audio_of_a_file_that_ends_early(tmp_path, monkeypatch, cut):
    """what the file holds is exported, zeros behind it, and the call returns wherever the file ends"""
    monkeypatch.chdir(tmp_path)
    data = open(A.SPLASH, "rb").read()
    third = data.find(b"AGAC", data.find(b"AGAC", data.find(b"AGAC") + 4) + 4)
    end = {"payload": third + 8 + 1000, "size field": third + 6, "fourcc": third + 2, "frame chunk": data.find(b"AGFC", third) + 9}[cut]
    (tmp_path / "cut.agmv").write_bytes(data[:end])
    _, _, _, size, channels, bits = A.header_audio(data)
    assert ours().AGMV_DecodeAudio(b"cut.agmv", A.AUDIO_WAV) == 0
    wav = (tmp_path / "quick_export.wav").read_bytes()
    codes = A.file_codes(data)
    held = len(A.file_codes(data[:third])) + {"payload": 1000, "frame chunk": A.file_chunks(data)[2][0]}.get(cut, 0)
    track = np.zeros(size, np.uint16)
    track[:held] = A.expand(codes[:held])
    assert len(wav) == 44 + 2 * size and (np.frombuffer(wav, np.uint16, offset=44) == track).all()


def test_find_chunk_returns_at_the_end_of_a_file(tmp_path):
    """the file-based chunk scan on a file that ends 1 to 3 bytes into a fourcc (the reference's loop never ends there)"""
    L, libc = ours(), A.libc()
    for tail in (b"A", b"AG", b"AGA", b"xyz", b""):
        p = tmp_path / "f.bin"
        p.write_bytes(b"0123456789" + tail)
        f = libc.fopen(str(p).encode(), b"rb")
        L.AGMV_FindNextAudioChunk(f)
        L.AGMV_FindNextFrameChunk(f)
        libc.fclose(f)


def test_the_audio_symbols_are_exported():
    L = H.lib()
    for s in ("AGMV_CompressAudio", "AGMV_SyncAudioTrack", "AGMV_SignedToUnsignedPCM", "AGMV_UnsigendToSignedPCM", "AGMV_WavToAudioTrack",
              "AGMV_RawSignedPCMToAudioTrack", "AGMV_Raw8PCMToAudioTrack", "AGMV_ExportAudioType", "AGMV_DecodeAudio",
              "AGMV_CalculateTotalAudioDuration", "AGMV_SetAudioDev", "AGMV_DecodeAudioDev"):
        assert hasattr(L, s), s
    import libagmv_amd
    assert callable(libagmv_amd.decode_audio)


def test_signed_unsigned_and_raw_importers(tmp_path):
    L, libc = ours(), A.libc()
    raw = np.random.default_rng(8).integers(0, 256, 2100).astype(np.uint8)
    buf = raw.copy()
    L.AGMV_SignedToUnsignedPCM(buf.ctypes.data_as(vp), C.c_ulong(len(buf)))
    assert (buf == raw + np.uint8(128)).all()
    L.AGMV_UnsigendToSignedPCM(buf.ctypes.data_as(vp), C.c_ulong(len(buf)))
    assert (buf == raw).all()
    (tmp_path / "s8.raw").write_bytes(raw.tobytes())
    a = L.CreateAGMV(1, 4, 4, 1)
    L.AGMV_RawSignedPCMToAudioTrack(str(tmp_path / "s8.raw").encode(), a, 2, 500)
    assert (L.AGMV_GetTotalAudioDuration(a), L.AGMV_GetSampleRate(a), L.AGMV_GetAudioSize(a), L.AGMV_GetNumberOfChannels(a), L.AGMV_GetBitsPerSample(a)) == (2, 500, 2100, 2, 8)
    assert (A.as_array(A.Track(a).pcm8(), 2100, np.uint8) == raw + np.uint8(128)).all()
    L.DestroyAGMV(a)
    a = L.CreateAGMV(1, 4, 4, 1)
    L.AGMV_Raw8PCMToAudioTrack(str(tmp_path / "s8.raw").encode(), a)
    t = A.Track(a)
    assert (L.AGMV_GetTotalAudioDuration(a), L.AGMV_GetSampleRate(a), L.AGMV_GetAudioSize(a), L.AGMV_GetNumberOfChannels(a)) == (0, 16000, 2100, 1)
    assert (A.as_array(t.satsample(), 2100, np.uint8) == raw).all()
    libc.free(t.satsample())                                                       # like the reference, DestroyAGMV leaves satsample to the caller
    t.satsample(None)
    L.DestroyAGMV(a)


def test_set_audio_dev_refusals():
    """AGMV_SetAudioDev stores its arguments: nothing is read and no device is opened, so the refusals need no GPU"""
    L = H.lib()
    p = 0x10000
    try:
        assert L.AGMV_SetAudioDev(p, 0, 48000, 48000, 2) == -1 and L.AGMV_SetAudioDev(p, 4, 48000, 48000, 2) == -1      # a bad format
        assert L.AGMV_SetAudioDev(p, A.PCM_S16, 48000, 48000, 0) == -2                                                    # 0 channels
        assert L.AGMV_SetAudioDev(p, A.PCM_F32P, 48000, 48000, 9) == -2 and L.AGMV_SetAudioDev(p, A.PCM_S16, 48000, 48000, 9) == 0
        assert L.AGMV_SetAudioDev(p, A.PCM_S16, 48000, 48000, 256) == -2 and L.AGMV_SetAudioDev(p, A.PCM_S16, 48000, 48000, 255) == 0      # the header's count is a byte
        assert L.AGMV_SetAudioDev(p, A.PCM_U8, 48000, 0, 2) == -3                                                         # a rate of 0
        assert L.AGMV_SetAudioDev(p, A.PCM_S16, 47999, 48000, 2) == -4                                                    # less than one second
        assert L.AGMV_SetAudioDev(p, A.PCM_S16, 1 << 31, 48000, 2) == -5
        assert L.AGMV_SetAudioDev(p, A.PCM_F32P, 48000, 48000, 8) == 0
    finally:
        assert L.AGMV_SetAudioDev(None, 0, 0, 0, 0) == 0                                                                  # NULL clears


def test_chunk_size_statement():
    assert A.chunk_size(5000, 16) == 312 and A.chunk_size(5000, 11) == 454 and A.chunk_size(0, 7) == 0
