"""The audio codec of the container stated in numpy (include/agmv.h, "audio tracks"), and what the audio tests share: the case
lists, a WAV writer, and ctypes views of an AGMV object's track that work on either library (both have the reference's layout,
tests/test_abi.py).  Nothing here touches a GPU."""
import ctypes as C
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FOXLOGO = os.path.join(HERE, "golden", "FOXLOGO.agmv")
SPLASH = os.path.join(HERE, "golden", "agmv_splash.agmv")

PCM_S16, PCM_U8, PCM_F32P = 1, 2, 3                # AGMV_PCMFMT
AUDIO_WAV, AUDIO_AIFF, AUDIO_AIFC = 1, 2, 3        # AGMV_AUDIO_TYPE

# sample counts around the 16-sample unit of the kernels' body, around a wave and a workgroup, and more than one workgroup
COUNTS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1023, 4097)
CHANNELS = (1, 2, 3, 6)


# ------------------------------------------------------------------ the statement
def compand(s):
    """uint16 samples (the WAV samples' bit patterns) -> code bytes: AGMV_CompressAudio's loop body in integers"""
    s = np.asarray(s).astype(np.int64)
    k = np.floor(np.sqrt(s.astype(np.float64))).astype(np.int64)
    k -= k * k > s
    k += (k + 1) * (k + 1) <= s
    e1 = np.where(k % 2 == 0, k, (k + 1) & 255)
    r = np.where(s > k * k + k, k + 1, k) & 255
    e2 = np.where(r % 2 == 0, r, (r + 1) & 255)
    e3 = (s >> 8) | 1
    d1, d2, d3 = np.abs(e1 * e1 - s), np.abs(e2 * e2 - s), np.abs((e3 << 8) - s)
    d = np.minimum(d1, d3)                         # the reference's second minimum overwrites its first
    return np.where(d == d1, e1, np.where(d == d2, e2, e3)).astype(np.uint8)


def expand(c):
    """code bytes -> uint16 samples: an even code is a root, an odd one the high byte"""
    c = np.asarray(c).astype(np.int64)
    return np.where(c & 1, (c << 8) & 0xFFFF, c * c).astype(np.uint16)


def from_f32(x):
    """float32 samples -> the track's uint16: clamp to [-1, 1], times 32767 in float32, round half to even, NaN is 0"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        y = np.rint(np.clip(x, np.float32(-1), np.float32(1)) * np.float32(32767))
    return np.where(np.isnan(x), np.float32(0), y).astype(np.int16).view(np.uint16)


def to_f32(u):
    return np.asarray(u, np.uint16).view(np.int16).astype(np.float32) / np.float32(32768)


def chunk_size(audio_size, frames):
    """(u32)(audio_size / (f32)frames): the size every AGAC chunk of a sequence encoder's file carries"""
    return int(np.float32(audio_size) / np.float32(frames))


def file_chunks(data):
    """[(size field, payload bytes)] of every AGAC chunk of a file image, found as AGMV_DecodeAudio walks: each frame chunk is
    skipped by its csize field, then the next 'AGAC' is looked for"""
    out, pos = [], data.find(b"AGFC")
    while pos >= 0:
        csize = struct.unpack_from("<I", data, pos + 12)[0]
        ac = data.find(b"AGAC", pos + 16 + csize)
        if ac < 0:
            break
        size = struct.unpack_from("<I", data, ac + 4)[0]
        out.append((size, data[ac + 8:ac + 8 + size]))
        pos = data.find(b"AGFC", ac + 8 + size)
    return out


def file_codes(data):
    """the codes a decoder meets, in order, as uint8"""
    return np.frombuffer(b"".join(p for _, p in file_chunks(data)), np.uint8)


def header_audio(data):
    """(frames, duration, sample_rate, audio_size, channels, bits) of a file image"""
    frames = struct.unpack_from("<I", data, 4)[0]
    duration, rate, size, channels, bits = struct.unpack_from("<IIIHH", data, 22)
    return frames, duration, rate, size, channels, bits


# ------------------------------------------------------------------ inputs
def float_cases():
    """float32 samples that meet every branch of the float rule, then 4096 seeded ones"""
    tiny = np.float32(1e-45)
    special = [1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(-1), np.float32(-2)), 1.5, -7.0, 0.0, -0.0,
               np.nan, np.inf, -np.inf, tiny, -tiny, np.float32(1e-39), np.finfo(np.float32).tiny, 0.5, -0.5, 0.25, 1.0 / 3, -1.0 / 3]
    halves = [(j + 0.5) / 32767 for j in (0, 1, 2, 3, 100, 101, 16383, 16384, 32765, 32766)]
    halves += [-h for h in halves]
    rng = np.random.default_rng(71)
    rand = np.concatenate([rng.uniform(-1.1, 1.1, 3072), rng.normal(0, 0.05, 1024)])
    return np.concatenate([np.array(special, np.float32), np.array(halves, np.float64).astype(np.float32), rand.astype(np.float32)])


def tone(n, channels, rate=1000, seed=5):
    """n sample frames of a few sines plus noise as int16 [n, channels]: every channel differs, quiet and loud parts"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None] / rate
    f = 40.0 * (1 + np.arange(channels))[None, :]
    x = 0.6 * np.sin(2 * np.pi * f * t) * np.linspace(0.05, 1, n)[:, None] + 0.05 * rng.standard_normal((n, channels))
    return np.ascontiguousarray(np.clip(np.rint(x * 32767), -32768, 32767).astype(np.int16))


def write_wav(path, pcm, rate):
    """the canonical 44-byte header and the samples of pcm: int16 [n, ch] or uint8 [n, ch]"""
    pcm = np.ascontiguousarray(pcm)
    bits, ch, raw = pcm.dtype.itemsize * 8, pcm.shape[1], pcm.tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, ch, rate, rate * ch * bits // 8, ch * bits // 8, bits))
        f.write(b"data" + struct.pack("<I", len(raw)) + raw)


# ------------------------------------------------------------------ an AGMV object's audio fields, either library
vp = C.c_void_p
OFF_AUDIO_CHUNK, OFF_AUDIO_TRACK = 4184, 4216      # AGMV.audio_chunk / .audio_track (the layout tests/test_abi.py pins)


def libc():
    L = C.CDLL(None)
    L.fopen.restype = vp
    L.fopen.argtypes = [C.c_char_p, C.c_char_p]
    L.fclose.argtypes = [vp]
    L.calloc.restype = vp
    L.calloc.argtypes = [C.c_size_t, C.c_size_t]
    L.free.argtypes = [vp]
    return L


def bind(L):
    """the API of include/agmv.h on either library"""
    import hostlib
    return hostlib.bind(L, missing_ok=True)


class Track:
    """the audio fields of an AGMV object: AGMV_AUDIO_TRACK { u32 duration, start_point; u16* pcm; u8* pcm8 } and
    AGMV_AUDIO_CHUNK { char fourcc[4]; u32 size; u8* atsample; s8* satsample }"""

    def __init__(self, a):
        self.track = vp.from_address(a + OFF_AUDIO_TRACK).value
        self.chunk = vp.from_address(a + OFF_AUDIO_CHUNK).value

    def _ptr(self, base, off, value=False):
        if value is not False:
            vp.from_address(base + off).value = value
        return vp.from_address(base + off).value

    def pcm(self, value=False):
        return self._ptr(self.track, 16, value)

    def pcm8(self, value=False):
        return self._ptr(self.track, 24, value)

    def atsample(self, value=False):
        return self._ptr(self.chunk, 16, value)

    def satsample(self, value=False):
        return self._ptr(self.chunk, 24, value)

    def start_point(self, value=None):
        if value is not None:
            C.c_ulong.from_address(self.track + 8).value = value
        return C.c_ulong.from_address(self.track + 8).value

    def chunk_size(self):
        return C.c_ulong.from_address(self.chunk + 8).value


def as_array(ptr, n, dtype):
    """a copy of n elements at a C pointer"""
    if n == 0:
        return np.zeros(0, dtype)
    ct = {np.uint8: C.c_uint8, np.uint16: C.c_uint16}[dtype]
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), (n,)).copy()


def set_track(L, libc_, a, pcm, rate):
    """the object's header fields through the setters, a buffer for the track, and the samples through AGMV_SyncAudioTrack: pcm is
    int16 / uint16 [n, ch] or uint8 [n, ch].  DestroyAGMV frees the buffer."""
    pcm = np.ascontiguousarray(pcm)
    n, ch = pcm.shape
    bits = pcm.dtype.itemsize * 8
    L.AGMV_SetBitsPerSample(a, bits)
    L.AGMV_SetAudioSize(a, n * ch)
    L.AGMV_SetSampleRate(a, rate)
    L.AGMV_SetNumberOfChannels(a, ch)
    L.AGMV_SetTotalAudioDuration(a, n // rate)
    t = Track(a)
    buf = libc_.calloc(n * ch + 64, bits // 8)
    (t.pcm if bits == 16 else t.pcm8)(buf)
    L.AGMV_SyncAudioTrack(a, pcm.ctypes.data_as(vp))
    return t
