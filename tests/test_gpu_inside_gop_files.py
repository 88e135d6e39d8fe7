"""A BMP driver on an object the caller began a GOP on, without any knob: AGMV_EncodeFrame fc0 times on an object under the caller's
palettes, then AGMV_EncodeFullAGMV on it.  The engine's first batch then only completes the caller's GOP (4 - fc0 frames) against the
object's I-frame entries, which the worker uploads; every later batch is whole GOPs.  tests/test_gpu_stabilise_files.py reaches that
step with the stabilisation, LZSS and the host LZ stage only.

14 frames of 64 x 48 of the golden clip, batches of 8 frames (4 - fc0, 8 and the rest), fc0 in (1, 3), LZSS and LZ77, each with the host
LZ stage and with the stage on the GPU workers (AGMV_LZ_DEVICE=1 / AGMV_LZ77_DEVICE=1).  The two stages must write the same file; every
chunk's usize and decompressed payload must be what agmv_hip_encode_frames_dev gives for the frames from frame count fc0 on, with the
palettes of the file's header and the entry plane of the caller's I-frame (agmv_hip_nearest of the caller's frame 0 under the caller's
palettes); and the chunks must differ from those of a driver that starts at frame count 0.  The drivers keep process-wide state and free
the object, so everything runs in one child process, once; this process never opens the GPU.  Needs an MI355X."""
import ctypes as C
import functools
import json
import os
import tempfile
import textwrap

import children as K
import numpy as np
import pytest

import dither_cases as D
import hostlib as H
import oracles as O

pytestmark = pytest.mark.gpu

T, W, HH, Y0, X0, BATCH = 14, 64, 48, 96, 128, 8
LZSS, LZ77 = 1, 2
FC0 = (1, 3)

CHILD = textwrap.dedent("""
    import ctypes as C, json, os, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    from libagmv_amd import seq
    L = seq.load_library()
    T, W, Hh = job["T"], job["W"], job["H"]
    L.AGMV_SetBatchFrames(job["batch"])
    libc = C.CDLL(None)
    libc.fopen.restype, libc.fopen.argtypes, libc.fclose.argtypes = C.c_void_p, [C.c_char_p, C.c_char_p], [C.c_void_p]
    host = np.load("frames.npy")
    cp0, cp1 = np.load("cp0.npy"), np.load("cp1.npy")
    wide0, wide1 = cp0.astype(np.uint64), cp1.astype(np.uint64)                 # (the header's u32 has 8 bytes)

    def drive(path, fc0, comp):
        a = L.CreateAGMV(T, W, Hh, 24)
        if fc0:                                       # the caller's own frames: under the caller's palettes, into a file of the caller's
            L.AGMV_SetOPT(a, 3)
            L.AGMV_SetCompression(a, comp)
            L.AGMV_SetICP0(a, wide0.ctypes.data)
            L.AGMV_SetICP1(a, wide1.ctypes.data)
            f = libc.fopen(b"begun.bin", b"wb")
            L.AGMV_EncodeHeader(f, a)
            for k in range(fc0):
                px = np.ascontiguousarray(host[k].reshape(-1)).astype(np.uint64)
                L.AGMV_EncodeFrame(f, a, px.ctypes.data)
            libc.fclose(f)
        L.AGMV_EncodeFullAGMV(a, path.encode(), b"fr", b"f", 1, 1, T, W, Hh, 24, 3, job["quality"], comp)

    for comp in job["compressions"]:
        for stage, value in (("host", "0"), ("device", "1")):
            os.environ["AGMV_LZ_DEVICE"] = os.environ["AGMV_LZ77_DEVICE"] = value     # (read when a sequence is opened)
            for fc0 in job["fc0"]:
                drive("inside_%d_%d_%s.agmv" % (fc0, comp, stage), fc0, comp)
        os.environ["AGMV_LZ_DEVICE"] = os.environ["AGMV_LZ77_DEVICE"] = "0"
        drive("from0_%d.agmv" % comp, 0, comp)
    # the expectation's raw streams: the frames from frame count fc0 on through agmv_hip_encode_frames_dev on a context with the palettes
    # of the file's header (38 bytes of fields, then 256 x R, G, B per palette) and the entry plane of the caller's I-frame
    frames = torch.from_numpy(host.view(np.int32)).cuda()
    for fc0 in job["fc0"]:
        data = open("inside_%d_%d_host.agmv" % (fc0, job["compressions"][0]), "rb").read()
        pal = lambda off: (np.frombuffer(data, np.uint8, 768, off).reshape(256, 3).astype(np.uint32) * np.array([65536, 256, 1], np.uint32)).sum(axis=1).astype(np.uint32)
        hip = libagmv_amd.AgmvHip(0)
        plane = hip.nearest_host(cp0, cp1, host[0], True)
        hip.set_palette(pal(38), pal(38 + 768), True)
        ient = torch.from_numpy(plane.view(np.int16).copy()).cuda()
        out, sizes = hip.encode_dev(frames, T, W, Hh, fc0, ientries=ient)
        torch.cuda.synchronize()
        hip.check()
        np.save("exp_bits_%d.npy" % fc0, out.cpu().numpy())
        np.save("exp_sizes_%d.npy" % fc0, sizes.cpu().numpy())
        hip.close()
    print(json.dumps({"done": True}))
""")


@functools.lru_cache(maxsize=None)
def clip():
    """14 frames of 64 x 48 of the golden clip (it moves)"""
    return np.ascontiguousarray(D.fox()[0][:T, Y0:Y0 + HH, X0:X0 + W])


@functools.lru_cache(maxsize=None)
def made():
    """-> ({file name: bytes}, {name: the expectation's array}); the child runs once"""
    import torch  # noqa: F401  (torch's HIP runtime in the process before the library's own, as in libagmv_amd.seq; the GPU is not opened here)
    frames = clip()
    job = {"T": T, "W": W, "H": HH, "quality": 1, "batch": BATCH, "fc0": FC0, "compressions": (LZSS, LZ77)}
    env = {"AGMV_STABILISE": None, "AGMV_DITHER": None, "AGMV_PALETTE_REFINE": None, "AGMV_TRACE": None, "AGMV_BATCH_FRAMES": None, "AGMV_DEVICES": None}
    with tempfile.TemporaryDirectory() as d:
        os.mkdir(os.path.join(d, "fr"))
        for t in range(1, T + 1):
            H.write_bmp(os.path.join(d, "fr", "f%d.bmp" % t), frames[t - 1])
        np.save(os.path.join(d, "frames.npy"), frames)
        np.save(os.path.join(d, "cp0.npy"), D.fox()[1])
        np.save(os.path.join(d, "cp1.npy"), D.fox()[2])
        r = K.start_child(d, CHILD, job, env, prelude="")
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        files = {f: open(os.path.join(d, f), "rb").read() for f in os.listdir(d) if f.endswith(".agmv")}
        exp = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.startswith("exp_")}
    return files, exp


def chunks(data):
    """-> (the file's version, [(frame number, usize, the payload's bytes, the payload decompressed, its length)] of the frame chunks of a file
    image without audio): chunk behind chunk, each payload with the writer's eight bytes behind it through the host library's LZ decoder
    into a buffer of its own"""
    buf = np.frombuffer(data, np.uint8).copy()
    info, p0, p1 = O._FileInfo(), np.zeros(256, np.uint32), np.zeros(256, np.uint32)
    assert O.oracle().orc_parse_header(buf, len(buf), C.byref(info), p0, p1) == 0
    pos, out = info.first_chunk, []
    while pos < len(buf):
        assert data[pos:pos + 4] == b"AGFC", pos
        number, usize, csize = (int.from_bytes(data[pos + o:pos + o + 4], "little") for o in (4, 8, 12))
        assert data[pos + 16 + csize:pos + 24 + csize] == b"\xff" * 8              # (the eight bytes the writer puts behind every payload)
        raw, used = np.zeros(usize + 512, np.uint8), C.c_size_t(0)
        bpos = H.lib().agmv_lz_decode_mem(info.version, np.ascontiguousarray(buf[pos + 16:pos + 24 + csize]), csize + 8, usize, csize, raw, len(raw), C.byref(used))
        out.append((number, usize, data[pos + 16:pos + 16 + csize], raw, int(bpos)))
        pos += 24 + csize
    assert pos == len(buf)
    return int(info.version), out


# What a payload keeps of its stream.  LZ77 tokens are whole bytes (offset, length, the next byte): every byte of the stream comes back, and the last
# token's next byte may be the one the encoder read behind the stream, so the decoder gives usize or usize + 1 bytes.  LZSS: csize is the bit count
# over 8, rounded down, so up to 7 bits of the last token (a literal, or a match of at most LZSS_MATCH bytes) are not in the file and the decoder reads
# the writer's 0xFF bytes for them: every byte before the last token comes back, the bytes of the last token need not.  There the payload itself is
# held, byte for byte, to the host LZSS of the expected stream, as tests/test_gpu_stabilise_files.py holds its files.
LZSS_MATCH = 15


@pytest.mark.parametrize("comp", (LZSS, LZ77), ids=("lzss", "lz77"))
@pytest.mark.parametrize("fc0", FC0)
def test_a_driver_that_starts_inside_a_gop_without_a_knob(fc0, comp):
    files, exp = made()
    host, device = files["inside_%d_%d_host.agmv" % (fc0, comp)], files["inside_%d_%d_device.agmv" % (fc0, comp)]
    assert host == device                                                         # the two LZ stages write the same file
    version, got = chunks(host)
    assert (version in (1, 2)) == (comp == LZSS), version
    bits, sizes = exp["exp_bits_%d" % fc0], exp["exp_sizes_%d" % fc0]
    assert len(got) == len(sizes) == T
    for f, (number, usize, payload, raw, bpos) in enumerate(got):
        want = bits[f, :sizes[f]]
        print("fc0 %d, compression %d, frame %d: number %d, usize %d (expected %d), csize %d, decompressed to %d bytes" % (fc0, comp, f, number, usize, sizes[f], len(payload), bpos))
        assert number == fc0 + f + 1 and usize == sizes[f], (f, number, usize, int(sizes[f]))
        kept = usize if comp == LZ77 else max(usize - LZSS_MATCH, 0)
        assert bpos >= kept and raw[:kept].tobytes() == want[:kept].tobytes(), f
        if comp == LZSS:
            packed, csize = H.lzss(want.copy())
            assert (len(payload), payload) == (csize, packed[:csize].tobytes()), f
    _, from0 = chunks(files["from0_%d.agmv" % comp])
    assert len(from0) == T and [c[1:3] for c in got] != [c[1:3] for c in from0]          # (not the file of a driver that starts at 0)

