"""Whole files with the temporal stabilisation: libagmv_amd.encode_frames(..., stabilise=s), AGMV_SetStabilise, env AGMV_STABILISE
and libagmv_amd.stabilise_stats() of libagmv_amd/libagmv.so.

Off, the file is the one the library writes without the knob: before it is set, after it was set and reset, and in a fresh
process without the variable.

On, every frame coded (AGMV_SCHEDULE_FULL), opt II and III: the file of encode_frames(X, stabilise=s) is held, chunk for chunk and
byte for byte, to the numpy statement (tests/stabilise_cases.py) applied to X and carried through agmv_hip_encode_frames_dev on a
context with the file's own palettes and the host LZSS, and its header to that of the plain file.  (The palette reads the source,
not the stabilised frames, so the file of encode_frames(statement(X)) has a palette of its own and is not the yardstick; the
frames are.)  X is 20 frames of 64 x 48 of the golden clip with noise, in batches of 8 frames: GOPs meet batch edges and both
workers take batches.  The counters must be the statement's.

The noisy still clip (tests/stabilise_cases.py) at the strength at which the statement replaces every block: every P-frame chunk
has usize = w * h / 16, with the dither beside it too, and the counters are 3 * blocks * GOPs, twice.

RGB24 and NV12 sources, the BMP driver under AGMV_SetStabilise and a fresh process under AGMV_STABILISE write the XRGB32 call's
file.  A BMP driver on an object the caller began a GOP on (AGMV_EncodeFrame 1, 2 or 3 times) leaves the frames that complete that
GOP alone, stabilises every later GOP, and counts accordingly.  Under the PDIFS and adaptive schedules the file decodes and `examined` is the P-frames written times the blocks.  The
drivers keep process-wide state, so each group runs in a child process, once; the child also encodes the expectation's frames, and
this process never opens the GPU.  Needs an MI355X."""
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
import stabilise_cases as S
import yuv_cases as Y

pytestmark = pytest.mark.gpu

T, W, HH, Y0, X0, STRENGTH, BATCH = 20, 64, 48, 96, 128, 12, 8
BLOCKS = W * HH // 16
OPT_II, OPT_III, HIGH = 2, 3, 1

CHILD = textwrap.dedent("""
    import json, sys
    import numpy as np
    import torch
    job = json.loads(sys.argv[1])
    sys.path.insert(0, job["root"])
    import libagmv_amd
    from libagmv_amd import seq
    L = seq.load_library()
    T, W, Hh, s, quality = job["T"], job["W"], job["H"], job["s"], job["quality"]
    packed = torch.from_numpy(np.load("frames.npy").view(np.int32)).cuda()
    L.AGMV_SetBatchFrames(job["batch"])
    stats = {}

    def bmp(path, strength):
        L.AGMV_SetStabilise(strength)
        L.AGMV_EncodeFullAGMV(L.CreateAGMV(T, W, Hh, 24), path.encode(), b"fr", b"f", 1, 1, T, W, Hh, 24, 3, quality, 1)
        L.AGMV_SetStabilise(0)

    if job["mode"] == "fresh":                        # with or without AGMV_STABILISE in the environment: plain calls
        libagmv_amd.encode_frames("fresh_3.agmv", packed, opt=3, quality=quality, schedule=1)
        stats["fresh_3"] = libagmv_amd.stabilise_stats()
        bmp("fresh_bmp.agmv", 0)
        stats["fresh_bmp"] = libagmv_amd.stabilise_stats()
    elif job["mode"] == "mixed":
        stats["before"] = libagmv_amd.stabilise_stats()
        for opt in (2, 3):
            libagmv_amd.encode_frames("plain_%d.agmv" % opt, packed, opt=opt, quality=quality, schedule=1)
            stats["plain_%d" % opt] = libagmv_amd.stabilise_stats()
            libagmv_amd.encode_frames("stab_%d.agmv" % opt, packed, opt=opt, quality=quality, schedule=1, stabilise=s)
            stats["stab_%d" % opt] = libagmv_amd.stabilise_stats()
            libagmv_amd.encode_frames("after_%d.agmv" % opt, packed, opt=opt, quality=quality, schedule=1)     # the knob went back
            stats["after_%d" % opt] = libagmv_amd.stabilise_stats()
            # the expectation's raw streams: the statement's frames (want.npy) through agmv_hip_encode_frames_dev on a context with
            # the palettes of the file's header (38 bytes of fields, then 256 x R, G, B per palette)
            data = open("stab_%d.agmv" % opt, "rb").read()
            pal = lambda off: (np.frombuffer(data, np.uint8, 768, off).reshape(256, 3).astype(np.uint32) * np.array([65536, 256, 1], np.uint32)).sum(axis=1).astype(np.uint32)
            p0, p1 = pal(38), pal(38 + 768) if opt == 3 else np.zeros(256, np.uint32)
            hip = libagmv_amd.AgmvHip(0)
            hip.set_palette(p0, p1, opt == 3)
            out, sizes = hip.encode_dev(torch.from_numpy(np.load("want.npy").view(np.int32)).cuda(), T, W, Hh, 0)
            torch.cuda.synchronize()
            hip.check()
            np.save("exp_bits_%d.npy" % opt, out.cpu().numpy())
            np.save("exp_sizes_%d.npy" % opt, sizes.cpu().numpy())
            np.save("exp_pal_%d.npy" % opt, np.concatenate([p0, p1]))
            hip.close()
        bmp("bmp_stab.agmv", s)
        stats["bmp_stab"] = libagmv_amd.stabilise_stats()
        bmp("bmp_plain.agmv", 0)
        p = packed.to(torch.int64)
        rgb = torch.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], dim=3).to(torch.uint8).contiguous()
        nv12 = torch.from_numpy(np.load("nv12.npy")).cuda().reshape(T, Hh * 3 // 2, W)
        stands = torch.from_numpy(np.load("nv12_stands_for.npy").view(np.int32)).cuda()
        for name, clip, kw in (("rgb24", rgb, {}), ("nv12", nv12, {"fmt": "nv12"}), ("nv12_stands_for", stands, {})):
            libagmv_amd.encode_frames(name + "_stab.agmv", clip, opt=3, quality=quality, schedule=1, stabilise=s, **kw)
        for name, schedule in (("pdifs", 2), ("adaptive", 3)):
            libagmv_amd.encode_frames(name + "_stab.agmv", packed, opt=3, quality=quality, schedule=schedule, stabilise=s)
            stats[name] = libagmv_amd.stabilise_stats()
            out, info = libagmv_amd.decode_frames(name + "_stab.agmv")
            stats[name + "_frames"] = [int(out.shape[0]), int(out.shape[1]), int(out.shape[2])]
        # a driver that starts inside a GOP: AGMV_EncodeFrame fc0 times on the object (under the caller's palettes cp0 | cp1), then
        # the BMP driver on it.  Its first batch only completes that GOP, against the object's I-frame entries.  The expectation:
        # the statement's frames from frame count fc0 on (want_in_<fc0>.npy) through agmv_hip_encode_frames_dev with the palettes
        # of the file's header and the entry plane of the caller's I-frame
        import ctypes as C
        libc = C.CDLL(None)
        libc.fopen.restype, libc.fopen.argtypes, libc.fclose.argtypes = C.c_void_p, [C.c_char_p, C.c_char_p], [C.c_void_p]
        host = np.load("frames.npy")
        cp0, cp1 = np.load("cp0.npy"), np.load("cp1.npy")
        wide0, wide1 = cp0.astype(np.uint64), cp1.astype(np.uint64)             # (the header's u32 has 8 bytes)
        for fc0 in (1, 2, 3):
            a = L.CreateAGMV(T, W, Hh, 24)
            L.AGMV_SetOPT(a, 3)
            L.AGMV_SetCompression(a, 1)
            L.AGMV_SetICP0(a, wide0.ctypes.data)
            L.AGMV_SetICP1(a, wide1.ctypes.data)
            f = libc.fopen(b"begun.bin", b"wb")
            L.AGMV_EncodeHeader(f, a)
            for k in range(fc0):
                px = np.ascontiguousarray(host[k].reshape(-1)).astype(np.uint64)
                L.AGMV_EncodeFrame(f, a, px.ctypes.data)
            libc.fclose(f)
            L.AGMV_SetStabilise(s)
            L.AGMV_EncodeFullAGMV(a, ("inside_%d.agmv" % fc0).encode(), b"fr", b"f", 1, 1, T, W, Hh, 24, 3, quality, 1)
            L.AGMV_SetStabilise(0)
            stats["inside_%d" % fc0] = libagmv_amd.stabilise_stats()
            data = open("inside_%d.agmv" % fc0, "rb").read()
            hip = libagmv_amd.AgmvHip(0)
            plane = hip.nearest_host(cp0, cp1, host[0], True)
            hip.set_palette(pal(38), pal(38 + 768), True)
            ient = torch.from_numpy(plane.view(np.int16).copy()).cuda()
            out, sizes = hip.encode_dev(torch.from_numpy(np.load("want_in_%d.npy" % fc0).view(np.int32)).cuda(), T, W, Hh, fc0, ientries=ient)
            torch.cuda.synchronize()
            hip.check()
            np.save("exp_bits_in%d.npy" % fc0, out.cpu().numpy())
            np.save("exp_sizes_in%d.npy" % fc0, sizes.cpu().numpy())
            hip.close()
    else:                                             # the noisy still clip
        for name, kw in (("still_plain", {}), ("still_stab", {"stabilise": s}), ("still_stab_dither", {"stabilise": s, "dither": 32})):
            libagmv_amd.encode_frames(name + ".agmv", packed, opt=3, quality=quality, schedule=1, **kw)
            stats[name] = libagmv_amd.stabilise_stats()
    print(json.dumps({"stats": stats}))
""")


def host_lib():
    """the host library, with torch's HIP runtime in the process before the library's own (as in libagmv_amd.seq).  This process
    never opens the GPU: the children do"""
    import torch  # noqa: F401
    return H.lib()


def run_child(cwd, job, env_extra=None):
    host_lib()
    env = dict({"AGMV_STABILISE": None, "AGMV_DITHER": None, "AGMV_PALETTE_REFINE": None, "AGMV_TRACE": None, "AGMV_BATCH_FRAMES": None}, **(env_extra or {}))
    r = K.start_child(cwd, CHILD, job, env, prelude="")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return json.loads(r.stdout.decode().strip().splitlines()[-1])["stats"], r.stderr.decode()


@functools.lru_cache(maxsize=None)
def clip():
    """20 frames of 64 x 48 of the golden clip (it moves) with Gaussian noise of 2 levels: blocks of both kinds"""
    src = np.ascontiguousarray(D.fox()[0][:T, Y0:Y0 + HH, X0:X0 + W])
    c = np.clip(D.channels(src) + np.rint(np.random.default_rng(11).normal(0.0, 2.0, src.shape + (3,))).astype(np.int64), 0, 255)
    return (c[..., 0] << 16 | c[..., 1] << 8 | c[..., 2]).astype(np.uint32)


def files_of(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in os.listdir(d) if f.endswith(".agmv")}


@functools.lru_cache(maxsize=None)
def mixed_files():
    """-> (the counters by file, {file name: bytes}, the trace of the child under AGMV_STABILISE, the expectation's arrays); run once"""
    frames = clip()
    nv12 = Y.from_packed(Y.NV12, frames, W, HH)
    job = {"T": T, "W": W, "H": HH, "s": STRENGTH, "quality": HIGH, "batch": BATCH, "mode": "mixed"}
    with tempfile.TemporaryDirectory() as d:
        os.mkdir(os.path.join(d, "fr"))
        for t in range(1, T + 1):
            H.write_bmp(os.path.join(d, "fr", "f%d.bmp" % t), frames[t - 1])
        np.save(os.path.join(d, "frames.npy"), frames)
        np.save(os.path.join(d, "nv12.npy"), nv12)
        np.save(os.path.join(d, "nv12_stands_for.npy"), Y.to_packed(Y.NV12, nv12, W, HH))
        np.save(os.path.join(d, "want.npy"), S.stabilise(frames, STRENGTH, 0)[0])
        for fc0 in (1, 2, 3):
            np.save(os.path.join(d, "want_in_%d.npy" % fc0), S.stabilise(frames, STRENGTH, fc0)[0])
        np.save(os.path.join(d, "cp0.npy"), D.fox()[1])
        np.save(os.path.join(d, "cp1.npy"), D.fox()[2])
        stats, _ = run_child(d, job)
        files = files_of(d)
        exp = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.startswith("exp_")}
        for name, env in (("off", {}), ("env", {"AGMV_STABILISE": str(STRENGTH), "AGMV_TRACE": "1"})):
            for f in files_of(d):
                os.unlink(os.path.join(d, f))
            st, trace = run_child(d, dict(job, mode="fresh"), env)
            stats.update({name + "_" + k: v for k, v in st.items()})
            files.update({name + "_" + k: v for k, v in files_of(d).items()})
    return stats, files, trace, exp


@functools.lru_cache(maxsize=None)
def still_files():
    noisy, _ = S.noisy_still_clip()
    n, h, w = noisy.shape
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "frames.npy"), noisy)
        stats, _ = run_child(d, {"T": n, "W": w, "H": h, "s": S.NOISY_STRENGTH, "quality": HIGH, "batch": 0, "mode": "still"})
        return stats, files_of(d)


def chunks(data):
    """-> (header bytes, [(usize, csize, payload bytes)] of the frame chunks, (p0, p1)) of a file image without audio"""
    L = O.oracle()
    buf = np.frombuffer(data, np.uint8).copy()
    info, p0, p1 = O._FileInfo(), np.zeros(256, np.uint32), np.zeros(256, np.uint32)
    assert L.orc_parse_header(buf, len(buf), C.byref(info), p0, p1) == 0
    pos, out = info.first_chunk, []
    while pos < len(buf):
        assert L.orc_find_next_frame_chunk(buf, len(buf), pos) == pos             # chunk behind chunk, nothing between
        usize, csize = (int.from_bytes(data[pos + o:pos + o + 4], "little") for o in (8, 12))
        out.append((usize, csize, data[pos + 16:pos + 16 + csize]))
        assert data[pos + 16 + csize:pos + 24 + csize] == b"\xff" * 8                # (the eight bytes the writer puts behind every payload)
        pos += 24 + csize
    assert pos == len(buf)
    return data[:info.first_chunk], out, (p0, p1)


def frame_chunks(data):
    """the number of frame chunks of a file image, whatever lies between them (the PDIFS driver writes audio chunks of size 0)"""
    L = O.oracle()
    buf = np.frombuffer(data, np.uint8).copy()
    n, pos = 0, L.orc_find_next_frame_chunk(buf, len(buf), 0)
    while pos + 16 <= len(buf):
        n += 1
        pos = L.orc_find_next_frame_chunk(buf, len(buf), pos + 24 + int.from_bytes(data[pos + 12:pos + 16], "little"))
    return n


def expected_chunks(bits, sizes):
    """the raw streams of the expectation through the host LZSS, as the chunks' fields"""
    res = []
    for f in range(len(sizes)):
        payload, csize = H.lzss(bits[f, :sizes[f]].copy())
        res.append((int(sizes[f]), csize, payload[:csize].tobytes()))
    return res


@pytest.mark.parametrize("opt", (OPT_II, OPT_III), ids=("opt2", "opt3"))
def test_off_changes_nothing(opt):
    stats, files, _, _ = mixed_files()
    assert files["after_%d.agmv" % opt] == files["plain_%d.agmv" % opt]           # a call without `stabilise` after one with it: the knob went back
    assert files["stab_%d.agmv" % opt] != files["plain_%d.agmv" % opt]
    assert stats["before"] == stats["plain_%d" % opt] == stats["after_%d" % opt] == [0, 0]
    if opt == OPT_III:
        assert files["off_fresh_3.agmv"] == files["plain_3.agmv"]                 # a fresh process without the variable
        assert files["off_fresh_bmp.agmv"] == files["bmp_plain.agmv"] == files["plain_3.agmv"]
        assert stats["off_fresh_3"] == stats["off_fresh_bmp"] == [0, 0]


@pytest.mark.parametrize("opt", (OPT_II, OPT_III), ids=("opt2", "opt3"))
def test_the_file_is_the_statement_through_the_encoder(opt):
    stats, files, _, made = mixed_files()
    want, examined, replaced = S.stabilise(clip(), STRENGTH, 0)
    assert 0 < replaced < examined == (T - T // 4) * BLOCKS
    assert stats["stab_%d" % opt] == [examined, replaced]
    head, got, pal = chunks(files["stab_%d.agmv" % opt])
    assert head == chunks(files["plain_%d.agmv" % opt])[0]                        # the palette reads the source
    assert np.concatenate(pal).tolist()[:512 if opt == OPT_III else 256] == made["exp_pal_%d" % opt].tolist()[:512 if opt == OPT_III else 256]
    exp = expected_chunks(made["exp_bits_%d" % opt], made["exp_sizes_%d" % opt])
    assert len(got) == len(exp) == T
    for f in range(T):
        assert got[f][:2] == exp[f][:2] and got[f][2] == exp[f][2], (f, got[f][:2], exp[f][:2])
    plain = chunks(files["plain_%d.agmv" % opt])[1]
    print("opt %d, strength %d: %d of %d blocks replaced; stream bytes %d -> %d, file bytes %d -> %d" % (
        opt, STRENGTH, replaced, examined, sum(c[0] for c in plain), sum(c[0] for c in got), len(files["plain_%d.agmv" % opt]), len(files["stab_%d.agmv" % opt])))


def test_the_noisy_still_clip_is_copy_flags():
    stats, files = still_files()
    noisy, _ = S.noisy_still_clip()
    n, h, w = noisy.shape
    _, examined, replaced = S.stabilise(noisy, S.NOISY_STRENGTH, 0)
    assert examined == replaced == 3 * (w * h // 16) * (n // 4)
    assert stats["still_plain"] == [0, 0]
    for name in ("still_stab", "still_stab_dither"):
        assert stats[name] == [examined, replaced], name
        got = chunks(files[name + ".agmv"])[1]
        assert [c[0] for k, c in enumerate(got) if k & 3] == [w * h // 16] * (n - n // 4), name
    plain, stab = chunks(files["still_plain.agmv"])[1], chunks(files["still_stab.agmv"])[1]
    assert all(c[0] > w * h // 16 for k, c in enumerate(plain) if k & 3)
    assert [c for k, c in enumerate(stab) if not k & 3] == [c for k, c in enumerate(plain) if not k & 3]       # I-frames are untouched
    print("noisy still clip, sigma %d, strength %d: stream bytes %d -> %d, file bytes %d -> %d" % (
        S.NOISY_SIGMA, S.NOISY_STRENGTH, sum(c[0] for c in plain), sum(c[0] for c in stab), len(files["still_plain.agmv"]), len(files["still_stab.agmv"])))


def test_other_sources_and_the_bmp_driver_write_the_same_file():
    stats, files, _, _ = mixed_files()
    assert files["rgb24_stab.agmv"] == files["stab_3.agmv"]
    assert files["nv12_stab.agmv"] == files["nv12_stands_for_stab.agmv"]          # ... as its XRGB32 image
    assert files["nv12_stab.agmv"] != files["plain_3.agmv"]
    assert files["bmp_stab.agmv"] == files["stab_3.agmv"] and stats["bmp_stab"] == stats["stab_3"]


def test_fresh_process_under_the_environment_knob():
    stats, files, trace, _ = mixed_files()
    assert files["env_fresh_3.agmv"] == files["stab_3.agmv"] and files["env_fresh_bmp.agmv"] == files["stab_3.agmv"]
    assert stats["env_fresh_3"] == stats["env_fresh_bmp"] == stats["stab_3"]
    assert "temporal stabilisation" in trace and "strength %d" % STRENGTH in trace, trace[-1500:]
    assert "%d of %d P-frame blocks" % (stats["stab_3"][1], stats["stab_3"][0]) in trace, trace[-1500:]     # AGMV_TRACE prints the two counts


@pytest.mark.parametrize("fc0", (1, 2, 3))
def test_a_driver_that_starts_inside_a_gop(fc0):
    """AGMV_EncodeFrame fc0 times on the object, then AGMV_EncodeFullAGMV under AGMV_SetStabilise: the first batch only completes the
    caller's GOP and has no anchor, every later batch is whole GOPs from frame count 4, 12, 20 on"""
    stats, files, _, made = mixed_files()
    want, examined, replaced = S.stabilise(clip(), STRENGTH, fc0)
    lead = 4 - fc0
    assert (want[:lead] == clip()[:lead]).all() and 0 < replaced < examined == (T - lead - (T - lead + 3) // 4) * BLOCKS
    assert stats["inside_%d" % fc0] == [examined, replaced]
    _, got, _ = chunks(files["inside_%d.agmv" % fc0])
    exp = expected_chunks(made["exp_bits_in%d" % fc0], made["exp_sizes_in%d" % fc0])
    assert len(got) == len(exp) == T
    for f in range(T):
        assert got[f][:2] == exp[f][:2] and got[f][2] == exp[f][2], (f, got[f][:2], exp[f][:2])
    assert [c[:2] for c in got] != [c[:2] for c in chunks(files["bmp_stab.agmv"])[1]]      # (not the file of a driver that starts at 0)


@pytest.mark.parametrize("schedule", ("pdifs", "adaptive"))
def test_the_other_schedules_decode_and_count_their_p_frames(schedule):
    stats, files, _, _ = mixed_files()
    n, h, w = stats[schedule + "_frames"]
    written = frame_chunks(files[schedule + "_stab.agmv"])                       # (the schedule decides how many frames are coded)
    assert (h, w) == (HH, W) and 1 <= n <= written
    examined, replaced = stats[schedule]
    assert examined == (written - (written + 3) // 4) * BLOCKS and 0 <= replaced <= examined
